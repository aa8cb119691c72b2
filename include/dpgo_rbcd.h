/*
 * dpgo_rbcd.h -- pose-graph inputs and the multi-agent RBCD round engine (libdpgo_hip.so).
 *
 * Graph side (host C++):
 *   dpgo_graph_read_g2o      read_g2o_file            src/DPGO_utils.cpp:78-212 (+ SURVEY App. B fixes)
 *   dpgo_graph_laplacian_bsr constructConnectionLaplacianSE  src/DPGO_utils.cpp:214-286
 *   dpgo_graph_grid3d        synthetic 3D grid (replaces the missing g2o100k/1M inputs)
 *   dpgo_graph_chain_init    odometryInitialization   src/DPGO_utils.cpp:426-447, lifted by YLift
 *
 * Engine side: N PGOAgents partitioned over ranks (one process per GPU).  Per RBCD iteration
 * one colour class of the agent-adjacency graph is "selected" (doOptimization = true,
 * src/PGOAgent.cpp:642-718); all other agents run iterate(false).  Selected agents on a GPU are
 * solved as ONE batched dpgo_hip_problem (their Q blocks are independent).  Neighbour public poses
 * cross ranks either through the library's own RCCL exchange (dpgo_rbcd_comm_init / dpgo_rbcd_exchange)
 * or through caller-owned device buffers the caller moves itself (dpgo_rbcd_pack, then e.g. an RCCL
 * all_to_all, then dpgo_rbcd_update); same-rank neighbours are read directly from device memory.
 * Robust cost: L2 (default, the throughput setting) or any of the reference's RobustCostType with
 * on-device loop-closure reweighting every robust_opt_inner_iters iterations (PGOAgent::iterate +
 * updateLoopClosuresWeights, src/PGOAgent.cpp:642-718, 1174-1244; RobustCost, src/DPGO_robust.cpp).
 */
#ifndef DPGO_RBCD_H
#define DPGO_RBCD_H

#include "dpgo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dpgo_graph_s* dpgo_graph;
typedef struct dpgo_rbcd_s* dpgo_rbcd;

/* ---- pose graphs --------------------------------------------------------------------------*/
int dpgo_graph_read_g2o(const char* path, dpgo_graph* out);
int dpgo_graph_grid3d(int k, unsigned long long seed, double rot_sigma, double trans_sigma,
                      dpgo_graph* out);
int dpgo_graph_from_arrays(int d, int n, int m, const int* p1, const int* p2, const double* R,
                           const double* t, const double* kappa, const double* tau, dpgo_graph* out);
/* d, n = max pose index + 1, m = #edges, duplicates = #repeated (p1,p2) pairs */
int dpgo_graph_info(dpgo_graph g, int* d, int* n, int* m, int* duplicates);
/* R row-major d*d per edge, t d per edge; any output may be NULL */
int dpgo_graph_copy_out(dpgo_graph g, int* p1, int* p2, double* R, double* t, double* kappa,
                        double* tau);
int dpgo_graph_destroy(dpgo_graph g);
/* Whole-graph Q as BSR (block (j, bcol) column-major).  Call with browptr == NULL to get nnzb. */
int dpgo_graph_laplacian_bsr(dpgo_graph g, long long* nnzb, int* browptr, int* bcol, double* blocks);
/* X = YLift * T_odo, T_odo composed along the p2 = p1 + 1 edges (r x (d+1) n, column-major). */
int dpgo_graph_chain_init(dpgo_graph g, int r, const double* YLift_colmajor, double* X_out);
/* chordalInitialization (src/DPGO_utils.cpp:377-424, PGOAgent::localInitialization for the L2 cost):
 * rotations by least squares with R_0 = I then projectToRotationGroup, translations by least squares
 * with t_0 = 0 (normal equations by a host block Cholesky; the reference uses SPQR, same minimiser).
 * Host-only.  T_out: d x (d+1) n column-major ([R_i | t_i] per pose); R d*d row-major per edge. */
int dpgo_chordal_initialization(int d, int n, int m, const int* p1, const int* p2, const double* R,
                                const double* t, const double* kappa, const double* tau, double* T_out);
/* X = YLift * chordal T for a graph handle (r x (d+1) n, column-major). */
int dpgo_graph_chordal_init(dpgo_graph g, int r, const double* YLift_colmajor, double* X_out);
/* chordalInitialization with both linear solves by Jacobi-preconditioned CG on the GPU (for graphs
 * whose direct factor is too large: a 10^6-pose 3D grid): each right-hand side to |r| <= rtol |b|
 * (DPGO_HIP_EDEVICE if max_iters is not enough).  iters: PCG iterations of both solves; relres: the
 * largest final relative residual.  Same system assembly and projections as the host version. */
int dpgo_chordal_initialization_gpu(int d, int n, int m, const int* p1, const int* p2, const double* R,
                                    const double* t, const double* kappa, const double* tau, double rtol,
                                    int max_iters, double* T_out, int* iters, double* relres);
int dpgo_graph_chordal_init_gpu(dpgo_graph g, int r, const double* YLift_colmajor, double rtol, int max_iters,
                                double* X_out, int* iters, double* relres);
/* The multi-robot initialisation: PGOAgent::localInitialization on every agent (chordal on its private
 * graph, src/PGOAgent.cpp:947-962; anchored at the agent's breadth-first centre pose instead of its
 * first pose -- the unconstrained rotation relaxation shrinks with graph distance from the anchor)
 * then initializeInGlobalFrame (:369-432): agents join the frame of the agent holding pose 0 in
 * breadth-first order, each by the L2 average over its shared loop closures with agents already in
 * the frame (the reference averages with GNC-TLS; identical on outlier-free data: with outlier loop closures
 * use dpgo_graph_distributed_init_ex and DPGO_ALIGN_ROBUST_TWO_STAGE below).  use_gpu: the
 * block-diagonal chordal systems by Jacobi-PCG on the device (rtol, max_iters), else host Cholesky.
 * X_out = YLift * T (r x (d+1) n, column-major). */
int dpgo_graph_distributed_init(dpgo_graph g, int num_agents, const int* agent_of_pose, int r,
                                const double* YLift_colmajor, int use_gpu, double rtol, int max_iters, double* X_out,
                                int* iters, double* relres);
/* robustSingleRotationAveraging (src/DPGO_utils.cpp:582-644), host-only: GNC-TLS over the chordal mean of n rotations
 * (R row-major d*d per item; kappa NULL = all ones).  The initial estimate is the L2 chordal mean projected to SO(d);
 * mu_0 = min(c^2 / (2 max r^2 - c^2), 1e-5) with c = threshold and r_i^2 = kappa_i |R_opt - R_i|_F^2, and GNC is
 * skipped when mu_0 <= 0; per iteration the kappa .* w weighted mean is solved, the weights follow RobustCost::weight
 * for GNC_TLS (src/DPGO_robust.cpp:49-61), the loop stops when every weight is within 1e-8 of 0 or 1, else
 * mu <- mu_step mu (at most max_iters iterations; the reference: 1000 and 1.4).  R_opt (row-major) is the estimate
 * solved with the weights of the iteration BEFORE the final reweighting, as in the reference: converged outliers
 * leave a small trace in it.  weights[n]: the final weights (inliers: > 1 - 1e-8); iters (may be NULL): GNC iterations
 * run.  DPGO_HIP_EINVAL for n <= 0, d not 2 or 3, null R / R_opt / weights, or an item that is not a rotation to 1e-8
 * (determinant and |R^T R - I|_F; the reference asserts this). */
int dpgo_robust_rotation_average(int d, int n, const double* R, const double* kappa, double threshold, int max_iters,
                                 double mu_step, double* R_opt, double* weights, int* iters);
/* The multi-robot initialisation with the reference's choices under a robust cost, as per-agent local trajectories
 * plus one frame per agent (dpgo_rbcd_set_trajectory takes exactly these; dpgo_hip_frame_lift lifts them). */
#define DPGO_LOCAL_CHORDAL 0  /* chordal on the agent's private graph (the L2 cost's localInitialization) */
#define DPGO_LOCAL_ODOMETRY 1 /* odometryInitialization: what localInitialization does under any robust cost */
#define DPGO_ALIGN_L2 0               /* dpgo_graph_distributed_init's average over every shared closure */
#define DPGO_ALIGN_ROBUST_TWO_STAGE 1 /* computeRobustNeighborTransformTwoStage (src/PGOAgent.cpp:290-331) */
#define DPGO_ALIGN_PCM 2              /* the maximum set of pairwise consistent candidates (build-defined, below) */
typedef struct {
  int local_init;            /* DPGO_LOCAL_* (default CHORDAL) */
  int align;                 /* DPGO_ALIGN_* (default L2) */
  double max_rotation_error; /* GNC-TLS threshold, chordal: 2 sqrt(2) sin(0.25) = angular2ChordalSO3(0.5), ~30 deg */
  int gnc_max_iters;         /* 1000 */
  double gnc_mu_step;        /* 1.4 */
  int use_gpu;               /* chordal solves by Jacobi-PCG on the device (default 0: host Cholesky) */
  double rtol;               /* 1e-12 (use_gpu) */
  int max_iters;             /* 20000 (use_gpu) */
  /* pairwise consistency (DPGO_ALIGN_PCM, dpgo_graph_pcm); c_R is max_rotation_error */
  double max_translation_error; /* c_t; 0 = unset: PCM then refuses (the reference has no value for it) */
  long long clique_node_budget; /* dpgo_max_clique's node_budget per group (default 10,000,000; < 0: no limit) */
} dpgo_init_params;
void dpgo_default_init_params(dpgo_init_params* p);
/* LOCAL_ODOMETRY: each agent composes its odometry edges (both poses in the agent at consecutive local indices,
 * dpgo_rbcd_weight_owner's rule) from its first pose = identity; DPGO_HIP_EINVAL naming the agent when they do not
 * reach all of its poses (contiguous pose ranges, as in MultiRobotExample, are the supported partitions; the grid's
 * sub-cubes also qualify, the snake order within a sub-cube being a path of lattice neighbours).
 * ALIGN_ROBUST_TWO_STAGE: breadth-first from the agent holding pose 0, neighbours in ascending id; a new agent A is
 * aligned to the single agent being dequeued (the reference's one neighborID): per shared closure with it the
 * candidate frame is computeNeighborTransform's (:250-288), W_A-pose T_local(A-pose)^-1 with W_A-pose =
 * W_parent-pose T_e (T_e^-1 for an edge leaving A); the rotation is dpgo_robust_rotation_average of the candidates
 * (unit kappa, max_rotation_error), the translation the plain mean of the inlier candidates' translations.  An empty
 * inlier set skips the pair and A waits for another aligned neighbour; DPGO_HIP_EINVAL if an agent is never aligned.
 * ALIGN_PCM (build-defined, absent from the reference): the breadth-first order, the single parent and the candidate
 * frames of ALIGN_ROBUST_TWO_STAGE; the candidates of a (parent, child) pair are one group of
 * dpgo_hip_pair_consistency (include/dpgo_hip.h) with the child's closure pose in its local frame as the lever point,
 * c_R = max_rotation_error and c_t = max_translation_error (DPGO_HIP_EINVAL naming the field while that is unset);
 * the inlier set is dpgo_max_clique of the group (clique_node_budget); the rotation is the chordal L2 mean of the
 * clique's rotations projected to SO(d) (ALIGN_L2's mean with unit weights, on that subset, in candidate order), the
 * translation the plain mean of the clique's translations.  A single candidate is a clique of one: the agent is
 * aligned on that closure alone, and so is an agent whose candidates are all mutually inconsistent (on the lowest
 * index among the highest degrees: the greedy incumbent).  use_gpu = 1 runs the pair tests by the kernel, 0 by the
 * host twin: the same bits either way.
 * ALIGN_L2 with LOCAL_CHORDAL: frame o local is dpgo_graph_distributed_init's trajectory, bitwise.
 * Outputs: T_local d x (d+1) n column-major (each agent in its own frame); frames num_agents x d x (d+1) column-major
 * (identity for the root); parent[num_agents] (-1 for the root); candidates / inliers [num_agents] (0 for the root);
 * edge_inlier[m] (may be NULL): 1 an inlier candidate, 0 a rejected one, 255 not used as a candidate; iters / relres
 * (may be NULL): the chordal solves' PCG iterations and largest relative residual (0 otherwise). */
int dpgo_graph_distributed_init_ex(dpgo_graph g, int num_agents, const int* agent_of_pose,
                                   const dpgo_init_params* params, double* T_local, double* frames, int* parent,
                                   int* candidates, int* inliers, unsigned char* edge_inlier, int* iters,
                                   double* relres);
/* Pairwise consistent measurement set (PCM) over the inter-agent loop closures of the whole graph (build-defined,
 * DESIGN 3.17 and 7 item 17).  Every unordered agent pair A < B with shared closures is one group of
 * dpgo_hip_pair_consistency; closure k between pose a_k of A and pose b_k of B gives the candidate
 * F_k = T_local(a_k) Z_k T_local(b_k)^-1 (Z_k^-1 when the edge leaves B): B's local frame in A's, with the lever point
 * x_k = the translation of T_local(b_k).  T_local: d x (d+1) n column-major, each agent in its own frame
 * (dpgo_graph_distributed_init_ex's output).  params (NULL = defaults, which refuse: max_translation_error is unset):
 * max_rotation_error = c_R, max_translation_error = c_t, clique_node_budget, use_gpu (1: the kernel, one launch over
 * all groups; 0: the host twin; the same bits).  edge_inlier[m]: 1 a member of its group's maximum clique
 * (dpgo_max_clique), 0 a rejected shared closure, 255 an edge inside one agent.  A group of one closure is trivially
 * consistent: its closure gets 1.  info (may be NULL): see below. */
typedef struct {
  int groups;               /* agent pairs with shared closures */
  long long candidates;     /* shared closures */
  long long pair_tests;     /* sum over groups of m_g^2 */
  long long inliers;        /* entries of edge_inlier equal to 1 */
  double min_clique_ratio;  /* the smallest clique size / group size (1 without groups) */
  int unproven;             /* groups whose clique search ended on the node budget */
} dpgo_pcm_info;
int dpgo_graph_pcm(dpgo_graph g, int num_agents, const int* agent_of_pose, const double* T_local,
                   const dpgo_init_params* params, unsigned char* edge_inlier, dpgo_pcm_info* info);
/* Grid graphs: agent = sub-cube (x/s, y/s, z/s), s = k / A; id = ax + A (ay + A az). */
/* Certified optimality gap of an iterate X (r x (d+1) n, column-major, e.g. the engine's
 * dpgo_rbcd_get_X gathered over ranks) for the whole graph's central Q (unit weights): lambda_min of
 * the certificate matrix S(X) = Q - Lambda(X) (dpgo_hip_certify), f_relax = f(X), and f_rounded =
 * f of X rounded to SE(d) as PGOAgent::getTrajectoryInLocalFrame does (src/PGOAgent.cpp:481-498;
 * T_rounded: d x (d+1) n, optional; eigvec: the Ritz vector of lambda_min, r x (d+1) n, optional).
 * lambda_min >= -eps certifies f_relax <= f* <= f_rounded.
 * Not in the reference (parity-unpinned against it; pinned against the oracle's explicit S). */
int dpgo_graph_certify(dpgo_graph g, int r, const double* X, int max_iters, double tol, double* lambda_min,
                       double* residual, int* iters, double* f_relax, double* f_rounded, double* T_rounded,
                       double* eigvec);
/* The same through dpgo_hip_certify_ex (thick restart with basis_max, DPGO_CERT_SEED_X, the bound in info). */
int dpgo_graph_certify_ex(dpgo_graph g, int r, const double* X, int max_iters, int basis_max, int flags, double tol,
                          double* lambda_min, double* f_relax, double* f_rounded, double* T_rounded, double* eigvec,
                          dpgo_cert_info* info);
/* The certificate by factorisation (dpgo_hip_certify_chol_ex) on the whole graph's central edge-stream handle with
 * the weights w (per edge in the graph's order; NULL: ones).  dpgo_rbcd_get_weights' array gives the certificate of
 * the problem a robust run solved: S(X) is then the weighted Q's.  f_relax (optional) = f(X) with the same
 * weights.  eigvec (optional, r x (d+1) n) as dpgo_graph_escape takes it, untouched when info->certified. */
int dpgo_graph_certify_chol(dpgo_graph g, int r, const double* X, const double* w, double eta,
                            const dpgo_chol_cert_params* p, double* lambda_min, double* eigvec, double* f_relax,
                            dpgo_chol_cert_info* info);
/* The block certificate (dpgo_hip_certify_block) on the whole graph's central edge-stream handle with the weights w
 * (per edge in the graph's order; NULL: ones), the shape of dpgo_graph_certify_chol: any graph size, and with a
 * robust run's final weights the certificate of the problem that run solved.  f_relax (optional) = f(X) with the
 * same weights, evaluated first, so an error leaves every output untouched. */
int dpgo_graph_certify_block(dpgo_graph g, int r, const double* X, const double* w, const dpgo_block_cert_params* p,
                             double* lambda_min, double* eigvec, double* f_relax, dpgo_cert_info* info);
/* The rank staircase's step for the whole graph, next to dpgo_graph_certify_ex: when that returned lambda_min < 0
 * at a critical point X of rank r, X_out ((r+1) x (d+1) n, column-major) = dpgo_hip_escape on the central
 * unit-weight edge-stream handle at rank r + 1, along dpgo_hip_escape_direction of eigvec_or_v (vec_rows x (d+1) n,
 * column-major: the certificate's eigvec with vec_rows = r, or a plain eigenvector with vec_rows = 1).  X_out then
 * starts a solver at rank r + 1 (dpgo_rbcd_set_X of an engine created with params.r = r + 1).  DPGO_HIP_EINVAL for
 * r = 8, r < d, lambda_min >= 0 or a zero direction. */
int dpgo_graph_escape(dpgo_graph g, int r, const double* X, const double* eigvec_or_v, int vec_rows,
                      double lambda_min, const dpgo_escape_params* params, double* X_out, dpgo_escape_info* info);
/* The way down again, next to dpgo_graph_escape: truncate X (r x (d+1) n, column-major) to its numerical rank.  X is
 * uploaded once; dpgo_hip_gram_dev, dpgo_hip_gram_eig on the r x r Gram, *k = max(d, #{i : w_i > tol w_1}), then
 * dpgo_hip_rank_reduce_dev along the leading k eigenvectors into X_out (k x (d+1) n, column-major; the caller
 * provides room for r x (d+1) n).  info: the Gram's eigenvalues (w[r..8) = NaN), dropped = sum_{i > k} w_i, and f of
 * X and of X_out through the central unit-weight edge-stream handles of rank r and k, as dpgo_graph_escape gets
 * its f.  When k = r nothing is truncated: X_out = X, dropped = 0, f_after = f_before, DPGO_HIP_OK.  X_out then
 * starts a solver at rank k (dpgo_rbcd_set_X of an engine created with params.r = k).  DPGO_HIP_EINVAL for an
 * unsupported r, tol outside [0, 1), or a null argument. */
typedef struct {
  double w[8];      /* eigenvalues of sum_j Y_j Y_j^T, descending */
  double dropped;   /* sum_{i > k} w_i = sum_j |(I - W W^T) Y_j|_F^2 */
  double f_before;  /* f(X) at rank r */
  double f_after;   /* f(X_out) at rank k */
} dpgo_rank_info;
int dpgo_graph_rank_reduce(dpgo_graph g, int r, const double* X, double tol, int* k, double* X_out,
                           dpgo_rank_info* info);
/* dpgo_hip_edge_errors (include/dpgo_hip.h) over the graph's own measurements: X r x (d+1) n column-major at any
 * compiled r >= d -- a lifted solution or, at r = d, a rounded trajectory (dpgo_hip_round_se, dpgo_rbcd_get_trajectory)
 * -- and w per edge in the graph's order (NULL = ones; dpgo_rbcd_get_weights' array gives the cost a robust run
 * minimised).  err, rot_sq, tra_sq (m each) and cost (1) may each be NULL, not all.  With the weights Q was built
 * from, *cost = f(X).  The caller compares err against its own threshold (barc^2). */
int dpgo_graph_edge_errors(dpgo_graph g, int r, const double* X, const double* w,
                           double* err, double* rot_sq, double* tra_sq, double* cost);
int dpgo_graph_grid_partition(dpgo_graph g, int agents_per_axis, int* agent_of_pose);

/* ---- evaluation against a ground truth (build-defined; dpgo_hip_traj_* in include/dpgo_hip.h) ----
 * The poses dpgo_graph_grid3d(k, seed, ..) measured: rotation i from the first 4 n normals of the seed's stream, the
 * translation its lattice coordinates.  T_out: 3 x 4 n column-major, 12 doubles per pose [R_i | t_i]; bitwise the
 * oracle's grid3d(...).extra["ground_truth"].  Host only.  DPGO_HIP_EINVAL for k outside [2, 200] or a null T_out. */
int dpgo_graph_grid3d_truth(int k, unsigned long long seed, double* T_out);
/* The VERTEX_SE2 (id x y theta) and VERTEX_SE3:QUAT (id x y z qx qy qz qw) lines of a g2o file as a reference
 * trajectory of n poses, T_out d x (d+1) n column-major (the id's low 48 bits index the pose, as for the edges).
 * The quaternion is normalised before it becomes a rotation -- unlike the edge reader's, which keeps the
 * reference's unnormalised Eigen conversion -- because a reference pose must be a rotation.  present (n ints, may
 * be NULL) is 1 for the ids the file gave; an absent pose has present = 0 and NaN in all its d (d+1) entries (a
 * later line of the same id replaces an earlier one).  Host only.  DPGO_HIP_EINVAL for an unreadable file, d
 * outside {2, 3}, n <= 0, a vertex line of the other dimension, a zero quaternion, or an id >= n; the outputs are
 * then untouched. */
int dpgo_g2o_read_vertices(const char* path, int d, int n, double* T_out, int* present);
#define DPGO_ALIGN_NONE 0 /* compare as given */
#define DPGO_ALIGN_POSE 1 /* A = R_p R^_p^T, a = t_p - A t^_p of the pose `pose` */
#define DPGO_ALIGN_LSQ 2  /* dpgo_hip_traj_align over the used poses */
typedef struct {
  double count;        /* used poses */
  double Aa[12];       /* [A | a], d x (d+1) column-major */
  double sigma[3];     /* dpgo_align_info's (NaN unless DPGO_ALIGN_LSQ) */
  int rank;            /* dpgo_align_info's (-1 unless DPGO_ALIGN_LSQ) */
  double ate_rmse, ate_max;  /* sqrt(mean tra_sq), sqrt(max tra_sq) over the used poses */
  double rot_rmse, rot_max;  /* the same of the chordal rot_sq */
  double rpe_tra_rmse, rpe_rot_rmse;  /* sqrt(mean) of the RPE residuals over the edges used */
  double edges_used;   /* edges with both endpoints used */
} dpgo_eval_info;
/* A solution X (r x (d+1) n column-major, any compiled r >= d) of the graph against the truth T_truth
 * (d x (d+1) n), everything on the device after one upload: r > d is rounded by dpgo_hip_round_se_dev in the frame
 * of X's pose `pose` (r = d is taken as it is), aligned as `align` says, dpgo_hip_traj_errors_dev gives tra_sq and
 * rot_sq per pose (n each), dpgo_hip_relative_poses_dev the truth's relative poses over the graph's own edges, and
 * dpgo_hip_edge_errors_dev at r = d with kappa = tau = 1 the RPE residuals rpe_rot_sq and rpe_tra_sq per edge (m
 * each).  The RPE means are that kernel's cost with (kappa, tau) = (1, 0) and (0, 1) over the edges whose
 * endpoints are both used: deterministic.  The other edges are left out of the launch (as if they had weight 0,
 * but a truth that is NaN at its unused poses cannot reach the sums) and get NaN per edge.  use as in
 * dpgo_hip_traj_errors; every per-item array may be NULL.  DPGO_HIP_EINVAL for a null g, X, T_truth or info, an
 * unsupported r, an unknown align, pose outside [0, n), or DPGO_ALIGN_POSE on an unused pose. */
int dpgo_graph_evaluate(dpgo_graph g, int r, const double* X, const double* T_truth, const int* use, int align,
                        int pose, dpgo_eval_info* info, double* tra_sq, double* rot_sq, double* rpe_rot_sq,
                        double* rpe_tra_sq);

/* ---- RBCD engine ----------------------------------------------------------------------------*/
typedef struct {
  int r;                  /* relaxation rank */
  int acceleration;       /* Nesterov (PGOAgentParameters::acceleration) */
  int restart_interval;   /* 30 */
  int max_inner;          /* tCG iterations per update (10, src/PGOAgent.cpp:1135) */
  double initial_radius;  /* 100 (src/PGOAgent.cpp:1136) */
  double tolerance;       /* 1e-2 (src/PGOAgent.cpp:1133) */
  int precon;             /* DPGO_PRECON_BLOCK_JACOBI */
  int algorithm;          /* DPGO_ALG_RTR / DPGO_ALG_RGD */
  int q_format;           /* DPGO_QFMT_EDGES (default: edge-stream Q) or DPGO_QFMT_BSR (explicit Q) */
  /* robust cost (RobustCostParameters, include/DPGO/DPGO_robust.h; PGOAgentParameters) */
  int robust_cost;             /* DPGO_ROBUST_* (default L2) */
  int robust_opt_inner_iters;  /* 30: reweight when (iteration + 1) % this == 0 */
  int gnc_max_iters;           /* 100 */
  double gnc_barc;             /* 10 */
  double gnc_mu_step;          /* 1.4 */
  double gnc_init_mu;          /* 1e-4 */
  double huber_threshold;      /* 3 */
  double tls_threshold;        /* 10 */
  /* PGOAgent status after every selected update (src/PGOAgent.cpp:700-716): relativeChange =
   * |X - XPrev| / sqrt(n) and readyToTerminate, on the device (dpgo_rbcd_status) */
  int status;                    /* 1 (the reference always computes it) */
  double rel_change_tol;         /* 5e-3 (PGOAgentParameters::relChangeTol) */
  double min_convergence_ratio;  /* 0.8 (robustOptMinConvergenceRatio, GNC_TLS only) */
} dpgo_rbcd_params;

/* RobustCostType (include/DPGO/DPGO_robust.h): weights need an edge-stream Q (q_format EDGES) */
#define DPGO_ROBUST_L2 0
#define DPGO_ROBUST_L1 1
#define DPGO_ROBUST_TLS 2
#define DPGO_ROBUST_HUBER 3
#define DPGO_ROBUST_GM 4
#define DPGO_ROBUST_GNC_TLS 5

void dpgo_rbcd_default_params(dpgo_rbcd_params* p);
/* Host-only (no GPU needed): the public-pose exchange plan of `rank` -- poses per peer it sends /
 * receives (counts in poses) and, if the arrays are non-NULL, the global pose ids, peer-major,
 * ascending within a peer.  dpgo_rbcd_pack / all_to_all / dpgo_rbcd_update follow this plan. */
int dpgo_rbcd_plan(dpgo_graph g, int num_agents, const int* agent_of_pose, const int* agent_rank, int rank,
                   int world, long long* send_counts, long long* recv_counts, int* send_poses, int* recv_poses);
/* agent_of_pose[n] in [0, num_agents); agent_rank[num_agents] in [0, world). */
int dpgo_rbcd_create(dpgo_graph g, int num_agents, const int* agent_of_pose, const int* agent_rank,
                     int rank, int world, const dpgo_rbcd_params* p, dpgo_rbcd* out);
int dpgo_rbcd_destroy(dpgo_rbcd e);
/* Launch every engine operation on a caller-owned hipStream_t from now on (NULL = the HIP null
 * stream); work queued on the previous stream is drained first.  The engine never destroys it. */
int dpgo_rbcd_set_stream(dpgo_rbcd e, void* stream);
/* Back to the engine's own (non-blocking) stream. */
int dpgo_rbcd_reset_stream(dpgo_rbcd e);
/* number of colour classes, agents owned by this rank, poses owned by this rank */
int dpgo_rbcd_info(dpgo_rbcd e, int* num_colors, int* owned_agents, int* owned_poses,
                   int* owned_agents_per_color /* [num_colors] or NULL */);
int dpgo_rbcd_color_of_agent(dpgo_rbcd e, int* color /* [num_agents] */);
/* doubles this rank sends to / receives from each peer per exchange (world entries each) */
int dpgo_rbcd_exchange_counts(dpgo_rbcd e, long long* send_counts, long long* recv_counts);
/* global r x (d+1) n column-major host X: copy the owned poses in; (re)initialise Nesterov state */
int dpgo_rbcd_set_X(dpgo_rbcd e, const double* X_global);
/* write the owned poses into a global host array (other poses untouched) */
int dpgo_rbcd_get_X(dpgo_rbcd e, double* X_global);
/* The read-in that matches dpgo_rbcd_get_trajectory: start from an SE(d) trajectory.  T_global: d x (d+1) n
 * column-major host array, every pose in the frame of its agent's entry of `frames` (num_agents x d x (d+1)
 * column-major, dpgo_graph_distributed_init_ex's outputs), or already in one common frame with frames = NULL (an
 * earlier dpgo_rbcd_get_trajectory, any other SE(d) guess).  Only the owned poses' d x (d+1) blocks cross to the
 * device; there X = YLift [F_R R_j | F_R t_j + F_t] per pose (dpgo_hip_frame_lift_dev on the engine's stream; YLift
 * r x d column-major), then the Nesterov state is (re)initialised exactly as by dpgo_rbcd_set_X.  Synchronises. */
int dpgo_rbcd_set_trajectory(dpgo_rbcd e, const double* T_global, const double* YLift_colmajor, const double* frames);
/* ---- solution readout: SE(d) trajectory and loop-closure weights ---------------------------
 * lifted pose of global pose `pose` (r x (d+1), column-major) if this rank owns it: *owned = 1 and
 * anchor written; else *owned = 0 and anchor untouched.  Synchronises.  (PGOAgent::setGlobalAnchor takes
 * this pose; with several ranks the caller broadcasts it from the rank that owns it.) */
int dpgo_rbcd_get_anchor(dpgo_rbcd e, int pose, double* anchor, int* owned);
/* getTrajectoryInGlobalFrame (src/PGOAgent.cpp:500-519) of every owned agent in the frame of `anchor` (NULL =
 * global pose 0, which this rank must own, else EINVAL): rounded on the device from the engine's X
 * (dpgo_hip_round_se_dev on the engine's stream, after whatever is queued there), written at the owned poses
 * of a global d x (d+1) n column-major host array (other poses untouched, as get_X).  Only the rounded
 * poses cross to the host.  Synchronises. */
int dpgo_rbcd_get_trajectory(dpgo_rbcd e, const double* anchor, double* T_global);
/* ---- the engine's trajectory against a ground truth (dpgo_hip_traj_*, include/dpgo_hip.h): the rounded
 * trajectory never leaves the device and nothing is gathered ------------------------------------------------
 * The truth of the owned poses (from a global d x (d+1) n column-major host array) and their mask (use_global: one
 * int per global pose, NULL = every pose) go to the device once, in the engine's pose order.  T_truth_global NULL
 * clears it.  Synchronises. */
int dpgo_rbcd_set_truth(dpgo_rbcd e, const double* T_truth_global, const int* use_global);
/* This rank's moments (DPGO_TRAJ_MOMENTS(d) doubles) of its owned poses, rounded into engine scratch in the frame
 * of `anchor` with the conventions and refusals of dpgo_rbcd_get_trajectory, against their truth about `shift`
 * (2 d doubles, NULL = zeros): one rounding and one dpgo_hip_traj_moments_dev on the engine's stream; only the
 * moments cross to the host.  With several ranks the caller sums the vectors (a valid moment vector within the
 * rounding bound, not bitwise the one-rank value, as for dpgo_rbcd_gram), takes the means from the zero-shift call
 * as the shift of a second one, and gives that sum to dpgo_hip_align_moments.  A rank without poses writes zeros.
 * DPGO_HIP_EINVAL before dpgo_rbcd_set_truth.  Synchronises. */
int dpgo_rbcd_truth_moments(dpgo_rbcd e, const double* anchor, const double* shift, double* mom);
/* dpgo_hip_traj_errors_dev of the same rounded poses under Aa ([A | a], NULL = identity): tra_sq and rot_sq land
 * at the owned poses of global arrays of n doubles (other entries untouched, as get_X; each may be NULL), bitwise
 * dpgo_hip_traj_errors of the merged dpgo_rbcd_get_trajectory.  sums (DPGO_TRAJ_SUMS doubles, may be NULL) is this
 * rank's partial: the caller adds entries 0-2 over the ranks and takes the maximum of 3-4.  A rank without poses
 * writes zero sums.  DPGO_HIP_EINVAL before dpgo_rbcd_set_truth or with no output.  Synchronises. */
int dpgo_rbcd_truth_errors(dpgo_rbcd e, const double* anchor, const double* Aa, double* tra_sq_global,
                           double* rot_sq_global, double* sums);
/* ---- rank reduction on the engine's X (dpgo_hip_gram / dpgo_hip_rank_reduce, include/dpgo_hip.h) ------
 * This rank's partial Gram C (r x r, column-major) = sum over its owned poses of Y_j Y_j^T: the owned buffer is
 * contiguous, so one dpgo_hip_gram_dev on the engine's stream, and 8 r^2 bytes cross to the host.  Synchronises.  With
 * several ranks the caller sums the partials (as it broadcasts the anchor): that sum is a valid Gram within the
 * rounding bound but not bitwise the one-rank value, whose partials cover other spans.  A rank without poses
 * writes zeros. */
int dpgo_rbcd_gram(dpgo_rbcd e, double* C);
/* The engine's X truncated to rank k along W (r x k, column-major, host: the leading eigenvectors of the summed
 * Gram, dpgo_hip_gram_eig), by dpgo_hip_rank_reduce_dev on the engine's stream, written at the owned poses of a
 * global k x (d+1) n column-major host array (other poses untouched, as get_X).  Only k (d+1) doubles per pose
 * cross to the host.  Synchronises.  The merged array starts an engine of rank k (dpgo_rbcd_set_X).
 * DPGO_HIP_EINVAL for k < d or k >= r. */
int dpgo_rbcd_get_X_reduced(dpgo_rbcd e, int k, const double* W, double* Xk_global);
/* current weight of every measurement this rank is responsible for, at its index in the graph's
 * edge order (w[m]; entries of other ranks' edges untouched).  Responsible = dpgo_rbcd_weight_owner's agent
 * lives on this rank; odometry (owner -1) is written by the rank of its agent: 1 until dpgo_rbcd_set_weights, then
 * the value that was set.  With robust_cost L2 and no weights set every written entry is exactly 1 (nothing is read
 * from the device). */
int dpgo_rbcd_get_weights(dpgo_rbcd e, double* w);
/* Weights and known inliers from outside (the reference's RelativeSEMeasurement::weight and ::isKnownInlier,
 * src/PGOAgent.cpp:742-744, 796-798, 1186, 1203, 1257, 1266).  w[m]: one weight per edge of the graph the engine
 * was created from, in its edge order -- the full array on every rank (as dpgo_rbcd_set_X's X_global); a rank uses
 * the entries of the copies it holds, nothing is communicated.  fixed[m] (may be NULL = no edge fixed): nonzero
 * marks a known inlier, which no reweighting rewrites and the converged ratio leaves out of count and total.  A call
 * replaces both the weights and the flags.  Odometry weights are set like any other and never reweighted; their flag
 * is ignored.  Both agents' copies of a shared edge take the weight and the flag; afterwards GNC rewrites the
 * responsible (lower-ID) copy only, the other keeps what was set.  On the engine's stream: the colour problems' Q,
 * block-Jacobi inverses and (lazily) exact factors follow, the converged ratios are recomputed (GNC_TLS), and with
 * acceleration PGOAgent::initializeAcceleration runs (XPrev = V = Y = X, gamma = alpha = 0) as after a reweighting.
 * mu, the GNC iteration count and the iteration number are untouched.
 * The host form validates first: a negative or non-finite weight, or an engine whose q_format is not
 * DPGO_QFMT_EDGES, is DPGO_HIP_EINVAL and leaves the engine unchanged; it synchronises.  The _dev form takes device
 * pointers (w 8-byte aligned) valid until the stream has passed the call; its caller guarantees finite weights
 * >= 0 (only q_format is checked). */
int dpgo_rbcd_set_weights(dpgo_rbcd e, const double* w, const unsigned char* fixed);
int dpgo_rbcd_set_weights_dev(dpgo_rbcd e, const double* w_dev, const unsigned char* fixed_dev);
/* Average ms (HIP events on the engine's stream) of `reps` launches of k_set_weights for colour class c, repeating
 * the launch of the last host-form dpgo_rbcd_set_weights (the same values, so the engine does not change).  After a
 * device-form call or any reweighting since that call the staged values are no longer the engine's:
 * DPGO_HIP_ESTATE, nothing launched. */
int dpgo_rbcd_bench_set_weights(dpgo_rbcd e, int color, int reps, double* ms);
/* The residuals behind those weights: err = kappa |Y1 R - Y2|_F^2 + tau |p2 - p1 - Y1 t|^2 (and its two parts) of
 * exactly the measurements dpgo_rbcd_get_weights reports for this rank, at the engine's current X after whatever is
 * queued on its stream, written at their index in the graph's edge order (err, rot_sq, tra_sq of m doubles, each
 * may be NULL, not all; other entries untouched).  One dpgo_hip_edge_errors launch over a per-rank table (graph
 * edge, pose sources, measurement) that the first call builds: it reads the measurements of the graph the engine
 * was created from, which must still exist then (not needed by later calls, nor by an engine that never asks).  A shared edge's other endpoint is read
 * from the same rank's X or from recv_dev: a dpgo_rbcd_pack and exchange done after the last update, unpacked as
 * dpgo_rbcd_central_eval unpacks it; required when this rank receives poses, else EINVAL.
 * rounded = 0: the lifted errors.  rounded = 1: the errors of the rounded trajectory -- the owned poses and the
 * received ones are rounded by dpgo_hip_round_se_dev in the frame of `anchor` (r x (d+1), host; NULL = global pose
 * 0, which this rank must then own, else EINVAL, as dpgo_rbcd_get_trajectory) and the kernel runs at r = d.  Rounding
 * is per pose given the anchor, so no second exchange of rounded poses takes place, and the merged result is
 * bitwise dpgo_graph_edge_errors of the merged dpgo_rbcd_get_trajectory.  Synchronises.  On EINVAL the outputs are
 * untouched. */
int dpgo_rbcd_get_errors(dpgo_rbcd e, const double* recv_dev, int rounded, const double* anchor,
                         double* err, double* rot_sq, double* tra_sq);
/* host-only: the agent whose weight dpgo_rbcd_get_weights reports per edge (owner[m]); -1 = odometry
 * (both poses in one agent at consecutive local indices), never reweighted, weight 1.  A private loop
 * closure: its agent.  A shared loop closure: the lower-ID agent of the two -- the only copy
 * PGOAgent::updateLoopClosuresWeights ever updates (src/PGOAgent.cpp:1201-1235); the other copy stays 1. */
int dpgo_rbcd_weight_owner(dpgo_graph g, int num_agents, const int* agent_of_pose, int* owner);
/* Phase 1 of iteration with selected colour c: every non-selected agent runs iterate(false).  Any colour order:
 * a robust cost's reweighting (src/PGOAgent.cpp:1174-1244) reads the agent's own X and, for shared loop closures,
 * its neighborPoseDict -- the neighbour poses it received when it was last selected (the engine snapshots them in
 * dpgo_rbcd_update*), so results do not depend on the rank count or on the halo kind. */
int dpgo_rbcd_pre_exchange(dpgo_rbcd e, int color);
/* Pack the public poses peers need into send_dev (their X: with Nesterov the aux pose a receiver
 * uses equals the sender's X, which ran iterate(false) this iteration). */
int dpgo_rbcd_pack(dpgo_rbcd e, double* send_dev);
/* Phase 2: selected agents of colour c update from the received neighbour poses. */
/* Restrict the next updates to a subset of the selected colour's agents (agent_mask [num_agents], 1 =
 * optimise; nullptr = every agent of the colour, the colour schedule).  The others of the colour run
 * PGOAgent::iterate(false) like every other colour's agents (X = Y with acceleration, X unchanged without) and
 * do not receive neighbour poses (their reweighting keeps reading their older dictionaries), so
 * selecting one agent per round (colour = its colour) is the example's greedy schedule
 * (examples/MultiRobotExample.cpp:243-256: the next robot is the argmax of the per-robot |RieGrad|, which
 * dpgo_rbcd_central_eval returns squared per agent). */
int dpgo_rbcd_set_selected(dpgo_rbcd e, const int* agent_mask);
int dpgo_rbcd_update(dpgo_rbcd e, int color, const double* recv_dev, dpgo_opt_result* results);
/* Per-colour halo (examples/MultiRobotExample.cpp:188-213: only the selected robot pulls its neighbours'
 * poses): the poses the agents of colour c read this iteration -- about half the full plan with two
 * colours.  Same call order as the full halo: dpgo_rbcd_pre_exchange(c), dpgo_rbcd_pack_color(c) into a
 * buffer laid out by dpgo_rbcd_exchange_counts_color(c) (peer-major, ascending global pose id), the
 * exchange, dpgo_rbcd_update_color(c).  Results are bitwise those of the full halo, in any colour order and with
 * any robust cost (nothing but the selected colour reads the halo).  dpgo_rbcd_central_eval always takes the full
 * plan. */
int dpgo_rbcd_plan_color(dpgo_graph g, int num_agents, const int* agent_of_pose, const int* agent_rank, int color,
                         int rank, int world, long long* send_counts, long long* recv_counts, int* send_poses,
                         int* recv_poses);
int dpgo_rbcd_exchange_counts_color(dpgo_rbcd e, int color, long long* send_counts, long long* recv_counts);
int dpgo_rbcd_pack_color(dpgo_rbcd e, int color, double* send_dev);
int dpgo_rbcd_update_color(dpgo_rbcd e, int color, const double* recv_dev, dpgo_opt_result* results);
/* Algorithmic HBM bytes of one X.Q SpMM over colour class c on this rank, and the timed average
 * of `reps` such launches (ms, HIP events on the engine stream). */
int dpgo_rbcd_bench_spmm(dpgo_rbcd e, int color, int reps, double* bytes, double* ms);
/* Bytes of one X.Q SpMM over colour class c on this rank: SURVEY 8(d)'s B_spmm for Q as explicit
 * blocks, and the bytes of the form the engine stores (edge stream by default). */
int dpgo_rbcd_spmm_bytes(dpgo_rbcd e, int color, double* bsr_bytes, double* format_bytes);
/* Average ms of one Riemannian HVP over colour class c at the current X (HIP events). */
int dpgo_rbcd_bench_hvp(dpgo_rbcd e, int color, int reps, double* ms);
/* SpMM / HVP launches issued so far (for throughput accounting) */
int dpgo_rbcd_counters(dpgo_rbcd e, long long* agent_updates, long long* iterations);
/* Tuning key 15 (next-Y fusion): selected-colour combination passes skipped because the previous iteration's
   non-selected pass had already written that colour's Y / XPrev, and write-ahead records that did not match the
   next call (another colour, a restart or reweighting, another alpha) and were dropped.  Either may be null. */
int dpgo_rbcd_next_y_counters(dpgo_rbcd e, long long* skipped, long long* mispredicted);
/* Tuning key 16 (blocked tCG queueing) on colour class c: dpgo_hip_tcg_blocks of the colour's batch -- the blocks its
   last update was queued in (0: unblocked) and the tile count of each of its agents on this rank, in batch order
   (agent_tiles[agents of the colour on this rank]).  Either may be null. */
int dpgo_rbcd_tcg_blocks(dpgo_rbcd e, int color, int* blocks_last, int* agent_tiles);

/* Central evaluation (examples/MultiRobotExample.cpp:229-235): this rank's share of the whole-graph
 * cost f(X) = 1/2 <X Q, X> (sum over ranks = the central cost; Q is the dataset's, unit weights, as the
 * example's QCentral -- with a robust cost the reweighted Q of the solve is not what is evaluated)
 * and, per owned agent, |RieGrad|^2 of its block (the greedy selection / stop test, :243-256).
 * Call between iterations; recv_dev: the public poses of a dpgo_rbcd_pack + exchange done after the
 * last update (required when world > 1).  gradnorm_sq[num_agents]: 0 for agents of other ranks.
 * Synchronises. */
int dpgo_rbcd_central_eval(dpgo_rbcd e, const double* recv_dev, double* f_out, double* gradnorm_sq);
/* weighted = 0: dpgo_rbcd_central_eval (unit weights, always -- also after dpgo_rbcd_set_weights).  weighted = 1: the
 * problem the engine is solving -- the colour problems' current Q (the weights last set or last left by the
 * reweighting) and G assembled with the entries' current weights: this rank's share of 1/2 <X Q_w, X> and the
 * per-agent |RieGrad|^2 of that problem.  A shared edge's two copies enter with their own weights (equal after a
 * set_weights, until GNC rewrites the responsible one). */
int dpgo_rbcd_central_eval_ex(dpgo_rbcd e, const double* recv_dev, int weighted, double* f_out,
                              double* gradnorm_sq);
/* PGOAgentStatus of every owned agent's last selected update (src/PGOAgent.cpp:700-716):
 * relativeChange and readyToTerminate, written at the agent's global index (others untouched).
 * PGOAgent::shouldTerminate (:1007-1031) = every agent ready, gathered over ranks by the caller. */
int dpgo_rbcd_status(dpgo_rbcd e, double* rel_change, int* ready);
/* Cumulative solver counters per owned agent (DPGO_STATS_INTS ints at the agent's global index,
 * layout of dpgo_hip_stats). */
int dpgo_rbcd_stats(dpgo_rbcd e, int* out);
/* Algorithmic HBM bytes of every kernel the engine launched so far (SURVEY 8(d) accounting over the
 * exact per-agent launch counts) and, per colour, the bytes of one tCG-start evaluation pass
 * (k_spmm MODE_EVAL_TCG) over the colour (evaltcg_bytes_per_color[num_colors], may be NULL). */
int dpgo_rbcd_bytes(dpgo_rbcd e, double* bytes, double* evaltcg_bytes_per_color);
/* ---- native halo exchange (examples/MultiRobotExample.cpp:188-213) -------------------
 * RCCL point-to-point over the ranks of the engine, without torch: dpgo_rccl_unique_id on one rank
 * (DPGO_RCCL_ID_BYTES opaque bytes, broadcast by the caller out of band), dpgo_rbcd_comm_init on every
 * rank (collective; the engine owns and destroys the communicator), or dpgo_rbcd_comm_attach of a
 * caller-owned ncclComm_t of the same RCCL instance (its size / rank must equal world / rank).  Per
 * iteration, after dpgo_rbcd_pre_exchange: dpgo_rbcd_exchange packs the public poses and posts one
 * ncclGroupStart / per-peer ncclSend + ncclRecv / ncclGroupEnd on the engine stream; *recv_dev is the
 * engine-owned receive buffer to pass to dpgo_rbcd_update.  RCCL is resolved at run time (the copy
 * already loaded in the process, else the system librccl.so.1); DPGO_HIP_EDEVICE if absent. */
#define DPGO_RCCL_ID_BYTES 128
int dpgo_rccl_unique_id(void* id_out);
int dpgo_rbcd_comm_init(dpgo_rbcd e, const void* id);
int dpgo_rbcd_comm_attach(dpgo_rbcd e, void* comm);
/* dpgo_hip_exact_factor_info of the colour's batched problem (zeros when this rank owns none of its agents) */
int dpgo_rbcd_exact_factor_info(dpgo_rbcd e, int color, long long* nodes, int* levels, int* max_s_tiles,
                                long long* panel_doubles, double* factor_ms, int* factor_count);
/* dpgo_hip_exact_factor_flops of the colour's batched problem (zeros when this rank owns none of its agents) */
int dpgo_rbcd_exact_factor_flops(dpgo_rbcd e, int color, double* cholesky_flops, double* inverse_flops);
/* dpgo_hip_exact_sweep_bytes of the colour's batched problem (zeros when this rank owns none of its agents) */
int dpgo_rbcd_exact_sweep_bytes(dpgo_rbcd e, int color, double* fwd_bytes, double* bwd_bytes);
/* dpgo_hip_bench_precond over colour class c's batched problem, right-hand side the colour's current X */
int dpgo_rbcd_bench_precond(dpgo_rbcd e, int color, int reps, double* ms_fwd, double* ms_bwd, double* panel_bytes);
/* The engine's RCCL communicator as RCCL sees it (ncclCommCount, ncclCommUserRank); -1, -1 without one. */
int dpgo_rbcd_comm_info(dpgo_rbcd e, int* count, int* rank);
int dpgo_rbcd_exchange(dpgo_rbcd e, const double** recv_dev);
/* the per-colour halo of colour c by the same RCCL group (then dpgo_rbcd_update_color) */
int dpgo_rbcd_exchange_color(dpgo_rbcd e, int color, const double** recv_dev);
/* SpMM modes of the per-mode arrays, in this order: XQ, XQ_G, EVAL, HESS, F, EVAL_TCG, CERT, QF, HESS_QF,
 * HESS_M, HESS_QF_M (the last two: the merged tCG iteration's Hessian passes) */
#define DPGO_SPMM_MODES 11
/* Algorithmic bytes of one X.Q launch over every agent of `color`, per SpMM mode (out[DPGO_SPMM_MODES], indexed as
 * dpgo_rbcd_kernel_times; 0 for modes the engine does not launch in a step).  A launch over part of the batch (the
 * merged tCG's half-batch launches on two streams, tuning key 10) moves its share of these bytes: divide by
 * dpgo_rbcd_kernel_times_ex's full-batch equivalents, not by the launch count. */
int dpgo_rbcd_mode_bytes(dpgo_rbcd e, int color, double* out);
/* HIP events around in-step X.Q launches (on the launch stream): `period` 0 = off, 1 = every launch, k = every
 * k-th launch of each mode (a sample: an event pair adds a dispatch gap of a few microseconds around its launch);
 * dpgo_rbcd_kernel_times synchronises and returns, per SpMM mode (DPGO_SPMM_MODES entries, order above), the
 * summed milliseconds and launch counts of the timed launches since the last call. */
int dpgo_rbcd_set_kernel_timing(dpgo_rbcd e, int period);
/* dpgo_hip_problem_set_tuning on every colour problem of the engine (A/B timing on one engine). */
int dpgo_rbcd_set_tuning(dpgo_rbcd e, int key, int value);
/* Per-iteration RTR / tCG trace of every owned agent's updates (dpgo_hip_set_trace / _get_trace
 * records, per agent at its global index). */
int dpgo_rbcd_set_trace(dpgo_rbcd e, int capacity);
int dpgo_rbcd_get_trace(dpgo_rbcd e, int agent, double* out, int max_records, int* count);
int dpgo_rbcd_kernel_times(dpgo_rbcd e, double* ms_per_mode, long long* launches_per_mode);
/* dpgo_rbcd_kernel_times plus, per mode, the timed launches' summed share of their batch's tiles (full-batch launch
 * equivalents: a launch over every agent counts 1, a half-batch launch about 0.5); any pointer may be null. */
int dpgo_rbcd_kernel_times_ex(dpgo_rbcd e, double* ms_per_mode, long long* launches_per_mode, double* batch_equiv);

#ifdef __cplusplus
}
#endif
#endif /* DPGO_RBCD_H */

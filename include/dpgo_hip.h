/*
 * dpgo_hip.h -- C ABI of the MI355X-native DPGO RBCD hot path (libdpgo_hip.so).
 *
 * This is the drop-in boundary that sits under the reference's C++ API
 * (QuadraticProblem / QuadraticOptimizer / LiftedSEManifold / PGOAgent::updateX).
 * Every entry point cites the reference interface it replaces (paths relative to the
 * lajoiepy/dpgo source root).  The C++ shim classes in dpgo_amd/cpp keep the reference
 * signatures and forward here; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *  - All arithmetic is fp64.  d in {2,3}, b = d+1, r = relaxation rank, 2 <= r <= 8, r >= d.
 *  - Pose matrices use the reference layout: X is r x (b n), column-major, so pose j is the
 *    contiguous r*b doubles [Y_j (r x d, col-major) | p_j (r)]   (tests/testEigenMap.cpp:19-35).
 *  - A problem handle holds one or more *agents* (independent RBCD blocks) whose poses are
 *    concatenated in agent order; single-agent handles reproduce QuadraticProblem exactly.
 *    Per-agent outputs (f, norms, results) are arrays of length num_agents.
 *  - Host-pointer entry points copy in/out and synchronise; *_dev entry points take device
 *    pointers, run asynchronously on the handle's stream and never synchronise unless stated.
 *  - Return value: 0 (DPGO_HIP_OK) or a negative error code; dpgo_hip_last_error() returns a
 *    thread-local message.  No C++ exception crosses this boundary.  There is no CPU fallback:
 *    without a usable gfx950 device every compute call returns DPGO_HIP_ENODEV.
 */
#ifndef DPGO_HIP_H
#define DPGO_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPGO_HIP_OK 0
#define DPGO_HIP_EINVAL (-1)
#define DPGO_HIP_ENODEV (-2)
#define DPGO_HIP_EDEVICE (-3)
#define DPGO_HIP_ENOMEM (-4)
#define DPGO_HIP_ESTATE (-5)

/* Preconditioner modes (QuadraticProblem::PreConditioner, src/QuadraticProblem.cpp:75-87).
 * EXACT: the reference's own -- P_X(V (Q + 0.1 I)^-1) with a supernodal multifrontal Cholesky factor of
 * Q + 0.1 I: nested-dissection tree built on the host once per Q pattern, numeric factorisation on the GPU for an
 * edge-stream Q (per tree level, dense frontal tiles on the fp64 matrix cores; again after every on-device
 * reweighting) or on the host for a BSR Q; each application is two sweeps of dense panel products
 * [L_SS^-1 ; L_RS L_SS^-1] per supernode, one launch per tree level and sweep.  If Q + 0.1 I is not positive
 * definite it falls back to the identity, as the reference does (:81-86).
 * BLOCK_JACOBI: per-pose (Q_jj + 0.1 I)^-1 (the north_star's throughput choice). NONE: identity. */
#define DPGO_PRECON_EXACT 0
#define DPGO_PRECON_BLOCK_JACOBI 1
#define DPGO_PRECON_NONE 2

/* Device form of Q: explicit block-sparse rows, or the measurement (edge) stream it is built from */
#define DPGO_QFMT_BSR 0
#define DPGO_QFMT_EDGES 1

/* ROPTALG (include/DPGO/DPGO_types.h:29-35) */
#define DPGO_ALG_RTR 0
#define DPGO_ALG_RGD 1

/* ROPTLIB tCGstatusSet */
#define DPGO_TCG_NEGCURVTURE 0
#define DPGO_TCG_EXCREGION 1
#define DPGO_TCG_LCON 2
#define DPGO_TCG_SCON 3
#define DPGO_TCG_MAXITER 4

typedef struct dpgo_hip_problem_s* dpgo_hip_problem;

/* QuadraticOptimizer setters (include/DPGO/QuadraticOptimizer.h:34-71, defaults
 * src/QuadraticOptimizer.cpp:20-30) plus the preconditioner mode. */
typedef struct {
  int algorithm;             /* DPGO_ALG_RTR / DPGO_ALG_RGD */
  double rgd_stepsize;       /* setGradientDescentStepsize (1e-3) */
  int tr_iterations;         /* setTrustRegionIterations (1) */
  double tr_tolerance;       /* setTrustRegionTolerance (1e-2) */
  double tr_initial_radius;  /* setTrustRegionInitialRadius (10) */
  int tr_max_inner;          /* setTrustRegionMaxInnerIterations (50) */
  int verbose;               /* setVerbose */
  int precon;                /* DPGO_PRECON_* (BLOCK_JACOBI) */
} dpgo_opt_params;

/* ROPTResult (include/DPGO/DPGO_types.h:40-59) + solver counters */
typedef struct {
  int success;
  double fInit, gradNormInit, fOpt, gradNormOpt, relativeChange, elapsedMs;
  int tCGStatus;      /* DPGO_TCG_* of the last tCG, -1 if no tCG ran */
  int runs;           /* RTR Run() calls (radius-shrink retries) */
  int outer_iters;    /* RTR outer iterations */
  int inner_iters;    /* tCG iterations of the last tCG */
  int gave_up;        /* "Too many RTR rejections" (returned the input) */
} dpgo_opt_result;

/* ---- library ---------------------------------------------------------------------------*/
const char* dpgo_hip_version(void);
const char* dpgo_hip_last_error(void);
/* Number of usable gfx950 devices (0 if none). */
int dpgo_hip_device_count(void);
void dpgo_hip_default_params(dpgo_opt_params* p);

/* ---- problem lifecycle (QuadraticProblem ctor/dtor, src/QuadraticProblem.cpp:16-29) ----*/
int dpgo_hip_problem_create(int n, int d, int r, dpgo_hip_problem* out);
/* num_agents independent blocks with poses_per_agent[a] poses each (batched RBCD). */
int dpgo_hip_problem_create_batch(int num_agents, const int* poses_per_agent, int d, int r,
                                  dpgo_hip_problem* out);
int dpgo_hip_problem_destroy(dpgo_hip_problem h);
/* Launch on a caller-owned hipStream_t (NULL = the handle's own stream). */
int dpgo_hip_problem_set_stream(dpgo_hip_problem h, void* stream);
int dpgo_hip_problem_info(dpgo_hip_problem h, int* num_agents, int* total_poses, int* d, int* r);
int dpgo_hip_set_precon(dpgo_hip_problem h, int mode);

/* ---- problem data ------------------------------------------------------------------------*/
/* QuadraticProblem::setQ (src/QuadraticProblem.cpp:31-42): Q of one agent in the reference's
 * Eigen RowMajor CSR (include/DPGO/DPGO_types.h:23), (b n_a) x (b n_a), int32 indices. */
int dpgo_hip_set_Q_csr(dpgo_hip_problem h, int agent, int nrows, const int* rowptr,
                       const int* colidx, const double* vals);
/* Same data as block-sparse rows: block (j, colidx[k]) stored column-major (b*b doubles).
 * nbrows == n_a; column indices are agent-local pose indices. */
int dpgo_hip_set_Q_bsr(dpgo_hip_problem h, int agent, int nbrows, const int* browptr,
                       const int* bcolidx, const double* blocks);
/* Q of one agent given by the measurements it is built from, never materialised:
 * Q = A Omega A^T (constructConnectionLaplacianSE, src/DPGO_utils.cpp:214-286) for private edges,
 * plus the diagonal terms of shared edges (PGOAgent::constructQMatrix, src/PGOAgent.cpp:720-781).
 * m edges with agent-local endpoints p1 -> p2; an endpoint of -1 marks a shared edge whose other
 * end lives in another agent (it then adds T Omega T^T to Q_p1p1, or Omega to Q_p2p2, only).
 * R: d*d row-major per edge, t: d per edge, kappa/tau: precisions, weight: NULL = 1 (GNC weight w
 * multiplies both precisions).  The X.Q kernels then stream one 14-double record per edge
 * (8 for d = 2) instead of two b x b off-diagonal blocks plus diagonal blocks.  Every agent of a
 * handle must use the same form (BSR via set_Q_csr/_bsr, or edges). */
int dpgo_hip_set_Q_edges(dpgo_hip_problem h, int agent, int m, const int* p1, const int* p2,
                         const double* R, const double* t, const double* kappa, const double* tau,
                         const double* weight);
/* Reweight an edge-stream Q on the device (PGOAgent::constructQMatrix after a GNC weight update,
 * src/PGOAgent.cpp:720-781, 1181-1244): w_dev[e] (device, one weight per edge, agents' set_Q_edges
 * lists concatenated in agent order) replaces each edge's weight; records, diagonal blocks and the
 * block-Jacobi inverses are rebuilt by kernels (bitwise the host build with those weights), the
 * exact factor is refreshed on its next use.  Asynchronous on the handle's stream; w_dev must stay
 * valid until the next EXACT-preconditioned call. */
int dpgo_hip_set_edge_weights_dev(dpgo_hip_problem h, const double* w_dev);
/* QuadraticProblem::setG (src/QuadraticProblem.cpp:44-48) in sparse form: count pose blocks
 * (r x b column-major) at agent-local poses pose_idx[]; all other columns of G are zero. */
int dpgo_hip_set_G(dpgo_hip_problem h, int agent, int count, const int* pose_idx,
                   const double* blocks);
/* Dense r x (b n_a) G for one agent (column-major). */
int dpgo_hip_set_G_dense(dpgo_hip_problem h, int agent, const double* G);

/* ---- evaluations (QuadraticProblem, src/QuadraticProblem.cpp:50-101) ---------------------*/
/* f(X) = 0.5 <XQ, X> + <X, G> per agent (:50-60) */
int dpgo_hip_f(dpgo_hip_problem h, const double* X, double* f_out);
/* EucGrad: X Q + G (:62-66) */
int dpgo_hip_egrad(dpgo_hip_problem h, const double* X, double* EG);
/* EucHessianEta: V Q (:68-73) */
int dpgo_hip_ehvp(dpgo_hip_problem h, const double* V, double* HV);
/* RieGrad / RieGradNorm (:89-101): P_X(XQ + G), per-agent Frobenius norms; f_out optional */
int dpgo_hip_riegrad(dpgo_hip_problem h, const double* X, double* RG, double* norms,
                     double* f_out);
/* Riemannian Hessian at X applied to tangent V (ROPTLIB HessianEta = EucHessianEta + EucHvToHv) */
int dpgo_hip_rhvp(dpgo_hip_problem h, const double* X, const double* V, double* HV);
/* PreConditioner (:75-87) with the handle's mode */
int dpgo_hip_precondition(dpgo_hip_problem h, const double* X, const double* V, double* out);

/* ---- manifold (LiftedSEManifold / ROPTLIB Stiefel Set3), stateless ----------------------*/
/* ProductManifold::Projection: V_Y - Y sym(Y^T V_Y), V_p */
int dpgo_hip_tangent_project(int r, int d, int n, const double* X, const double* V, double* out);
/* QF retraction of scale*V at X: [qf(Y + s V_Y) | p + s V_p] */
int dpgo_hip_retract_qf(int r, int d, int n, const double* X, const double* V, double scale,
                        double* out);
/* LiftedSEManifold::project (src/manifold/LiftedSEManifold.cpp:34-45) */
int dpgo_hip_project_polar(int r, int d, int n, const double* in, double* out);
/* T (d x (d+1) n, column-major) = SE(d) rounding of X (r x (d+1) n) in the frame of `anchor`
 * (r x (d+1), column-major; NULL = pose 0 of X, i.e. getTrajectoryInLocalFrame): per pose
 * R_j = projectToRotationGroup(Y_a^T Y_j), t_j = Y_a^T p_j - Y_a^T p_a
 * (PGOAgent::getTrajectoryInGlobalFrame, src/PGOAgent.cpp:500-519).  DPGO_HIP_EINVAL for an unsupported
 * (r, d), n <= 0, or null X or T. */
int dpgo_hip_round_se(int r, int d, int n, const double* X, const double* anchor, double* T);
/* the same on device pointers, queued on `stream` (hipStream_t or NULL), no synchronisation; T_dev must not
 * overlap X_dev */
int dpgo_hip_round_se_dev(int r, int d, long long n, const double* X_dev, const double* anchor_dev,
                          double* T_dev, void* stream);
/* The inverse of dpgo_hip_round_se: lift n SE(d) poses T (d x (d+1) n, column-major, [R_j | t_j] per pose) to rank r,
 * each composed with a frame first: X_out (r x (d+1) n) = YLift [F_R R_j | F_R t_j + F_t] per pose, F = entry
 * frame_of[j] of `frames` (nf x d x (d+1), column-major); YLift r x d column-major.  frames and frame_of both NULL:
 * X_out = YLift T (T's entries only pass through the YLift product).  One streaming kernel.  DPGO_HIP_EINVAL for an
 * unsupported (r, d), n <= 0, null T, YLift or X_out, exactly one of frames / frame_of null (or nf <= 0 with them),
 * or a frame_of entry outside [0, nf). */
int dpgo_hip_frame_lift(int r, int d, int n, const double* T, const double* YLift, const double* frames, int nf,
                        const int* frame_of, double* X_out);
/* the same on device pointers (YLift: host), queued on `stream` (hipStream_t or NULL), no synchronisation;
 * X_out_dev must not overlap the inputs; frame_of_dev's entries are not checked */
int dpgo_hip_frame_lift_dev(int r, int d, long long n, const double* T_dev, const double* YLift, const double* frames_dev,
                            int nf, const int* frame_of_dev, double* X_out_dev, void* stream);

/* ---- optimisation (QuadraticOptimizer::optimize, src/QuadraticOptimizer.cpp:34-149) -----*/
/* Runs every agent of the handle; results[num_agents].  agent_enabled (optional, device or
 * host per variant) skips agents (their X_out = X_in, result.success = 0). */
int dpgo_hip_optimize(dpgo_hip_problem h, const dpgo_opt_params* params, const double* X_in,
                      double* X_out, dpgo_opt_result* results);

/* ---- device-pointer variants (asynchronous on the handle's stream) -----------------------*/
int dpgo_hip_f_dev(dpgo_hip_problem h, const double* X, double* f_out_host);
int dpgo_hip_egrad_dev(dpgo_hip_problem h, const double* X, double* EG);
int dpgo_hip_ehvp_dev(dpgo_hip_problem h, const double* V, double* HV);
int dpgo_hip_riegrad_dev(dpgo_hip_problem h, const double* X, double* RG);
int dpgo_hip_rhvp_dev(dpgo_hip_problem h, const double* X, const double* V, double* HV);
int dpgo_hip_project_polar_dev(dpgo_hip_problem h, const double* in, double* out);
/* out = project(ca[a] * A + cb[a] * B) per agent a (Nesterov updateY / updateV,
 * src/PGOAgent.cpp:1075-1091); ca/cb host arrays[num_agents]. */
int dpgo_hip_polar_combine_dev(dpgo_hip_problem h, const double* A, const double* B,
                               const double* ca, const double* cb, double* out);
/* Synchronises once per RTR Run (radius-shrink bookkeeping); results host array (may be NULL). */
int dpgo_hip_optimize_dev(dpgo_hip_problem h, const dpgo_opt_params* params, const double* X_in,
                          double* X_out, const int* agent_enabled_host, dpgo_opt_result* results);
/* Device buffer of the last tCG / RTR scalar state (for profiling / tests) */
int dpgo_hip_synchronize(dpgo_hip_problem h);

/* ---- solver statistics and per-iteration trace --------------------------------------------
 * Cumulative per-agent counters since the handle was created, DPGO_STATS_INTS ints per agent:
 * [optimize calls, calls that returned at once (|grad| < tol), RTR Runs, tCG inner iterations,
 *  tCG exits NEGCURVTURE, EXCREGION, LCON, SCON, MAXITER, updates that gave up, tCG CG steps,
 *  Runs whose tCG ended at its first step on the trust-region boundary, Runs whose first step test
 *  was the full pass that also stores Hess[delta] (chosen when the previous call took CG steps)]. */
#define DPGO_STATS_INTS 13
int dpgo_hip_stats(dpgo_hip_problem h, int* out /* [num_agents * DPGO_STATS_INTS] */);
/* Per-iteration RTR / tCG trace (the reference prints it with ROPTLIB Debug = ITERRESULT when
 * verbose, src/QuadraticOptimizer.cpp:82-86): after this call every tCG step test, tCG stopping
 * test and rho test appends one record of DPGO_TRACE_WIDTH doubles per agent, up to `capacity`
 * records per agent (0 turns tracing off).  Record fields (kernels.h TraceField): op (3 step test,
 * 4 stopping test, 5 rho test), j, f1, f2, rho, Delta, alpha, beta, tau, <delta, H delta>, |r|,
 * <z, r>, tCG status (-1 if none), accepted, |grad(x1)|, Run index. */
#define DPGO_TRACE_WIDTH 16
int dpgo_hip_set_trace(dpgo_hip_problem h, int capacity);
/* Copies agent's records (at most max_records) into out; *count = records written since
 * set_trace (may exceed capacity: the later ones were dropped). */
int dpgo_hip_get_trace(dpgo_hip_problem h, int agent, double* out, int max_records, int* count);

/* Source hash the library was compiled from (sha256 of the sources, hex; "unknown" if built
 * without it): lets a caller check that a shipped binary matches the tree it runs with. */
const char* dpgo_hip_build_id(void);

/* The tile that block `block` of a pose-tiled launch of `num_blocks` blocks works on (the kernels' own map, tuning
 * key 13): blocks b and b + 8 share an XCD, XCD slot b & 7 owns one contiguous range of tiles and walks it from its
 * start, or from its end when reverse != 0.  A bijection on [0, num_blocks); -1 for a block outside it.  No device
 * is needed. */
int dpgo_hip_tile_of_block(int block, int num_blocks, int reverse);
/* The same for every block of the launch: tiles[b], b < num_blocks. */
int dpgo_hip_tile_map(int num_blocks, int reverse, int* tiles);

/* ---- certification (not in the reference: parity is pinned against a sparse
 * eigensolver on the explicitly formed matrix) --------------------------------------------------
 * Smallest eigenvalue of the certificate matrix S(X) = Q - Lambda(X), Lambda = blockdiag of
 * [sym(Y_j^T (XQ + G)_Y) 0; 0 0]: X is a global minimiser of the rank-r relaxation iff S(X) >= 0.
 * Lanczos with full re-orthogonalisation on the device (the operator V -> V S(X) on r x (d+1) n
 * matrices has S's spectrum), stopping when the Ritz residual <= tol * |lambda|_max-estimate or
 * after max_iters steps.  Single-agent handles.  eigvec (host, r x (d+1) n, optional): the Ritz
 * vector of lambda_min. */
int dpgo_hip_certify(dpgo_hip_problem h, const double* X, int max_iters, double tol, double* lambda_min,
                     double* residual, int* iters, double* eigvec);
/* The same with a thick restart and a seed block.  basis_max > 0: at most basis_max Krylov vectors; a full
 * basis restarts from its lowest max(basis_max / 4, 8) Ritz vectors and the newest Krylov direction
 * (Rayleigh-Ritz on the dense projected matrix); max_iters counts operator applications over all
 * restarts.  flags DPGO_CERT_SEED_X: the principal directions of X's rows (S(X) X^T ~ 0 at a critical
 * point: the near-null space; singular values >= 1e-3 of the largest) and the translation gauge (every
 * translation column = 1, an exact null vector), orthonormalised, form a locked block U; the chain runs on its complement and U's block is
 * resolved exactly, S = [A_s B^T; B C] in (U, U_perp).  Everything lives on row 0 of the lifted layout
 * (the operator acts row by row).  lambda_min = the lowest Ritz value found (an upper bound of
 * lambda_min(S)); info (optional) carries the true residual of the returned pair and the bound
 * lower_bound = (a + c) / 2 - sqrt(((c - a) / 2)^2 + |B|_F^2), a = lambda_min(A_s), c = theta_C -
 * residual_C (the smallest eigenvalue of [a -|B|; -|B| c], which bounds x^T S x from below), rigorous when
 * theta_C is C's lowest eigenvalue to within its residual (Lanczos from a random start: with
 * probability ~1). */
#define DPGO_CERT_SEED_X 1
typedef struct {
  int iters;                  /* operator applications (all restarts) */
  int restarts;
  int seeds;                  /* independent rows of X in the locked block */
  double residual;            /* |S y - lambda_min y| of the returned Ritz pair */
  double lambda_seed;         /* lambda_min(U^T S U) (NaN without seeds) */
  double lambda_complement;   /* the chain's lowest Ritz value theta_C */
  double residual_complement; /* |P S y - theta_C y|, P = I - U U^T: its residual on C */
  double coupling;            /* |(I - U U^T) S U|_F (0 without seeds) */
  double lower_bound;         /* see above (theta_C - residual_C without seeds) */
  double ritz[8];             /* the chain's lowest Ritz values (NaN-padded) */
} dpgo_cert_info;
int dpgo_hip_certify_ex(dpgo_hip_problem h, const double* X, int max_iters, int basis_max, int flags, double tol,
                        double* lambda_min, double* eigvec, dpgo_cert_info* info);

/* ---- certification by factorisation (SE-Sync's fast verification; build-defined: pinned against dense Cholesky
 * and eigenvalues of the explicitly formed matrix) ---------------------------------------------------
 * S(X) = Q - Lambda(X) has Q's block pattern, so S(X) + sigma I goes through the exact preconditioner's
 * supernodal Cholesky with other diagonal blocks and another shift.  *pd = 1 iff no pivot of the factorisation of
 * S(X) + sigma I failed d > 0, which means lambda_min(S(X)) > -sigma up to the factorisation's backward error.
 * The numeric factorisation always runs on the device, on a factor state of its own: a handle that also uses
 * DPGO_PRECON_EXACT keeps its preconditioner's factor and counters as they were.  Single-agent handles with an
 * edge-stream Q (DPGO_HIP_EINVAL otherwise, and for a non-finite sigma); the exact preconditioner's size refusals
 * (the 24 GiB panel cap, host memory) surface unchanged. */
int dpgo_hip_certify_chol(dpgo_hip_problem h, const double* X, double sigma, int* pd);
typedef struct {
  double ratio;            /* the bracket is bisected on log sigma until sigma_hi / sigma_lo <= ratio (1 + 1/16) */
  int max_factorisations;  /* ... or this many factorisations were run (24) */
  double tol;              /* inverse iteration stops at |v S - lambda v| <= tol * sigma_top (1e-8) */
  int max_iters;           /* ... or after this many solves (200) */
} dpgo_chol_cert_params;
void dpgo_default_chol_cert_params(dpgo_chol_cert_params* p);
typedef struct {
  int certified;           /* 1: S(X) + eta I is positive definite, lambda_min > -eta; nothing else was computed */
  int factorisations;      /* numeric factorisations of this call */
  double sigma_lo;         /* S + sigma_lo I not positive definite, S + sigma_hi I positive definite:          */
  double sigma_hi;         /* -sigma_hi < lambda_min <= -sigma_lo (certified: sigma_lo = sigma_hi = eta)       */
  int invit_iters;         /* inverse iterations (solves with the factor at sigma_hi) */
  double residual;         /* |v S - lambda v| of the returned pair */
  double factor_ms;        /* device time of the last factorisation */
  long long panel_doubles; /* doubles of the factor's stored panels */
} dpgo_chol_cert_info;
/* lambda_min(S(X)) by a bracket and shifted inverse iteration.  First the test at sigma = eta (> 0); positive
 * definite: certified, *lambda_min = -eta (a strict lower bound), eigvec untouched.  Otherwise sigma_top =
 * (1 + 1e-6) max_j |Lambda_j|_F + eta is confirmed positive definite (Q >= 0; DPGO_HIP_EDEVICE if it is not), the
 * bracket [eta, sigma_top] is bisected on log sigma, every trial one numeric refactorisation, and inverse iteration
 * v <- normalise(v (S + sigma_hi I)^-1) from a seeded start on row 0 of the lifted layout converges at the rate
 * (lambda_min + sigma_hi) / (lambda_2 + sigma_hi).  *lambda_min: the Rayleigh quotient <v S, v> (an upper bound
 * of lambda_min, as the Lanczos value); eigvec (host, r x (d+1) n, optional): the unit vector on row 0, rows 1..
 * zero, as dpgo_hip_escape_direction takes it.  p NULL: the defaults.  Outputs are written only on success. */
int dpgo_hip_certify_chol_ex(dpgo_hip_problem h, const double* X, double eta, const dpgo_chol_cert_params* p,
                             double* lambda_min, double* eigvec, dpgo_chol_cert_info* info);

/* ---- block certificate (LOBPCG on the r rows of the lifted layout; build-defined: pinned against the eigenvalues
 * of the explicitly formed matrix and a numpy restatement, tests/_lobpcg.py) --------------------------
 * The operator V -> V S(X) acts on every row of the lifted r x (d+1) n layout in one launch, so the r rows serve as
 * r start vectors per operator pass: locally optimal block preconditioned CG on the iterate X_b, the residual block
 * W and the direction block P (six r-row blocks in all: the memory does not grow with the iteration count), one
 * Rayleigh-Ritz of at most 3r x 3r per iteration on the host and one wait per iteration.  Any Q format, any
 * weights (the handle's Q as it stands), no size refusal.  flags DPGO_CERT_SEED_X locks the block U of
 * dpgo_hip_certify_ex (X's principal row directions and the translation gauge) and the iteration runs on its
 * complement; info has dpgo_hip_certify_ex's meaning, with iters = operator passes (the start, one per iteration,
 * one per refresh, the final residual's and those of U's block), restarts = iterations that ran without P because
 * [X_b; W; P] had lost its conditioning, ritz = the block's r lowest values.  It stops when the lowest row's
 * residual (off U) <= tol * the largest |Ritz value| seen, or after max_iters iterations.  precon = 1: W = R Minv per
 * pose with the handle's block-Jacobi inverse of Q + 0.1 I (fewer iterations at a critical point, more at a
 * random one).  eigvec (host, r x (d+1) n, optional): the unit vector on row 0, rows 1.. zero, as
 * dpgo_hip_escape_direction takes it.  p NULL: the defaults.  DPGO_HIP_EINVAL, outputs untouched: a batched handle,
 * 3 r > (d+1) n - seeds, max_iters < 1, a non-finite tol, an unknown precon or flag, refresh < 0. */
typedef struct {
  int max_iters; /* iterations at most (2000) */
  double tol;    /* relative residual of the lowest pair (1e-8) */
  int flags;     /* DPGO_CERT_SEED_X (the default) or 0 */
  int precon;    /* 0 none (the default), 1 the handle's block-Jacobi inverse */
  int refresh;   /* every this many iterations X_b is re-projected, re-orthonormalised and S X_b recomputed (50; 0 never) */
} dpgo_block_cert_params;
void dpgo_default_block_cert_params(dpgo_block_cert_params* p);
int dpgo_hip_certify_block(dpgo_hip_problem h, const double* X, const dpgo_block_cert_params* p, double* lambda_min,
                           double* eigvec, dpgo_cert_info* info);

/* ---- rank staircase (SE-Sync / DC2-PGO's Riemannian staircase; not in the reference: pinned against the
 * oracle's retract_qf and a numpy restatement) ------------------------------------------------------
 * When the certificate fails at a critical point X of rank r (lambda_min(S(X)) < 0 with eigenvector v, a
 * (d+1) n vector), [X; 0] is a saddle of the rank r + 1 problem and [0; v^T] a direction of negative curvature
 * there: f(Retr_[X; 0](alpha [0; v^T])) = f(X) + 1/2 alpha^2 lambda_min + O(alpha^3) for unit v.
 * dpgo_hip_lift_escape: X_out ((r+1) x (d+1) n) = Retr_[X; 0](alpha [0; v^T]) with the QF retraction of
 * dpgo_hip_retract_qf, per pose [qf([Y_j; alpha v_Y^T]) | (p_j; alpha v_p)]; v NULL = the plain lift [X; 0]
 * (bitwise X's entries and zeros).  One streaming kernel.  DPGO_HIP_EINVAL for an unsupported (r, d), r = 8
 * (rank 9 is not compiled), n <= 0, or null X or X_out. */
int dpgo_hip_lift_escape(int r, int d, int n, const double* X, const double* v, double alpha, double* X_out);
/* the same on device pointers, queued on `stream` (hipStream_t or NULL), no synchronisation; X_out_dev must not
 * overlap X_dev */
int dpgo_hip_lift_escape_dev(int r, int d, long long n, const double* X_dev, const double* v_dev, double alpha,
                             double* X_out_dev, void* stream);
/* The escape direction from the certificate's Ritz matrix eigvec (r x (d+1) n, column-major, as dpgo_hip_certify*
 * returns it: the operator acts row by row, so every non-zero row is an eigenvector of S): the row of largest
 * 2-norm, normalised, into v ((d+1) n).  r = 1 takes a plain vector.  Host only, no device needed.
 * DPGO_HIP_EINVAL if every row is zero. */
int dpgo_hip_escape_direction(int r, int d, int n, const double* eigvec, double* v);
typedef struct {
  double alpha0;        /* first step length tried (1) */
  double decrease;      /* accept when f(X+) <= f_before + decrease alpha^2 lambda_min (0.25: half the prediction) */
  double min_gradnorm;  /* the escape is accepted only if |RieGrad(X+)| >= this (0): set it to the tolerance below
                           which the solver that takes X+ returns its input unchanged */
  int max_halvings;     /* alpha = alpha0 2^-k, k <= max_halvings (30) */
} dpgo_escape_params;
typedef struct {
  int accepted;          /* 1: X_out = X+(alpha); 0: X_out = the plain lift [X; 0] */
  int trials;            /* step lengths evaluated */
  double alpha;          /* the last step length tried */
  double f_before;       /* f([X; 0]) on h_next */
  double f_after;        /* f(X+(alpha)) */
  double gradnorm_after; /* |RieGrad(X+(alpha))| (0 when no step length passed the decrease test) */
} dpgo_escape_info;
void dpgo_hip_default_escape_params(dpgo_escape_params* p);
/* The escape with its line search.  h_next: a single-agent handle at rank r + 1 with Q set (r = its rank - 1);
 * X (r x (d+1) n) and the unit direction v ((d+1) n) are uploaded once, then per trial one dpgo_hip_lift_escape_dev
 * and one f through the handle's X.Q path run on the device and only f comes back.  The first alpha = alpha0 2^-k,
 * k <= max_halvings, with f(X+) <= f_before + decrease alpha^2 lambda_min is taken, |RieGrad(X+)| is evaluated
 * once, and the escape is accepted iff it is >= min_gradnorm (the gradient shrinks with alpha: a smaller alpha
 * cannot help).  Not accepted, or no alpha passed: X_out = [X; 0], info filled, DPGO_HIP_OK.  params NULL = the
 * defaults.  DPGO_HIP_EINVAL for lambda_min >= 0, a batched handle, or a handle of rank <= d. */
int dpgo_hip_escape(dpgo_hip_problem h_next, const double* X, const double* v, double lambda_min,
                    const dpgo_escape_params* params, double* X_out, dpgo_escape_info* info);

/* ---- rank reduction (SE-Sync's last step: truncate a solution to its numerical rank; not in the reference:
 * pinned against a numpy / long double restatement) ----------------------------------------------------
 * The way down the staircase.  With X r x (d+1) n, pose j = [Y_j | p_j]:
 * dpgo_hip_gram: C (r x r, column-major, full symmetric) = sum_j Y_j Y_j^T over the rotation columns only (tr C =
 * d n on the manifold; at a critical point of a connected graph the translations lie in span(Y) up to the
 * translation gauge, so no centring is needed).  One streaming kernel that leaves one partial per 128 poses and one
 * finishing kernel that sums them in a fixed order, no atomics: C is a function of (X, n) alone, bitwise
 * repeatable, and bitwise the same for any alignment of X.  DPGO_HIP_EINVAL for an unsupported (r, d), n <= 0, or
 * null X or C. */
int dpgo_hip_gram(int r, int d, int n, const double* X, double* C);
/* doubles of the work buffer dpgo_hip_gram_dev needs for (r, d, n): the block partials (0 for bad arguments) */
long long dpgo_hip_gram_work_doubles(int r, int d, long long n);
/* the same on device pointers, queued on `stream` (hipStream_t or NULL), no synchronisation; C_dev (r r doubles)
 * and work_dev (dpgo_hip_gram_work_doubles) must not overlap X_dev or each other */
int dpgo_hip_gram_dev(int r, int d, long long n, const double* X_dev, double* C_dev, double* work_dev, void* stream);
/* Eigenpairs of the symmetric r x r matrix C (column-major, r <= 8; its symmetric part is taken) by cyclic Jacobi:
 * w[r] descending, U (r x r, column-major) the eigenvectors in that order, each column signed so that its
 * largest-magnitude entry (the first of equals) is positive.  The numerical rank at tolerance tol is
 * k = max(d, #{i : w_i > tol w_1}); truncating to it drops sum_j |(I - W W^T) Y_j|_F^2 = sum_{i > k} w_i,
 * W = U[:, :k].  Host only, no device needed.  DPGO_HIP_EINVAL for r outside [1, 8], a null pointer or a
 * non-finite entry. */
int dpgo_hip_gram_eig(int r, const double* C, double* w, double* U);
/* X_out (k x (d+1) n) = the truncation of X to rank k along W (r x k, column-major, host memory: the leading k
 * columns of dpgo_hip_gram_eig's U), per pose [polar(W^T Y_j) | W^T p_j] with the polar factor of
 * dpgo_hip_project_polar.  If X has exact rank k, W^T Y_j is already on St(d, k), X_out^T X_out = X^T X and f is
 * unchanged; at k = d the result lies in O(d) per pose (dpgo_hip_round_se at r = d then handles the determinant;
 * this pass does not).  A pose whose W^T Y_j is exactly rank-deficient gets a finite, non-orthonormal block (the
 * Jacobi path leaves a zero singular direction zero).  One streaming kernel.  DPGO_HIP_EINVAL for an unsupported
 * (r, d) or (k, d), k < d or k >= r, n <= 0, null X, W or X_out, or X_out overlapping X. */
int dpgo_hip_rank_reduce(int r, int d, int n, const double* X, int k, const double* W, double* X_out);
/* the same on device pointers (W: host), queued on `stream` (hipStream_t or NULL), no synchronisation */
int dpgo_hip_rank_reduce_dev(int r, int d, long long n, const double* X_dev, int k, const double* W,
                             double* X_out_dev, void* stream);

/* ---- edge errors (the batch form of computeMeasurementError, src/DPGO_utils.cpp:509-515; the reference has the
 * per-edge function only: pinned against a long double restatement) -------------------------------------
 * For measurement e = (p1, p2, R, t, kappa, tau) and poses [Y_j | p_j] of r x (d+1) doubles (X column-major, a
 * lifted X or, at r = d, an SE(d) trajectory):
 *   rot_sq[e] = |Y_p1 R - Y_p2|_F^2,  tra_sq[e] = |p_p2 - p_p1 - Y_p1 t|^2,
 *   err[e] = kappa rot_sq[e] + tau tra_sq[e],  *cost = 1/2 sum_e w_e err[e]   (w NULL = ones).
 * With the weights Q was built from, cost = f(X) = 1/2 <Q, X^T X>.  One edge-parallel kernel; err[e] depends on
 * the measurement and its two poses alone, through one operation order per (r, d): equal inputs give bitwise
 * equal errors wherever the edge stands in the list.  The cost is one partial per 256 edges and one finishing
 * launch that sums the partials in a fixed order (no atomics): a function of (edge list in its order, X, w),
 * bitwise repeatable.  Any of err, rot_sq, tra_sq, cost may be NULL, not all four.  DPGO_HIP_EINVAL for an
 * unsupported (r, d), m <= 0, n <= 0, a null required pointer, p1 == p2 or an index outside [0, n); the outputs are
 * then untouched. */
typedef struct {                 /* R row-major d*d per edge, t d per edge, as dpgo_graph_copy_out */
  long long m;
  const int *p1, *p2;
  const double *R, *t, *kappa, *tau, *w;   /* w NULL = ones */
} dpgo_edges;
int dpgo_hip_edge_errors(int r, int d, int n, const dpgo_edges* E, const double* X,
                         double* err, double* rot_sq, double* tra_sq, double* cost);
/* doubles of the work buffer dpgo_hip_edge_errors_dev needs for the cost of m edges (0 for m <= 0) */
long long dpgo_hip_edge_errors_work_doubles(long long m);
/* the same on device pointers, queued on `stream` (hipStream_t or NULL), no synchronisation.  E_dev's arrays are
 * device pointers, the struct itself is host memory; the indices are trusted.  work_dev
 * (dpgo_hip_edge_errors_work_doubles) is needed only with cost_dev. */
int dpgo_hip_edge_errors_dev(int r, int d, long long n, const dpgo_edges* E_dev, const double* X_dev,
                             double* err_dev, double* rot_sq_dev, double* tra_sq_dev,
                             double* cost_dev, double* work_dev, void* stream);

/* ---- trajectory evaluation against a ground truth: alignment, ATE, RPE (build-defined; the reference has none:
 * pinned against a long double restatement) -----------------------------------------------------------------
 * A trajectory is d x (d+1) n doubles column-major, the layout dpgo_hip_round_se writes: pose j is d (d+1)
 * contiguous doubles [R_j (d x d column-major) | t_j].  That is the estimate, T the truth, d in {2, 3}.  `use` has
 * one int per pose: NULL = every pose, otherwise pose j counts iff use[j] != 0.
 *
 * Moments.  With a shift (s^, s) (2 d doubles, host memory, NULL = zeros), a_j = fl(t^_j - s^), b_j = fl(t_j - s):
 *   mom = [count, sum |a|^2, sum |b|^2, sum a (d), sum b (d), M = sum b a^T (d x d column-major)]
 * over the used poses, DPGO_TRAJ_MOMENTS(d) doubles.  Every entry is additive over disjoint pose sets: ranks merge
 * by summation.  One streaming kernel that leaves one partial per 128 poses and one finishing launch that sums them
 * in a fixed order, no atomics: mom is a function of the inputs alone, bitwise repeatable, and bitwise the same for
 * any 8-byte alignment of the pointers.
 *
 * Alignment from moments (host, no device needed).  n = count, mu^ = s^ + sum a / n, mu = s + sum b / n,
 * C = M - (sum b)(sum a)^T / n = U Sigma V^T (one-sided Jacobi), A = U diag(1, .., 1, det(U V^T)) V^T,
 * a = mu - A mu^: Horn / Umeyama without scale on the translations, the minimiser of sum |A t^_j + a - t_j|^2 over
 * SE(d).  Aa = [A | a], d x (d+1) column-major.  info: count, sigma descending with the d-th signed by that
 * determinant, rank = #{sigma_i > rank_tol sigma_1} (rank_tol <= 0 = the default 1e-12).  A is unique iff
 * rank >= d - 1; it is returned either way (C = 0, one pose: A = I).  count = 0 is DPGO_HIP_EINVAL.
 * dpgo_hip_traj_align takes the moments twice -- with a zero shift for the means, then about those means, where C's
 * correction term is at rounding level however far the trajectory lies from the origin -- and aligns: one upload,
 * two launches, one host step.  At several ranks the caller sums the moment vectors between the two.
 *
 * Errors.  Given Aa (host memory, NULL = identity), per pose
 *   tra_sq[j] = |A t^_j + a - t_j|^2,   rot_sq[j] = |A R^_j - R_j|_F^2   (chordal; the angle is
 *   2 asin(min(1, sqrt(rot_sq / 8)))),
 * a quiet NaN for an unused pose; sums (DPGO_TRAJ_SUMS doubles) = [count, sum tra_sq, sum rot_sq, max tra_sq,
 * max rot_sq] over the used poses: ATE RMSE = sqrt(sums[1] / sums[0]).  A pose's outputs depend on its own data and
 * Aa alone, through one operation order per d; the sums go through block partials in a fixed order and the maxima
 * are exact.  Any of tra_sq, rot_sq, sums may be NULL, not all three.  Ranks merge sums by adding entries 0-2 and
 * taking the maximum of 3-4.
 *
 * Relative poses of a trajectory over an edge list (p1, p2), as dpgo_edges takes measurements:
 *   R_out[e] (d d row-major) = R_p1^T R_p2,   t_out[e] = R_p1^T (t_p2 - t_p1).
 * RPE is dpgo_hip_edge_errors at r = d on the estimate with the truth's relative poses as the measurements and
 * kappa = tau = 1: its rot_sq and tra_sq per edge are gauge-free, no alignment enters.
 *
 * DPGO_HIP_EINVAL for d outside {2, 3}, n <= 0 (m <= 0), a null required pointer, an output overlapping an input
 * or another output and, on the host-pointer entries, p1 == p2 or an index outside [0, n); the outputs are then
 * untouched.  The _dev entries take device pointers (shift and Aa stay host memory), queue on `stream`
 * (hipStream_t or NULL) without synchronisation, trust the indices, and take their block partials from the caller
 * (work_dev, the *_work_doubles query; it must not overlap anything else). */
#define DPGO_TRAJ_MOMENTS(d) (3 + 2 * (d) + (d) * (d))
#define DPGO_TRAJ_SUMS 5
typedef struct {
  double count;     /* used poses */
  double sigma[3];  /* singular values of C, descending; the d-th carries the sign of det(U V^T) */
  int rank;         /* #{i : sigma_i > rank_tol sigma_1} (0 for C = 0) */
} dpgo_align_info;
int dpgo_hip_traj_moments(int d, int n, const double* That, const double* T, const int* use, const double* shift,
                          double* mom);
long long dpgo_hip_traj_moments_work_doubles(int d, long long n);
int dpgo_hip_traj_moments_dev(int d, long long n, const double* That_dev, const double* T_dev, const int* use_dev,
                              const double* shift, double* mom_dev, double* work_dev, void* stream);
int dpgo_hip_align_moments(int d, const double* shift, const double* mom, double rank_tol, double* Aa,
                           dpgo_align_info* info);
int dpgo_hip_traj_align(int d, int n, const double* That, const double* T, const int* use, double* Aa,
                        dpgo_align_info* info);
int dpgo_hip_traj_errors(int d, int n, const double* That, const double* T, const int* use, const double* Aa,
                         double* tra_sq, double* rot_sq, double* sums);
long long dpgo_hip_traj_errors_work_doubles(int d, long long n);
int dpgo_hip_traj_errors_dev(int d, long long n, const double* That_dev, const double* T_dev, const int* use_dev,
                             const double* Aa, double* tra_sq_dev, double* rot_sq_dev, double* sums_dev,
                             double* work_dev, void* stream);
int dpgo_hip_relative_poses(int d, int n, const double* T, int m, const int* p1, const int* p2, double* R_out,
                            double* t_out);
int dpgo_hip_relative_poses_dev(int d, long long n, const double* T_dev, long long m, const int* p1_dev,
                                const int* p2_dev, double* R_out_dev, double* t_out_dev, void* stream);

/* ---- pairwise consistency of frame candidates (build-defined) ----------------------
 * A candidate k is a rigid frame F_k = [R_k | t_k] (d x (d+1) column-major, d (d+1) doubles) plus a lever point
 * x_k (d doubles); a group is a contiguous run of candidates that should all describe one frame (group g holds
 * candidates group_off[g] .. group_off[g+1]; sizes 0 and 1 are allowed; group_off[0] = 0, ascending,
 * group_off[ngroups] = m).  For two candidates of one group, with dR = R_k - R_l and dt = t_k - t_l formed first:
 *   e_rot(k,l) = |dR|_F^2,   e_tra(k,l) = 1/2 (|dR x_k + dt|^2 + |dR x_l + dt|^2),
 *   A(k,l) = 1 iff k != l and e_rot <= c_R^2 and e_tra <= c_t^2   (any NaN gives 0; the diagonal is 0).
 * (l,k) is the exact negation of (k,l), so A and both e are bitwise symmetric.  One operation order per d, shared
 * by the kernel and the host twin, multiplications and additions never contracted: per entry of dR in storage
 * order, df = R_k - R_l, e_rot = e_rot + df df; per lever x and row i, v = dR[i,0] x[0], v = v + dR[i,c] x[c]
 * (c = 1 .. d-1), v = v + dt[i], s = s + v v; e_tra = 0.5 (s_k + s_l); c_R^2 = c_R c_R and c_t^2 = c_t c_t.
 * Outputs: adj -- per group g of size m_g, m_g rows of ceil(m_g / 64) 64-bit words at word_off[g]
 * (dpgo_hip_pair_consistency_words), bit l % 64 of word l / 64 of row k = A(k,l), padding bits zero, groups back to
 * back; degree[m] -- the row popcounts; e_rot / e_tra (each may be NULL; tests and diagnostics) -- dense m_g x m_g
 * doubles per group, entry (k,l) at k m_g + l, groups back to back at sum of the earlier m_g^2, refused when the sum
 * of m_g^2 passes DPGO_PCM_DENSE_MAX.  adj_capacity: the words the caller's adj holds (< 0: not checked).  m = 0 or ngroups = 0 writes
 * nothing.  DPGO_HIP_EINVAL for d outside {2, 3}, m < 0, ngroups < 0, a null required pointer, a group_off that
 * does not start at 0, descends or does not end at m, or a capacity below the words needed. */
#define DPGO_PCM_DENSE_MAX (1LL << 26)
/* word_off[ngroups + 1]: the offset of every group's rows in adj (word_off[ngroups] = the total).  capacity < 0:
 * no limit; else DPGO_HIP_EINVAL when the total passes it, as when it does not fit a long long. */
int dpgo_hip_pair_consistency_words(int ngroups, const int* group_off, long long* word_off, long long capacity);
/* Host pointers in and out; one kernel launch over a host-built table of (group, row tile, column tile) 64 x 64
 * tiles, one integer-atomic degree count.  Synchronises. */
int dpgo_hip_pair_consistency(int d, int m, const double* F, const double* x, int ngroups, const int* group_off,
                              double c_R, double c_t, unsigned long long* adj, long long adj_capacity, int* degree,
                              double* e_rot, double* e_tra);
/* The same on device pointers (group_off stays a host array: the tile table is built from it), queued on `stream`;
 * the call returns after the stream has run it (its tile table is released then). */
int dpgo_hip_pair_consistency_dev(int d, int m, const double* F_dev, const double* x_dev, int ngroups,
                                  const int* group_off, double c_R, double c_t, unsigned long long* adj_dev,
                                  long long adj_capacity, int* degree_dev, double* e_rot_dev, double* e_tra_dev,
                                  void* stream);
/* Measurement: the tile table is built and uploaded once, then warmup + reps launches (degree memset + kernel, no
 * dense outputs) run on the null stream, each between two HIP events; ms[reps] receives the timed launches'
 * milliseconds.  m >= 1. */
int dpgo_hip_pair_consistency_bench(int d, int m, const double* F_dev, const double* x_dev, int ngroups,
                                    const int* group_off, double c_R, double c_t, unsigned long long* adj_dev,
                                    long long adj_capacity, int* degree_dev, int warmup, int reps, double* ms);
/* The host twin: no device, the same bits (adj, degree, e_rot, e_tra). */
int dpgo_pair_consistency_host(int d, int m, const double* F, const double* x, int ngroups, const int* group_off,
                               double c_R, double c_t, unsigned long long* adj, long long adj_capacity, int* degree,
                               double* e_rot, double* e_tra);
/* Maximum clique of the graph on m vertices whose row k is adj_rows[k words_per_row ..] (bit l of the row = an
 * edge k-l; symmetric, zero diagonal and zero padding, as dpgo_hip_pair_consistency leaves a group: not checked).
 * Host only, deterministic, one thread: a bitset branch and bound (Tomita's colour bound, popcounts).  The first
 * incumbent is the greedy clique that walks the vertices by descending degree, ties to the lower index, and keeps
 * every vertex adjacent to all kept so far.  node_budget: the search nodes that may be expanded (< 0: no limit; 0:
 * the greedy clique alone).  proven = 1: the search finished and clique[0 .. size) is a maximum clique; proven = 0:
 * the best clique found within the budget.  Members ascending.  m = 0: size 0, proven 1.  DPGO_HIP_EINVAL for
 * m < 0, words_per_row < ceil(m / 64) or a null pointer (adj_rows may be NULL when m = 0). */
int dpgo_max_clique(int m, int words_per_row, const unsigned long long* adj_rows, long long node_budget, int* clique,
                    int* size, int* proven);

/* ---- measurement helpers ----------------------------------------------------------------*/
/* Select a compiled kernel variant / host sequence for A/B timing (process-wide; every setting gives
 * results within the documented bars, most bitwise the default's).  key 0: BSR X.Q SpMM
 * neighbour-loop variant 0 = 1 neighbour/step (default), 1 = same with non-temporal block loads,
 * 2 = 2 neighbours/step, 3 = 4 neighbours/step, 4 = 4 + XCD-aware tile remap, 5 = 2 + XCD remap,
 * 6 = 1 + XCD remap.  key 1: edge-stream variant for every SpMM mode (same numbering over
 * incidences; -1 = the compiled default).  key 2: epilogue operands ahead of the edge loop (1, default).
 * key 3: consumer-side tCG finalize (classic sequence).  key 4: first tCG step kind (0 predicted,
 * 1 each-edge-once pass, 2 full pass).  key 5: 1 = the classic five-launch tCG iteration instead of the
 * merged one.  key 6: 1 = HESS_M operands prefetched.  key 7: tCG queueing (0 adaptive, 1 one iteration
 * ahead, 2 all at once; the classic sequence of the exact preconditioner queues all at once only with 2).  key 8: 1 = second-visit record staging (set before Q).  key 9: 1 = the agent
 * status by its own pass instead of folded into the rho test.  key 10: merged tCG iterations of a small
 * batch (<= 4,096 tiles) in two agent halves on two streams (1, default; 0 off; 2 the halves out of phase).
 * key 16: merged tCG iterations queued at once in blocks of consecutive agents of at most this many tiles, each block's
 * iterations back to back (default 2000; 0 off; a batch of at most this many tiles is queued as without the key).
 * key 17: blocks in flight, 1..4 (block b on stream b % value; default 2).
 * DESIGN.md records each key's measurement.  These are the process DEFAULTS: a handle copies them when it is
 * created, so handles created afterwards follow; dpgo_hip_problem_set_tuning changes one existing handle. */
int dpgo_hip_set_tuning(int key, int value);
/* The exact preconditioner's factor of the handle (after a solve that used it): supernodes, tree levels, the
 * widest separator in 64-row tiles, panel doubles, and the last device factorisation's time (ms, 0 when it ran on
 * the host) with the number of device factorisations so far. */
int dpgo_hip_exact_factor_info(dpgo_hip_problem h, long long* nodes, int* levels, int* max_s_tiles,
                               long long* panel_doubles, double* factor_ms, int* factor_count);
/* Flop counts of one numeric factorisation of that factor (the roofline of dpgo_hip_exact_factor_info's factor_ms):
 * the classic supernodal Cholesky count sum_nodes s^3/3 + s^2 t + s t^2 (s, t = the node's S and R scalars; the
 * work CHOLMOD does for src/QuadraticProblem.cpp:37-41), and the extra flops of the panels' inverse blocks
 * [L_SS^-1; L_RS L_SS^-1] (s^3/3 + s^2 t per node) that make the solves dense products.  Zeros before a factor. */
int dpgo_hip_exact_factor_flops(dpgo_hip_problem h, double* cholesky_flops, double* inverse_flops);
/* The agents of the handle whose last exact factorisation met a non-positive pivot: QuadraticProblem::PreConditioner's
 * "Preconditioner failed" branch (src/QuadraticProblem.cpp:81-86) applies to them alone -- their output is their input,
 * unprojected -- while the batch's other agents keep their factors.  flags (K ints, may be null) receives 1 per such
 * agent, *count their number (0 before any factor).  Waits for the handle's stream. */
int dpgo_hip_exact_fallback_agents(dpgo_hip_problem h, int* flags, int* count);
/* The exact preconditioner's two sweeps over every agent of the handle (right-hand side V_dev, the handle's layout),
 * `reps` applications after 3 untimed ones, each timed with HIP events on the handle's stream: the forward sweep
 * (every level's k_sn_assemble + k_sn_fwd) and the backward sweep (every level's k_sn_bwd), ms per application, and
 * the bytes of the stored panel tiles (64 x 64, padding included). */
int dpgo_hip_bench_precond(dpgo_hip_problem h, const double* V_dev, int reps, double* ms_fwd, double* ms_bwd,
                           double* panel_bytes);
/* The panel bytes one application's sweeps read: every wide supernode's 64 x 64 tiles (padding included) and the
 * compact copy of every narrow one (at most 2 S column tiles: the backward sweep always, the forward sweep on levels
 * of narrow nodes only).  Zeros before a factor. */
int dpgo_hip_exact_sweep_bytes(dpgo_hip_problem h, double* fwd_bytes, double* bwd_bytes);
/* The process default of a tuning key. */
int dpgo_hip_get_tuning(int key, int* value);
/* The same keys on one existing handle (A/B timing of variants on one problem without rebuilding it). */
int dpgo_hip_problem_set_tuning(dpgo_hip_problem h, int key, int value);
/* Tuning key 16: the number of agent blocks the handle's last optimise call queued its merged tCG loop in (0: the
 * unblocked queueing ran), and the tile count of every agent of the batch (agent_tiles[num_agents]); either may be
 * null. */
int dpgo_hip_tcg_blocks(dpgo_hip_problem h, int* blocks_last, int* agent_tiles);
/* Algorithmic HBM bytes of one X.Q SpMM over this handle: BSR blocks + indices + X + Y, or, for
 * an edge-stream Q, every edge record once + 8 B per incidence + pointers + X + Y. */
double dpgo_hip_spmm_bytes(dpgo_hip_problem h);
/* SURVEY 8(d)'s algorithmic bytes of one X.Q SpMM over this handle's Q as explicit b x b blocks
 * (B_spmm = nnzb (b^2 8 + 4) + (n + 1) 4 + 2 r b n 8), whatever form the handle stores it in. */
double dpgo_hip_spmm_bytes_bsr(dpgo_hip_problem h);
/* Riemannian HVP timing: one EVAL at X_dev (S and the Riemannian gradient into V_dev), then `reps`
 * back-to-back Hessian-vector products HV_dev = Hess f(X)[V]; average ms per product in *ms. */
int dpgo_hip_bench_hvp(dpgo_hip_problem h, const double* X_dev, double* V_dev, double* HV_dev, int reps, double* ms);
/* Time `reps` back-to-back X.Q SpMM launches with HIP events on the handle's stream; returns the
 * average milliseconds per launch in *ms. */
int dpgo_hip_bench_spmm(dpgo_hip_problem h, const double* X_dev, double* Y_dev, int reps, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* DPGO_HIP_H */

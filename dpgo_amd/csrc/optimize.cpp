// The trust-region driver: host side of every colour update.  It decides which kernels are queued,
// in what order, on which stream, and when the host waits for a published status word.  All vector arithmetic and
// all scalar recurrences run on the GPU (kernels.hip); the host only sequences launches and, once per RTR Run, reads
// the per-agent "still running" flags to drive QuadraticOptimizer::trustRegion's radius-shrink retry loop
// (src/QuadraticOptimizer.cpp:92-110).  What a Run queues is decided by plan_run (tcg_plan.h); one function per
// queueing regime acts on it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "problem_internal.h"
#include "tcg_plan.h"

namespace dpgo {
namespace {

using Clock = std::chrono::high_resolution_clock;

// PGOAgent status pass (src/PGOAgent.cpp:700-716): |X_out - XPrev|^2 per agent, then OP_STATUS.
// `partials`: |X_out - st.ref|^2 per tile already there (nullptr: computed here into pa)
int status_pass(dpgo_hip_problem h, const double* X_out, const StatusArgs& st, const OptScalars& o0,
                const double* partials) {
  if (!partials) {
    auto c = make_ctx(h, FLAG_NONE, h->pa.p);
    HIP_TRY(launch_sqdiff(h->r, h->b, c, X_out, st.ref));
    partials = h->pa.p;
  }
  OptScalars o = o0;
  o.rel_tol = st.rel_tol;
  o.min_ratio = st.min_ratio;
  FinalizeArgs f = make_fin(h, OP_STATUS, partials, 1, nullptr, 0, &o);
  f.conv_ratio = st.conv_ratio;
  HIP_TRY(launch_finalize(f, h->K, h->stream));
  return DPGO_HIP_OK;
}

void fill_result(const AgentState& s, bool single, bool enabled, dpgo_opt_result* out) {
  std::memset(out, 0, sizeof(*out));
  out->success = enabled ? 1 : 0;
  out->fInit = s.f_init;
  out->gradNormInit = s.ngf_init;
  if (single) {
    const bool moved = s.runs > 0 && s.accepted && !s.gave_up;
    out->fOpt = moved ? s.f2 : s.f_init;
    out->gradNormOpt = moved ? s.ngf2 : s.ngf_init;
  } else {
    out->fOpt = s.f1;
    out->gradNormOpt = s.ngf;
  }
  out->relativeChange = s.rel_change;
  out->tCGStatus = s.tcg_status;
  out->runs = s.runs;
  out->outer_iters = s.outer_iters;
  out->inner_iters = s.tcg_iters;
  out->gave_up = s.gave_up;
}

// the RGD step's: f and |grad|^2 at the output come from the agent's sums (OP_SUM: f, |grad|^2), no tCG ran
void fill_result_rgd(const AgentState& s, bool enabled, const double* sums, dpgo_opt_result* out) {
  std::memset(out, 0, sizeof(*out));
  out->success = enabled ? 1 : 0;
  out->fInit = s.f_init;
  out->gradNormInit = s.ngf_init;
  out->fOpt = enabled ? sums[0] : s.f_init;
  out->gradNormOpt = enabled ? std::sqrt(sums[1]) : s.ngf_init;
  out->relativeChange = s.rel_change;
  out->tCGStatus = -1;
}

// One optimize call.  The first group of members holds for the whole call; the second is one Run's and is reset by
// begin_run (a call's Runs: the first and its radius-shrink retries, or the outer iterations of a multi-iteration RTR).
struct Driver {
  // ---- the call
  dpgo_hip_problem h = nullptr;
  dpgo_opt_params P;
  OptScalars o;
  const double* X_in = nullptr;
  double* X_out = nullptr;
  const StatusArgs* st = nullptr;
  dpgo_opt_result* results = nullptr;
  std::vector<int> en;          // per agent: enabled
  const int* en_dev = nullptr;  // the same on the device (nullptr: every agent)
  double *x1 = nullptr, *x2 = nullptr;
  bool single = false;     // RTR with one outer iteration
  bool exact = false;      // the exact preconditioner
  int pmode = PRECON_NONE; // the preconditioner the fused tCG kernels apply
  bool fused_tcg = false;  // the first evaluation also forms the first tCG start
  bool stats = false;      // results or verbose output were asked for
  bool direct = false;     // an accepted candidate is retracted straight into X_out
  bool g_valid = true;     // grad(x1) is in h->g (tcg_start_stores_grad, then true once a retry Run recomputed it)
  bool status_done = false;  // the status was folded into the last rho test for every agent
  Clock::time_point t0;
  // ---- one Run
  TcgPlan plan;
  std::vector<int> tags, step_tags;  // published tag per queued iteration (0: unpublished) / per step test
  bool tail_pending = false;  // this Run's last merged iteration was queued without its k_tcg_updir
  int launched = 0;           // iterations queued so far (the one-ahead regimes)
  bool cg_agents = false;     // some agent may still be in tCG after the first step test
  int rtag = 0;               // the tag of the Run's last rho test

  int r() const { return h->r; }
  int b() const { return h->b; }

  TcgPlanIn plan_in() const {
    TcgPlanIn in;
    in.rtr = P.algorithm == DPGO_ALG_RTR;
    in.single = single;
    in.exact = exact;
    in.tr_max_inner = P.tr_max_inner;
    in.status = st != nullptr;
    in.predict_boundary = h->predict_boundary;
    in.fuse_finalize = h->fuse_finalize;
    in.K = h->K;
    in.num_tiles = h->num_tiles;
    in.fuse_tcg = h->tuning[TUNE_FUSE_TCG];
    in.first_step = h->tuning[TUNE_FIRST_STEP];
    in.classic_tcg = h->tuning[TUNE_CLASSIC_TCG];
    in.lookahead = h->tuning[TUNE_TCG_LOOKAHEAD];
    in.status_pass = h->tuning[TUNE_STATUS_PASS];
    in.split_streams = h->tuning[TUNE_SPLIT_STREAMS];
    in.tail_fuse = h->tuning[TUNE_TAIL_FUSE];
    in.tcg_block = h->tuning[TUNE_TCG_BLOCK];
    return in;
  }

  // ---- set-up: parameters, the enabled mask, x1 / x2, the call-level flags
  int init(dpgo_hip_problem hh, const dpgo_opt_params* params, const double* Xin, double* Xout,
           const int* agent_enabled_host, dpgo_opt_result* res, const StatusArgs* status) {
    h = hh;
    X_in = Xin;
    X_out = Xout;
    results = res;
    st = status;
    DPGO_TRY(problem_ready(h));
    if (params)
      P = *params;
    else
      dpgo_hip_default_params(&P);
    if (P.tr_iterations < 1 || P.tr_max_inner < 0) return fail(DPGO_HIP_EINVAL, "bad optimizer parameters");
    DPGO_TRY(ensure_work_public(h));
    t0 = Clock::now();
    const int K = h->K;
    exact = P.precon == DPGO_PRECON_EXACT;
    if (exact) DPGO_TRY(sync_chol(h));
    // the exact solve runs as its own stages; the fused tCG kernels then see the identity
    pmode = P.precon == DPGO_PRECON_BLOCK_JACOBI ? PRECON_BLOCK_JACOBI : PRECON_NONE;
    en.assign(K, 1);
    if (agent_enabled_host)
      for (int a = 0; a < K; ++a) en[a] = agent_enabled_host[a] != 0;
    // (a pageable H2D copy would synchronise the stream: only copy when a mask is given)
    if (agent_enabled_host)
      HIP_TRY(hipMemcpyAsync(h->enabled.p, en.data(), sizeof(int) * K, hipMemcpyHostToDevice, h->stream));
    // without a mask every agent is enabled: k_finalize reads no mask (no fill launch)
    en_dev = agent_enabled_host ? h->enabled.p : nullptr;

    single = P.algorithm == DPGO_ALG_RTR && P.tr_iterations == 1;
    // x1 only moves in a multi-iteration Run; a single Run (the RBCD setting) reads X_in in place.
    x1 = h->x1.p;
    if (single || P.algorithm == DPGO_ALG_RGD) {
      x1 = const_cast<double*>(X_in);
    } else {
      HIP_TRY(hipMemcpyAsync(h->x1.p, X_in, h->vec_bytes(), hipMemcpyDeviceToDevice, h->stream));
    }
    std::memset(&o, 0, sizeof(o));
    o.tol = P.tr_tolerance;
    o.Delta0 = P.tr_initial_radius;
    o.Delta_max = single ? P.tr_initial_radius : 5.0 * P.tr_initial_radius;
    o.theta = 1.0;
    o.kappa = 0.1;
    o.min_inner = 0;
    o.max_iter = P.tr_iterations;
    o.single_run = single ? 1 : 0;
    const TcgPlanIn in = plan_in();
    fused_tcg = tcg_start_fused(in);
    g_valid = tcg_start_stores_grad(in);
    // Statistics nobody asked for are not computed: without results / verbose, the x2 evaluation of
    // a single Run needs f(x2) only (gradNormOpt is only printed, src/PGOAgent.cpp:1155-1161), and an
    // accepted candidate is retracted straight into X_out (only agents that did not move copy X_in).
    stats = results != nullptr || P.verbose;
    direct = single && !stats && X_out != X_in;
    x2 = direct ? X_out : h->x2.p;
    return DPGO_HIP_OK;
  }

  // f(x1), grad(x1), S(x1)  (QuadraticOptimizer::optimize :36-37, SolversTR start); for RTR the
  // first tCG start (delta = -Prec(grad), <z, grad>) is fused into the same pass
  int first_eval() {
    if (fused_tcg) {
      const FinalizeArgs fin = make_fin(h, OP_EVAL_TCG_INIT, h->pa.p, 3, nullptr, 0, &o, en_dev);
      DPGO_TRY(eval_at(h, x1, g_valid ? h->g.p : nullptr, h->S.p, h->pa.p, FLAG_NONE, MODE_EVAL_TCG, h->delta.p, pmode,
                       &fin));
    } else {
      DPGO_TRY(eval_at(h, x1, h->g.p, h->S.p, h->pa.p, FLAG_NONE));
      DPGO_TRY(finalize(h, OP_EVAL_INIT, h->pa.p, 2, nullptr, 0, &o, en_dev));
    }
    return DPGO_HIP_OK;
  }

  // one fixed-step Riemannian gradient step (QuadraticOptimizer::gradientDescent :124-149), the whole RGD call
  int rgd() {
    const int K = h->K;
    auto cr = make_ctx(h, FLAG_NONE, h->pb.p);
    HIP_TRY(launch_retract(r(), b(), cr, x1, h->g.p, -P.rgd_stepsize, h->x2.p, nullptr, nullptr));
    HIP_TRY(hipMemcpyAsync(h->use_a.p, en.data(), sizeof(int) * K, hipMemcpyHostToDevice, h->stream));
    // X_in may alias X_out (in-place update): the candidate stays in x2 until the select
    auto cs = make_ctx(h, FLAG_NONE, h->pa.p);
    // one pass: X_out = x2 and the partials |X_out - X_in|^2 (pa).  When the status reference is X_in
    // (PGOAgent's XPrev), those partials ARE the status's: an in-place update (X_out == X_in, the engine's)
    // has overwritten X_in by now, so they must not be recomputed from memory.
    HIP_TRY(launch_select(r(), b(), cs, h->x2.p, x1, h->use_a.p, x1, X_out));
    if (stats) DPGO_TRY(finalize(h, OP_REL_CHANGE, h->pa.p, 1, nullptr, 0));
    if (st) DPGO_TRY(status_pass(h, X_out, *st, o, st->ref == X_in ? h->pa.p : nullptr));
    if (!stats) return DPGO_HIP_OK;
    DPGO_TRY(eval_at(h, X_out, h->g2.p, h->S2.p, h->pb.p, FLAG_NONE));
    DPGO_TRY(finalize(h, OP_SUM, h->pb.p, 2, nullptr, 0));
    DPGO_TRY(download_sums(h));
    DPGO_TRY(download_state(h));
    const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    for (int a = 0; results && a < K; ++a) {
      fill_result_rgd(h->h_state[a], en[a] != 0, &h->h_sums[a * 4], &results[a]);
      results[a].elapsedMs = std::floor(ms);
    }
    return DPGO_HIP_OK;
  }

  // ---- a Run begins: its plan (predict_boundary may have changed since the last Run), and the tCG start unless the
  // first evaluation already formed it
  int begin_run(int round) {
    plan = plan_run(plan_in(), h->h_agent_tile_off.data());
    tags.clear();
    step_tags.clear();
    tail_pending = false;
    launched = 0;
    rtag = 0;
    cg_agents = !plan.qf0;
    if (round == 0) h->tcg_blocks_last = 0;  // (a call's Runs: the first and its radius-shrink retries)
    if (plan.regime == TcgRegime::MergedBlocked) h->tcg_blocks_last = static_cast<int>(plan.blocks.size()) - 1;
    // ---- truncated CG (A.4)
    if (round > 0 || !fused_tcg) {
      if (!g_valid) {  // a retry Run restarts tCG from grad(x1), which EVAL_TCG did not store
        DPGO_TRY(eval_at(h, x1, h->g.p, h->S.p, h->pa.p, FLAG_RUN, MODE_EVAL_TCG, h->delta.p, pmode));
        g_valid = true;
      }
      if (exact) {  // delta = -P_X(g P^-1), partials <z, g>, |g|^2
        DPGO_TRY(exact_precond(h, h->g.p, nullptr, h->delta.p, x1, h->g.p, h->pa.p, FLAG_RUN));
      } else {
        auto ci = make_ctx(h, FLAG_RUN, h->pa.p);
        HIP_TRY(launch_tcg_init(r(), b(), ci, x1, h->minv.p, pmode, h->g.p, h->delta.p));
      }
      DPGO_TRY(finalize(h, OP_TCG_INIT, h->pa.p, 2, nullptr, 0, &o));
    }
    return DPGO_HIP_OK;
  }

  // ---- the classic sequence's launches
  // iteration j's step test: Hdelta = Hess[delta] and d_Hd = <delta, Hdelta> (MODE_HESS); for the
  // first step d_Hd by the each-edge-once formula, alone (MODE_QF) or with Hdelta stored (MODE_HESS_QF)
  int launch_step(int mode) {
    auto ch = make_ctx(h, FLAG_TCG, h->pa.p);
    // the step test publishes too: when it already stopped every agent (a boundary or
    // negative-curvature step, the common RBCD case) the host launches no further iteration
    const int stag = next_tag(h);
    step_tags.push_back(stag);
    const bool qf = mode == MODE_QF;
    const SpmmArgs sa{h->delta.p, nullptr, nullptr, x1, h->S.p, qf ? nullptr : h->Hdelta.p, nullptr,
                      nullptr, nullptr, PRECON_NONE};
    if (plan.fuse_tcg && mode == MODE_HESS) return spmm_launch(h, mode, ch, sa);  // decided by the update
    OptScalars os = o;
    os.first_full = mode == MODE_HESS_QF ? 1 : 0;
    return spmm_then_finalize(h, mode, ch, sa, make_fin(h, OP_TCG_STEP, h->pa.p, 1, nullptr, 0, &os, nullptr, 1, stag));
  }

  // the rest of iteration j: update, stopping test, direction.
  // step_decided: the first step after a QF step test was decided by the QF pass's finalize
  int launch_rest(int j, bool step_decided) {
    auto cu = make_ctx(h, FLAG_TCG_MODE, h->pb.p);
    const bool fs = plan.fuse_tcg && !step_decided;
    const FinalizeArgs fstep = make_fin(h, OP_TCG_STEP, h->pa.p, 1, nullptr, 0, &o, nullptr, 1, step_tags[j]);
    HIP_TRY(launch_tcg_update(r(), b(), cu, x1, h->minv.p, pmode, h->delta.p, h->Hdelta.p, h->eta.p,
                              j == 0 ? h->g.p : h->rv.p, h->rv.p, h->z.p, j == 0 ? 1 : 0, fs ? &fstep : nullptr,
                              h->arrive.p));
    if (exact)  // z = Prec(r) with the factor; replaces the identity z and its partials
      DPGO_TRY(exact_precond(h, h->rv.p, h->z.p, nullptr, x1, h->rv.p, h->pb.p, FLAG_TCG_MODE));
    const int tag = next_tag(h);
    tags.push_back(tag);
    const FinalizeArgs fcheck = make_fin(h, OP_TCG_CHECK, h->pb.p, 3, nullptr, 0, &o, nullptr, 1, tag);
    const bool dir = j + 1 < P.tr_max_inner;  // the last direction update is never used
    if (!(plan.fuse_tcg && dir)) HIP_TRY(launch_finalize(fcheck, h->K, h->stream));
    if (dir) {
      auto cd = make_ctx(h, FLAG_TCG, nullptr);
      HIP_TRY(launch_tcg_dir(r(), b(), cd, h->z.p, h->delta.p, plan.fuse_tcg ? &fcheck : nullptr, h->arrive.p));
    }
    return DPGO_HIP_OK;
  }

  // ---- the merged iteration
  // Iteration j over agents [a0, a1) on `on`: tiles, partial slots and finalize rows of that agent range; every
  // kernel of the iteration reads and writes only those agents' poses (Q and the tCG vectors are block-diagonal over
  // agents), so agent groups are independent and each agent's arithmetic is the unsplit launch's, bit for bit.
  // order_h / order_u: the tile orders of the iteration's HESS_M and k_tcg_updir, drawn by the caller once per
  // iteration so that every agent group runs a phase in the same direction (each group's own tiles then alternate
  // launch by launch).  pub_tag: the status tag its finalize publishes (0: it publishes none).
  // TUNE_TAIL_FUSE: the last iteration's k_tcg_updir is not launched; every path to the last iteration comes through
  // here, which sets tail_pending instead of launching, and launch_candidate hands it to the retraction.  Both
  // kernels would read the state the last OP_TCG_STEP_CHECK / OP_TCG_CHECK_M left: no finalize runs between them.
  int launch_merged_range(int j, int mode, int flag, int op, int a0, int a1, hipStream_t on, int order_h, int order_u,
                          int pub_tag) {
    const int t0 = h->h_agent_tile_off[a0], t1 = h->h_agent_tile_off[a1];
    if (t1 == t0) return DPGO_HIP_OK;
    const LaunchCtx ch = range_ctx(flag, h->pa.p, t0, t1, on, order_h);
    SpmmArgs sa{h->delta.p, nullptr, nullptr, x1, h->S.p, h->Hdelta.p, nullptr, h->minv.p, nullptr, pmode};
    sa.rvec = j == 0 ? h->g.p : h->rv.p;
    // |r_j|^2 and <z_j, r_j>: from the previous k_tcg_updir's partials (peh), formed by the SpMM itself on
    // the first iteration (r_0 = grad)
    const bool rz_pc = j > 0;
    sa.rz_own = rz_pc ? 0 : 1;
    OptScalars os = o;
    os.first_full = mode == MODE_HESS_QF_M ? 1 : 0;
    FinalizeArgs fin = make_fin(h, op, h->pa.p, 7, nullptr, 0, &os, nullptr, pub_tag ? 1 : 0, pub_tag);
    fin.pc = h->peh.p;
    fin.nq_c = 1;
    fin.dd_mask = merged_dd_mask(h->fmt, h->tuning);  // which merged partials are double-double
    fin.rz_pc = rz_pc ? 1 : 0;
    fin.agent_tile_off += a0;  // tile offsets stay global: the partial slots are the unsplit ones
    fin.agent_num_poses += a0;
    fin.state += a0;
    fin.out_sums += 4 * a0;
    if (fin.trace) fin.trace += static_cast<long>(a0) * fin.trace_cap * kTraceWidth;
    if (a0 == 0 && a1 == h->K && on == h->stream) {  // the whole batch: the finalize may be fused into the SpMM
      DPGO_TRY(spmm_then_finalize(h, mode, ch, sa, fin));
    } else {
      DPGO_TRY(spmm_launch(h, mode, ch, sa));
      HIP_TRY(launch_finalize(fin, a1 - a0, on));
    }
    if (plan.tail_fuse && j + 1 == P.tr_max_inner) {  // every group's last step waits for the (unsplit) retraction
      tail_pending = true;
      return DPGO_HIP_OK;
    }
    const LaunchCtx cu = range_ctx(FLAG_TCG_MODE, h->peh.p, t0, t1, on, order_u);
    HIP_TRY(launch_tcg_updir(r(), b(), cu, x1, h->minv.p, pmode, h->delta.p, h->Hdelta.p, h->eta.p,
                             j == 0 ? h->g.p : h->rv.p, h->rv.p, j == 0 ? 1 : 0, j + 1 == P.tr_max_inner ? 1 : 0));
    return DPGO_HIP_OK;
  }

  // the launch context of tiles [t0, t1) on `on`
  LaunchCtx range_ctx(int flag, double* partials, int t0, int t1, hipStream_t on, int order) const {
    LaunchCtx c = make_ctx_order(h, flag, partials + static_cast<long>(t0) * kPartialStride, order);
    c.tile_agent += t0;
    c.tile_start += t0;
    c.tile_count += t0;
    if (c.tile_meta) c.tile_meta += t0;
    c.num_tiles = t1 - t0;
    c.stream = on;
    return c;
  }

  // the two tile orders of one merged iteration, in launch order
  // (a fused last iteration launches no k_tcg_updir and draws no order for it: the retraction draws it)
  void draw_orders(int j, int* order_h, int* order_u) {
    *order_h = tile_order_next(h);
    *order_u = plan.tail_fuse && j + 1 == P.tr_max_inner ? 0 : tile_order_next(h);
  }

  // the whole batch on the launch stream
  int launch_merged(int j, int mode, int flag, int op, bool publish = true) {
    int oh, ou;
    draw_orders(j, &oh, &ou);
    const int tag = publish ? next_tag(h) : 0;
    tags.push_back(tag);
    return launch_merged_range(j, mode, flag, op, 0, h->K, h->stream, oh, ou, tag);
  }

  // ---- the candidate x2 = R_x1(eta), f(x2) and the rho test (radius update); *tag_out: the rho test's status tag
  int launch_candidate(int run_flag, int filter, int* tag_out) {
    auto cr = make_ctx(h, run_flag, h->pa.p);
    // a pending last step: its partial goes to peh (the rho test's FinalizeArgs::pc below), the retraction's to pa
    const RetractTail tail{h->delta.p, h->Hdelta.p, h->peh.p, P.tr_max_inner == 1 ? 1 : 0};
    const bool with_tail = tail_pending && run_flag != FLAG_RUN_IMPL;
    HIP_TRY(launch_retract(r(), b(), cr, x1, h->eta.p, 1.0, x2, h->g.p, nullptr, h->delta.p,
                           plan.status_fold ? st->ref : nullptr, with_tail ? &tail : nullptr));
    if (with_tail) tail_pending = false;
    // single Run: only f(x2) and |grad(x2)| are consumed (fOpt / gradNormOpt), |grad(x2)| only as a
    // statistic
    *tag_out = next_tag(h);
    OptScalars orho = o;
    orho.tail_fused = with_tail ? 1 : 0;
    if (plan.status_fold) {
      orho.status_fold = 1;
      orho.rel_tol = st->rel_tol;
      orho.min_ratio = st->min_ratio;
    }
    FinalizeArgs fin =
        make_fin(h, OP_RHO, h->pa.p, plan.status_fold ? 4 : 2, h->pb.p, 2, &orho, nullptr, 2, *tag_out, filter);
    if (plan.status_fold) fin.conv_ratio = st->conv_ratio;
    if (plan.merged) {  // the last k_tcg_updir's <eta_old, Hdelta>, folded before the rho test
      fin.pc = h->peh.p;
      fin.nq_c = 1;
    }
    if (single)
      return eval_at(h, x2, nullptr, nullptr, h->pb.p, run_flag, stats ? MODE_EVAL : MODE_F, nullptr, PRECON_NONE,
                     &fin);
    return eval_at(h, x2, h->g2.p, h->S2.p, h->pb.p, run_flag, MODE_EVAL, nullptr, PRECON_NONE, &fin);
  }

  // ---- the split streams (TUNE_SPLIT_STREAMS' agent groups, TUNE_TCG_BLOCK's blocks): group 0 runs on the launch
  // stream, group s on split_stream[s - 1]
  hipStream_t split_on(int s) const { return s == 0 ? h->stream : h->split_stream[s - 1]; }

  // streams and events for n groups: created once per handle, when first needed
  int ensure_split(int n) {
    if (n > 1 && !h->split_fork) HIP_TRY(hipEventCreateWithFlags(&h->split_fork, hipEventDisableTiming));
    for (int s = 0; s + 1 < n; ++s) {
      if (!h->split_stream[s]) HIP_TRY(hipStreamCreateWithFlags(&h->split_stream[s], hipStreamNonBlocking));
      if (!h->split_join[s]) HIP_TRY(hipEventCreateWithFlags(&h->split_join[s], hipEventDisableTiming));
    }
    return DPGO_HIP_OK;
  }

  // streams 1 .. n - 1 start after what the launch stream holds now
  int fork(int n) {
    if (n <= 1) return DPGO_HIP_OK;
    HIP_TRY(hipEventRecord(h->split_fork, h->stream));
    for (int s = 1; s < n; ++s) HIP_TRY(hipStreamWaitEvent(split_on(s), h->split_fork, 0));
    return DPGO_HIP_OK;
  }

  // the launch stream goes on after what streams 1 .. n - 1 hold now
  int join(int n) {
    for (int s = 1; s < n; ++s) {
      HIP_TRY(hipEventRecord(h->split_join[s - 1], split_on(s)));
      HIP_TRY(hipStreamWaitEvent(h->stream, h->split_join[s - 1], 0));
    }
    return DPGO_HIP_OK;
  }

  // ---- the queueing regimes
  // Block b runs its tr_max_inner iterations back to back on stream b % S (0: the launch stream, s:
  // split_stream[s - 1]), so two touches of a block's lines are one block launch apart instead of one batch
  // launch and at most S blocks are in flight.  Queued wave by wave (S blocks), a wave's blocks interleaved per
  // iteration so every stream has work from the first launches on.  One pair of tile orders per wave and
  // iteration: each block's consecutive launches alternate direction.
  int run_merged_blocked() {
    const std::vector<int>& blocks = plan.blocks;
    const int B = static_cast<int>(blocks.size()) - 1;
    const int S = std::max(1, std::min({h->tuning[TUNE_TCG_BLOCK_STREAMS], 4, B}));
    static_assert(dpgo_hip_problem_s::kMaxSplit >= 4, "streams of TUNE_TCG_BLOCK_STREAMS");
    DPGO_TRY(ensure_split(S));
    DPGO_TRY(fork(S));
    for (int w = 0; w < B; w += S) {
      for (int j = 0; j < P.tr_max_inner; ++j) {
        const int mode = j == 0 ? MODE_HESS_QF_M : MODE_HESS_M;
        int oh, ou;
        draw_orders(j, &oh, &ou);
        for (int s = 0; s < S && w + s < B; ++s)
          DPGO_TRY(launch_merged_range(j, mode, FLAG_TCG, OP_TCG_STEP_CHECK, blocks[w + s], blocks[w + s + 1],
                                       split_on(s), oh, ou, 0));
      }
    }
    DPGO_TRY(join(S));
    cg_agents = true;
    return DPGO_HIP_OK;
  }

  // groups of agents [a_g, a_g+1): two halves (values 1, 2), four groups (3) or one group per agent up to
  // eight (4); group 0 on the launch stream, group g on split_stream[g - 1]
  int run_merged_split() {
    const int K = h->K;
    const int sv = h->tuning[TUNE_SPLIT_STREAMS];
    const int G = std::min(K, sv == 3 ? 4 : sv >= 4 ? dpgo_hip_problem_s::kMaxSplit : 2);
    DPGO_TRY(ensure_split(G));
    auto first = [K, G](int g) { return static_cast<int>(static_cast<long>(K) * g / G); };
    // value 2: the second half starts once the first half's first iteration is done, so the two halves run
    // out of phase (one half's HESS_M beside the other's k_tcg_updir) rather than side by side
    const bool offset = sv == 2 && G == 2;
    if (!offset) DPGO_TRY(fork(G));
    for (int j = 0; j < P.tr_max_inner; ++j) {
      const int mode = j == 0 ? MODE_HESS_QF_M : MODE_HESS_M;
      int oh, ou;
      draw_orders(j, &oh, &ou);
      DPGO_TRY(launch_merged_range(j, mode, FLAG_TCG, OP_TCG_STEP_CHECK, first(0), first(1), split_on(0), oh, ou, 0));
      if (offset && j == 0) DPGO_TRY(fork(G));
      for (int g = 1; g < G; ++g)
        DPGO_TRY(launch_merged_range(j, mode, FLAG_TCG, OP_TCG_STEP_CHECK, first(g), first(g + 1), split_on(g), oh, ou,
                                     0));
    }
    DPGO_TRY(join(G));
    cg_agents = true;
    return DPGO_HIP_OK;
  }

  int run_merged_all_ahead() {
    for (int j = 0; j < P.tr_max_inner; ++j)
      DPGO_TRY(launch_merged(j, j == 0 ? MODE_HESS_QF_M : MODE_HESS_M, FLAG_TCG, OP_TCG_STEP_CHECK, false));
    cg_agents = true;
    return DPGO_HIP_OK;
  }

  // first step: MODE_QF (boundary predicted; CG-step agents then get a HESS_M pass and the stopping
  // test alone) or the full HESS_QF_M pass; one published status per iteration, one iteration queued
  // ahead of the status the host waits for
  int run_merged_one_ahead() {
    if (plan.full0) {
      DPGO_TRY(launch_merged(0, MODE_HESS_QF_M, FLAG_TCG, OP_TCG_STEP_CHECK));
    } else {
      DPGO_TRY(launch_step(MODE_QF));
      if (plan.spec) DPGO_TRY(launch_candidate(FLAG_RUN_IMPL, 1, &rtag));
    }
    launched = 1;
    for (int j = 0; j < P.tr_max_inner; ++j) {
      bool act = false;
      if (j == 0 && !plan.full0) {
        DPGO_TRY(wait_published(h, step_tags[0], &act));  // after the QF step test
        h->predict_boundary = !act;
        cg_agents = act;
        if (!act) break;
        if (!g_valid)  // the CG-step agents' gradient (EVAL_TCG skipped storing it; same pass again)
          DPGO_TRY(eval_at(h, x1, h->g.p, h->S.p, h->pa.p, FLAG_TCG_CG, MODE_EVAL_TCG, h->delta.p, pmode));
        DPGO_TRY(launch_merged(0, MODE_HESS_M, FLAG_TCG_CG, OP_TCG_CHECK_M));
      }
      if (launched < P.tr_max_inner) {  // lookahead: iteration j+1 queued while j runs
        DPGO_TRY(launch_merged(launched, MODE_HESS_M, FLAG_TCG, OP_TCG_STEP_CHECK));
        ++launched;
      }
      DPGO_TRY(wait_published(h, tags[j], &act));  // after iteration j's step and stopping tests
      if (j == 0 && plan.full0) {
        h->predict_boundary = !act;
        cg_agents = act;
      }
      if (!act) break;
    }
    return DPGO_HIP_OK;
  }

  // the classic sequence's first step test (and, with the exact preconditioner, the rest of iteration 0)
  int launch_classic_first() {
    DPGO_TRY(launch_step(plan.full0 ? MODE_HESS_QF : plan.qf0 ? MODE_QF : MODE_HESS));
    if (plan.spec) DPGO_TRY(launch_candidate(FLAG_RUN_IMPL, 1, &rtag));
    if (!plan.qf0) DPGO_TRY(launch_rest(0, false));
    launched = 1;
    return DPGO_HIP_OK;
  }

  int run_classic_all_ahead() {
    DPGO_TRY(launch_classic_first());
    for (; launched < P.tr_max_inner; ++launched) {
      DPGO_TRY(launch_step(MODE_HESS));
      DPGO_TRY(launch_rest(launched, false));
    }
    cg_agents = true;
    return DPGO_HIP_OK;
  }

  // one published status per step test and per stopping test, one iteration queued ahead of the one the host waits for
  int run_classic_one_ahead() {
    DPGO_TRY(launch_classic_first());
    for (int j = 0; j < P.tr_max_inner; ++j) {
      bool act = false;
      DPGO_TRY(wait_published(h, step_tags[j], &act));  // after the step test of iteration j
      if (j == 0) {
        h->predict_boundary = !act;
        cg_agents = act;
      }
      if (!act) break;
      if (j == 0 && plan.qf0) {
        if (!g_valid)  // the CG-step agents' gradient (EVAL_TCG skipped storing it; same pass again)
          DPGO_TRY(eval_at(h, x1, h->g.p, h->S.p, h->pa.p, FLAG_TCG_CG, MODE_EVAL_TCG, h->delta.p, pmode));
        if (!plan.full0) {  // Hess[delta] of the agents taking a CG step (the QF pass did not form it)
          auto cg = make_ctx(h, FLAG_TCG_CG, h->pb.p);
          DPGO_TRY(spmm_launch(h, MODE_HESS, cg,
                               SpmmArgs{h->delta.p, nullptr, nullptr, x1, h->S.p, h->Hdelta.p, nullptr, nullptr,
                                        nullptr, PRECON_NONE}));
        }
        DPGO_TRY(launch_rest(0, true));
      }
      if (launched < P.tr_max_inner) {  // lookahead: iteration j+1 queued while j's update runs
        DPGO_TRY(launch_step(MODE_HESS));
        DPGO_TRY(launch_rest(launched, false));
        ++launched;
      }
      DPGO_TRY(wait_published(h, tags[j], &act));  // after the stopping test of iteration j
      if (!act) break;
    }
    return DPGO_HIP_OK;
  }

  // Host control without stream synchronisation: k_finalize publishes each agent's tCG / Run flag
  // to host-mapped memory; the host keeps one tCG iteration of launches queued ahead of the flag
  // it is waiting for, so the GPU never drains (agents that finished skip their tiles).
  int run_tcg() {
    switch (plan.regime) {
      case TcgRegime::None: return DPGO_HIP_OK;
      case TcgRegime::ClassicOneAhead: return run_classic_one_ahead();
      case TcgRegime::ClassicAllAhead: return run_classic_all_ahead();
      case TcgRegime::MergedOneAhead: return run_merged_one_ahead();
      case TcgRegime::MergedAllAhead: return run_merged_all_ahead();
      case TcgRegime::MergedSplit: return run_merged_split();
      case TcgRegime::MergedBlocked: return run_merged_blocked();
    }
    return fail(DPGO_HIP_ESTATE, "unknown tCG regime");
  }

  // ---- candidate x2 = R_x1(eta), rho test, radius update: of every agent, or (first steps queued speculatively
  // behind the step test) of the agents that went on into tCG
  int run_candidate() {
    if (!plan.spec) return launch_candidate(FLAG_RUN, 0, &rtag);
    if (cg_agents) return launch_candidate(FLAG_RUN_EXPL, 2, &rtag);
    return DPGO_HIP_OK;
  }

  // what the Run's outcome moves: x1 (multi-iteration), or X_out for the agents it decided (single Run)
  int accept_or_select(int round) {
    if (!single) {
      auto ca = make_ctx(h, FLAG_NONE, nullptr);
      HIP_TRY(launch_accept(r(), b(), ca, h->x2.p, h->g2.p, h->S2.p, h->x1.p, h->g.p, h->S.p));
    } else if (!direct) {
      // speculative output, queued before the host knows whether another Run follows: the agents whose
      // outcome this Run decided write X_out = accepted ? x2 : X_in, once (X_out may alias X_in), and
      // their |X_out - X_in|^2 partials into pc; agents that retry are written by a later Run
      auto cs = make_ctx(h, FLAG_DECIDED, h->pc.p);
      cs.round = round;
      HIP_TRY(launch_select(r(), b(), cs, h->x2.p, X_in, nullptr, X_in, X_out));
    } else {
      // x2 already sits in X_out: agents that did not move take X_in (queued before the retry
      // decision; a retry Run retracts into X_out again and repeats this)
      auto cm = make_ctx(h, FLAG_MOVED, h->pa.p);
      HIP_TRY(launch_select(r(), b(), cm, X_in, X_in, nullptr, X_in, X_out));
    }
    return DPGO_HIP_OK;
  }

  // radius-shrink retry / next outer iteration needed?  (waits for the Run's rho test)
  int another_run(bool* again) {
    bool any = false, any_cg = false, any_never = false;
    DPGO_TRY(wait_published(h, rtag, &any, &any_cg, &any_never));
    status_done = plan.status_fold && !any_never && !any;
    // (published by the rho test: no status inside tCG)
    if (queued_all_ahead(plan.regime)) h->predict_boundary = !any_cg;
    *again = any;
    return DPGO_HIP_OK;
  }

  // ---- output select, status, results
  int finish() {
    const int K = h->K;
    // X_out: accepted candidate or the input (single Run), x1 (multi-iteration)
    auto cs = make_ctx(h, FLAG_NONE, h->pc.p);  // (drawn for a single Run too: the serpentine sequence)
    if (!single) {
      HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->use_a.p), 1, K, h->stream));
      HIP_TRY(launch_select(r(), b(), cs, x1, X_in, h->use_a.p, X_in, X_out));
    }
    // QuadraticOptimizer relativeChange against the input (the output select's partials, ref X_in)
    if (stats) DPGO_TRY(finalize(h, OP_REL_CHANGE, h->pc.p, 1, nullptr, 0));
    if (st && !status_done) {
      // the output select left |X_out - X_in|^2 in pc: reuse it when the status reference is X_in
      // itself (an in-place update without acceleration)
      const bool reuse = st->ref == X_in && !direct;
      DPGO_TRY(status_pass(h, X_out, *st, o, reuse ? h->pc.p : nullptr));
    }
    if (!stats) return DPGO_HIP_OK;  // no host round trip needed
    DPGO_TRY(download_state(h));
    const double ms = std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
    for (int a = 0; results && a < K; ++a) {
      fill_result(h->h_state[a], single, en[a] != 0, &results[a]);
      results[a].elapsedMs = std::floor(ms);
    }
    if (P.verbose) {
      for (int a = 0; a < K; ++a) {
        const AgentState& s = h->h_state[a];
        std::printf("[dpgo_hip] agent %d: f %.6g -> %.6g, |g| %.6g -> %.6g, runs %d, tCG %d (%d its)\n", a, s.f_init,
                    single ? s.f2 : s.f1, s.ngf_init, single ? s.ngf2 : s.ngf, s.runs, s.tcg_status, s.tcg_iters);
      }
    }
    return DPGO_HIP_OK;
  }
};

}  // namespace

// --------------------------------------------------------------------------- optimisation
int optimize_dev_status(dpgo_hip_problem h, const dpgo_opt_params* params, const double* X_in, double* X_out,
                        const int* agent_enabled_host, dpgo_opt_result* results, const StatusArgs* st) {
  Driver d;
  DPGO_TRY(d.init(h, params, X_in, X_out, agent_enabled_host, results, st));
  DPGO_TRY(d.first_eval());
  if (d.P.algorithm == DPGO_ALG_RGD) return d.rgd();
  if (d.P.tr_max_inner == 0) HIP_TRY(hipMemsetAsync(h->eta.p, 0, h->vec_bytes(), h->stream));
  // a single Run retries with a shrunk radius (QuadraticOptimizer::trustRegion); otherwise one Run per outer iteration
  const int max_rounds = d.single ? 12 : d.P.tr_iterations;
  for (int round = 0; round < max_rounds; ++round) {
    DPGO_TRY(d.begin_run(round));
    DPGO_TRY(d.run_tcg());
    DPGO_TRY(d.run_candidate());
    DPGO_TRY(d.accept_or_select(round));
    if (round + 1 < max_rounds) {
      bool again = false;
      DPGO_TRY(d.another_run(&again));
      if (!again) break;
    }
  }
  return d.finish();
}

bool merged_split(dpgo_hip_problem h) {
  return merged_split(h->K, h->num_tiles, h->fuse_finalize, h->tuning[TUNE_SPLIT_STREAMS]);
}

void merged_blocks(dpgo_hip_problem h, std::vector<int>* blocks) {
  merged_blocks(h->K, h->num_tiles, h->fuse_finalize, h->tuning[TUNE_TCG_BLOCK], h->h_agent_tile_off.data(), blocks);
}

}  // namespace dpgo

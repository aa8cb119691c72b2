// Internal (non-ABI) view of a dpgo_hip_problem, shared by capi.cpp, optimize.cpp and rbcd.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dpgo_hip.h"
#include "kernels.h"
#include "sn_schedule.h"

namespace dpgo {

int fail(int code, const std::string& msg);
inline int check_handle(dpgo_hip_problem h) { return h ? DPGO_HIP_OK : fail(DPGO_HIP_EINVAL, "null problem handle"); }
int usable_devices();

// Debug runs (DPGO_POISON=1): every fresh device allocation, and the exact preconditioner's frontal / panel /
// sweep buffers before each factorisation and application, are filled with 0xFF bytes -- a NaN in every double --
// so a kernel that reads an entry nothing wrote yields NaN instead of a plausible stale value.
bool poison_enabled();
hipError_t poison_fill(void* p, size_t bytes, hipStream_t stream);

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return ::dpgo::fail(DPGO_HIP_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

#define DPGO_TRY(expr)                  \
  do {                                  \
    int _rc = (expr);                   \
    if (_rc != DPGO_HIP_OK) return _rc; \
  } while (0)

struct HostBSR {
  std::vector<int> rowptr, col;
  std::vector<double> blocks;
};

// One agent's Q as its measurement stream (QFMT_EDGES): agent-local endpoints (-1 = the endpoint
// lives in another agent), R (d*d row-major), t (d), and the weighted precisions w kappa, w tau.
struct HostEdges {
  std::vector<int> p1, p2;
  std::vector<double> R, t, kw, tw, kappa0, tau0;  // kw = w kappa0, tw = w tau0
};

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  unsigned alloc_flags = 0;  // hipExtMallocWithFlags flags (e.g. hipDeviceMallocContiguous); hipMalloc if it fails
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n), alloc_flags(o.alloc_flags) {
    o.p = nullptr;
    o.n = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {  // by exchange: o leaves with this buffer's allocation
    std::swap(p, o.p);
    std::swap(n, o.n);
    std::swap(alloc_flags, o.alloc_flags);
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    release();
    n = std::max<size_t>(count, 1);
    hipError_t e = hipErrorMemoryAllocation;
    if (alloc_flags != 0) {
      e = hipExtMallocWithFlags(reinterpret_cast<void**>(&p), n * sizeof(T), alloc_flags);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        p = nullptr;
      }
    }
    if (e != hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e != hipSuccess || !poison_enabled()) return e;
    const hipError_t f = poison_fill(p, n * sizeof(T), nullptr);
    return f != hipSuccess ? f : hipDeviceSynchronize();
  }
};

// A pair of events owned by its holder, movable with it (the device factorisation's timing window)
struct EventPair {
  hipEvent_t e[2] = {nullptr, nullptr};
  EventPair() = default;
  EventPair(const EventPair&) = delete;
  EventPair& operator=(const EventPair&) = delete;
  EventPair(EventPair&& o) noexcept : e{o.e[0], o.e[1]} { o.e[0] = o.e[1] = nullptr; }
  EventPair& operator=(EventPair&& o) noexcept {
    std::swap(e[0], o.e[0]);
    std::swap(e[1], o.e[1]);
    return *this;
  }
  ~EventPair() {
    for (auto x : e)
      if (x) (void)hipEventDestroy(x);
  }
  hipEvent_t& operator[](int i) { return e[i]; }
  hipEvent_t* begin() { return e; }
  hipEvent_t* end() { return e + 2; }
};

// The exact preconditioner's device state (exact.cpp): supernodal Cholesky of Q + 0.1 I (chol.cpp), one launch per
// tree level and sweep.  The tables are SnSchedule's (sn_schedule.h), uploaded under the same names.
struct ExactPrecond {
  int state = 0;  // 0 stale, 1 ready, 2 Q + 0.1 I not positive definite (identity, as the reference)
  long nodes = 0;          // supernodes of the current symbolic structure (s may be larger: capacity)
  long panel_doubles = 0;  // doubles of the stored tiles (guard gaps included)
  DevBuf<double> panel, F, U;
  DevBuf<long> panel_off, f_off, u_off;
  DevBuf<int> s, t, poses_off, poses, cpos_off, cpos;
  DevBuf<int2> contrib, items;
  DevBuf<int> node_agent;       // [nodes] batch agent of each supernode (per-agent skip in the sweeps)
  std::vector<SnLevel> levels;  // index = depth (0 = the roots)
  // narrow supernodes' compact panels (SnView::cpanel): per node its offset (-1: tiles only), the copy's items
  // (node, 64-row block) for launch_sn_compact after every factorisation, and the bytes a sweep then reads
  DevBuf<double> cpanel;
  DevBuf<long> cpanel_off;
  DevBuf<int2> citems;
  DevBuf<SnItem> desc;  // [items] per sweep item its node's record (SnView::desc)
  int citems_n = 0;
  bool compact = false;
  double sweep_bytes_fwd = 0.0, sweep_bytes_bwd = 0.0;
  // DPGO_PANEL_GUARD (debug runs): (offset, doubles) of the NaN gap after every supernode's panel and after the last
  std::vector<std::pair<long, long>> guards;
  double flops = 0.0;      // the factorisation's classic flop count: sum over supernodes s^3/3 + s^2 t + s t^2
  double inv_flops = 0.0;  // the panels' extra: L_SS^-1 (s^3/3) and L_RS L_SS^-1 (s^2 t) per supernode
  // device numeric factorisation (TUNE_DEVICE_CHOL, edge-stream Q): the symbolic structure is built once per Q
  // pattern (sym_ready); every refresh after a reweighting re-runs only k_sn_factor, level by level
  bool sym_ready = false;
  std::vector<int> level_off;  // [depth + 1] into fac_nodes
  DevBuf<int> fac_nodes, ch_off, ch, tp_off, tp, ent_off, src;
  // [K] per agent: 1 = its factorisation met a non-positive pivot (identity preconditioner for that agent only,
  // src/QuadraticProblem.cpp:81-86); written by the device factor, or uploaded by the host factorisation
  DevBuf<int> not_pd;
  DevBuf<long> fac_off;
  DevBuf<SnEntry> ent;
  DevBuf<double> fac_F[2];  // frontal matrices of the even / odd tree depths
  // tree levels factorised tile-parallel (few, large supernodes): per depth the launch sequence of
  // launch_sn_factor_tiled over titems (empty: one workgroup per node, k_sn_factor)
  std::vector<std::vector<FacLaunch>> fac_seq;
  DevBuf<int2> titems;
  double factor_ms = 0.0;       // the last device factorisation (hipEvent), for the benches
  bool factor_pending = false;  // fac_ev holds a factorisation whose time is not yet in factor_ms
  int factor_count = 0;
  EventPair fac_ev;  // the device factorisation's timing (created once per handle)
  // What the factor is of: Q + 0.1 I from the handle's diagonal blocks (the preconditioner), or, for the
  // certificate's state (dpgo_hip_problem_s::cert), S(X) + shift I from the diagonal blocks in cert_diag.
  // force_device: the numeric factorisation runs on the device whatever TUNE_DEVICE_CHOL says.
  double shift = 0.1;
  DevBuf<double> cert_diag;
  bool use_cert_diag = false, force_device = false;
};

}  // namespace dpgo

struct dpgo_hip_problem_s {
  int K = 0, d = 0, r = 0, b = 0;
  int tuning[dpgo::TUNE_COUNT] = {};  // this handle's tuning keys (the process defaults at creation)
  long N = 0;  // total poses
  std::vector<int> n_agent;
  std::vector<long> pose_off;
  hipStream_t stream = nullptr;
  hipStream_t own_stream = nullptr;

  // tiles
  std::vector<int> h_tile_agent, h_tile_start, h_tile_count, h_agent_tile_off;
  int num_tiles = 0;
  dpgo::DevBuf<int> tile_agent, tile_start, tile_count, agent_tile_off, agent_np, enabled, use_a;

  // Q (per-agent host copies, concatenated on upload)
  std::vector<dpgo::HostBSR> q_agent;
  std::vector<dpgo::HostEdges> e_agent;
  std::vector<int> q_fmt;  // per agent: QFMT_BSR / QFMT_EDGES
  int fmt = 0;             // format of the uploaded Q (all agents agree)
  bool q_dirty = true;
  dpgo::DevBuf<int> rowptr, col;
  dpgo::DevBuf<double> blocks, minv;
  long nnzb = 0;
  dpgo::DevBuf<int> inc_ptr, rec_first;
  dpgo::DevBuf<int2> inc;
  // second-visit staging: per tile the sorted ids of its second-visit edges (sv_ptr / sv_ids) and the
  // incidences with tile-local record slots (inc_sv: second visits 0.., first visits after them)
  dpgo::DevBuf<int> sv_ptr, sv_ids;
  dpgo::DevBuf<int2> inc_sv;
  dpgo::DevBuf<double> rec, diag;
  long nnz_inc = 0, num_edges = 0;
  // on-device reweighting (dpgo_hip_set_edge_weights_dev): unweighted measurement per record slot
  // [R | t | kappa | tau], problem edge -> slot, and per pose every incident edge incl. shared ones
  // (slot * 2 + (pose == p1)) in edge order, for the diagonal blocks
  dpgo::DevBuf<double> raw, wslot;
  dpgo::DevBuf<int> slot_of_edge, dinc_ptr, dinc;
  bool host_weights_stale = false;
  const double* w_dev_last = nullptr;  // caller's weight array of the last device reweighting

  // G (sparse pose blocks per agent)
  std::vector<std::map<int, std::vector<double>>> g_agent;
  bool g_dirty = true;
  dpgo::DevBuf<int> gidx;
  dpgo::DevBuf<double> gblk;
  int num_gslots = 0;

  int precon = DPGO_PRECON_BLOCK_JACOBI;

  dpgo::ExactPrecond ex;  // exact preconditioner: supernodal Cholesky of Q + 0.1 I
  // the Cholesky certificate's factor of S(X) + sigma I (dpgo_hip_certify_chol*): exchanged with `ex` around its
  // calls, so the preconditioner's factor, flags and counters never see it
  dpgo::ExactPrecond cert;
  dpgo::DevBuf<int4> tile_meta;  // edge-stream Q: per tile stage ranges (LaunchCtx::tile_meta); empty otherwise
  // edge-stream records and diagonal blocks at unit weights (kept by the engine under a robust cost): the central
  // evaluation of examples/MultiRobotExample.cpp:229-235 reads the dataset's Q, not the reweighted one
  dpgo::DevBuf<double> rec_unit, diag_unit;
  bool central_unit = false;  // qview() serves rec_unit / diag_unit
  // host copy of the edge-stream incidences (sync_q_edges), for the factor's assembly tables
  std::vector<int> h_inc_ptr;
  std::vector<dpgo::SnPair> h_inc;

  // work
  dpgo::DevBuf<double> x1, x2, g, g2, S, S2, eta, rv, z, delta, Hdelta, tA, tB;
  dpgo::DevBuf<double> pa, pb, sums, coef_a, coef_b;
  // |X_out - X_in|^2 partials of the single-Run output select: each tile written once, in the Run
  // its agent's outcome was decided (an in-place X_in is overwritten by then)
  dpgo::DevBuf<double> pc;
  dpgo::DevBuf<double> peh;  // merged tCG: k_tcg_updir's <eta_old, Hdelta> partials (FinalizeArgs::pc)
  // TUNE_SPLIT_STREAMS: agent groups 1.. of the merged tCG iterations run on split_stream[g - 1], forked
  // from / joined into the launch stream by events
  static constexpr int kMaxSplit = 8;
  hipStream_t split_stream[kMaxSplit - 1] = {};
  hipEvent_t split_fork = nullptr, split_join[kMaxSplit - 1] = {};
  // TUNE_TCG_BLOCK: agent blocks the last optimise call queued its merged tCG loop in (0: the unblocked queueing);
  // the blocks' streams and events are the split's
  int tcg_blocks_last = 0;
  dpgo::DevBuf<dpgo::AgentState> state;
  std::vector<dpgo::AgentState> h_state;
  // per-agent arrival counts of a k_spmm with a fused finalize (0 between launches)
  dpgo::DevBuf<int> arrive;
  // finalize after an SpMM: 0 separate k_finalize launch, 1 / 2 fused into the SpMM's last block per
  // agent (SpmmArgs::fin_mode); DPGO_FUSE_FINALIZE overrides
  int fuse_finalize = 0;
  // serpentine tile order (TUNE_TILE_ORDER >= 2): the handle's next pose-tiled launch walks its tiles in reverse
  // (tile_order_next flips it at every such launch)
  bool tile_reverse = false;
  // host-mapped status words written by k_finalize (zero-copy polling, no stream sync)
  int* pub_host = nullptr;
  int* pub_dev = nullptr;
  int pub_tag = 0;
  // the first tCG step of the previous optimize call stopped every agent on the trust-region
  // boundary (or negative curvature): the next call's first step evaluates only <delta, Hess delta>
  // (MODE_QF) and forms Hess[delta] only for agents that turn out to take a CG step
  bool predict_boundary = true;
  std::vector<double> h_sums;
  // per-iteration trace (dpgo_hip_set_trace): [K][trace_cap][kTraceWidth] doubles
  dpgo::DevBuf<double> trace;
  int trace_cap = 0;
  // in-step SpMM timing (dpgo_rbcd_set_kernel_timing): HIP events around every X.Q launch on the
  // handle's stream, resolved per mode by take_spmm_times()
  int timing = 0;  // 0 off, k > 0: every k-th launch of each mode (a sample: events cost dispatch gaps)
  long long timing_seq[dpgo::kSpmmModes] = {};
  struct TimedLaunch {
    int mode;
    hipEvent_t a, b;
    int tiles;  // the launch's tiles (a launch over part of the batch: an agent group or block of the merged tCG)
  };
  std::vector<TimedLaunch> timed;
  std::vector<hipEvent_t> ev_pool;
  // completed timed launches drained out of `timed` (bounded event count on long timed runs)
  double timed_ms[dpgo::kSpmmModes] = {};
  long long timed_n[dpgo::kSpmmModes] = {};
  // summed TimedLaunch::tiles: over the batch's tile count the full-batch launch equivalents, exact when the timed
  // sub-launches add up to whole batches
  long long timed_tiles[dpgo::kSpmmModes] = {};
  ~dpgo_hip_problem_s() {
    for (auto& t : timed) {
      (void)hipEventDestroy(t.a);
      (void)hipEventDestroy(t.b);
    }
    for (auto e : ev_pool) (void)hipEventDestroy(e);
  }

  size_t vec_len() const { return static_cast<size_t>(N) * r * b; }
  size_t vec_bytes() const { return vec_len() * sizeof(double); }
  size_t s_len() const { return static_cast<size_t>(N) * (b - 1) * b / 2; }  // packed symmetric S per pose
};


namespace dpgo {
// helpers implemented in capi.cpp (the optimiser driver and the block rules: optimize.cpp)
// the launch context of the handle's next pose-tiled launch: its tile order comes from tile_order_next
LaunchCtx make_ctx(dpgo_hip_problem h, int flag_kind, double* partials);
LaunchCtx make_ctx_order(dpgo_hip_problem h, int flag_kind, double* partials, int order);
int tile_order_next(dpgo_hip_problem h);
int problem_ready(dpgo_hip_problem h);
int ensure_work_public(dpgo_hip_problem h);

// PGOAgent status after an update (src/PGOAgent.cpp:700-716): relativeChange of X_out against ref
// (XPrev), readyToTerminate with the converged loop-closure ratio per agent (nullptr = 1).
struct StatusArgs {
  const double* ref;
  const double* conv_ratio;
  double rel_tol, min_ratio;
};
// dpgo_hip_optimize_dev + the status pass (st may be null)  (optimize.cpp)
int optimize_dev_status(dpgo_hip_problem h, const dpgo_opt_params* params, const double* X_in, double* X_out,
                        const int* agent_enabled_host, dpgo_opt_result* results, const StatusArgs* st);
bool merged_split(dpgo_hip_problem h);  // TUNE_SPLIT_STREAMS applies to this batch (optimize.cpp, tcg_plan.h)
void merged_blocks(dpgo_hip_problem h, std::vector<int>* blocks);  // TUNE_TCG_BLOCK's agent blocks (the same)
// f / |grad|^2 / <G, X> per agent at X into the handle's sums (OP_SUM, nq 3): asynchronous
int eval_sums_dev(dpgo_hip_problem h, const double* X);
// the same with the edge-stream Q at unit weights (keep_unit_q: the copy taken before any reweighting)
int eval_sums_unit_dev(dpgo_hip_problem h, const double* X);
int keep_unit_q(dpgo_hip_problem h);
// copy the per-agent sums (4 per agent) to the host (synchronises)
int download_sums_public(dpgo_hip_problem h, std::vector<double>& out);
// X.Q launch with the handle's optional event timing
int spmm_launch(dpgo_hip_problem h, int mode, const LaunchCtx& c, const SpmmArgs& a);
// synchronise and add the elapsed ms / launch counts of the timed launches per SpmmMode (kSpmmModes)
int take_spmm_times(dpgo_hip_problem h, double* ms_per_mode, long long* launches_per_mode, double* batch_equiv);
// fold completed (wait: all) timed launches into the handle's per-mode running totals
int drain_timed(dpgo_hip_problem h, bool wait);
// one agent's Q as block-sparse rows, whichever format it was set in
void agent_bsr(dpgo_hip_problem h, int a, HostBSR& out);

// ---- launch helpers of capi.cpp that the optimiser driver (optimize.cpp) uses too
// the arguments of one k_finalize launch over the whole batch (pub_kind 0: publishes no status word)
FinalizeArgs make_fin(dpgo_hip_problem h, int op, const double* pa, int nqa, const double* pb, int nqb,
                      const OptScalars* opt = nullptr, const int* enabled = nullptr, int pub_kind = 0, int pub_tag = 0,
                      int agent_filter = 0);
// make_fin + the launch on the handle's stream
int finalize(dpgo_hip_problem h, int op, const double* pa, int nqa, const double* pb, int nqb,
             const OptScalars* opt = nullptr, const int* enabled = nullptr, int pub_kind = 0, int pub_tag = 0,
             int agent_filter = 0);
// An SpMM followed by finalize `fin`: fused into the SpMM's last block per agent (spmm_arrive), or as
// a separate k_finalize launch when fusion is off.
int spmm_then_finalize(dpgo_hip_problem h, int mode, const LaunchCtx& c, SpmmArgs a, const FinalizeArgs& fin);
// EVAL sweep at X: g = P_X(XQ+G), S, per-agent f and |g|^2 partials into pa.  mode MODE_F: f only;
// MODE_EVAL_TCG: also the tCG start delta = -Prec(g) and the <z, g> partial.  fin: the finalize that follows it.
int eval_at(dpgo_hip_problem h, const double* X, double* gout, double* Sout, double* part, int flag,
            int mode = MODE_EVAL, double* delta = nullptr, int pmode = PRECON_NONE, const FinalizeArgs* fin = nullptr);
// the next status tag of the handle (tags only grow: wait_published compares them with <)
int next_tag(dpgo_hip_problem h);
// spin on the host-mapped status words until every agent published `tag` or a later one; *any: some agent's flag is set
int wait_published(dpgo_hip_problem h, int tag, bool* any, bool* any_cg = nullptr, bool* any_never = nullptr);
// copy the agents' state / the per-agent sums into h_state / h_sums (synchronises)
int download_state(dpgo_hip_problem h);
int download_sums(dpgo_hip_problem h);

// Events created for one scope and destroyed on every exit from it (an early HIP_TRY return included)
struct ScopedEvents {
  std::vector<hipEvent_t> ev;
  explicit ScopedEvents(size_t n) : ev(n, nullptr) {}
  ~ScopedEvents() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  hipError_t create() {
    for (auto& e : ev)
      if (!e) {
        const hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
      }
    return hipSuccess;
  }
};
// launches of a standalone kernel benchmark that run before its timed window
constexpr int kBenchWarmup = 3;

// certify.cpp: out[j] = <x, B_j>, j < k, over vectors of L doubles (B_j at B + j L) by launch_dot_multi into `part`
// (kDotBlocks k doubles on the device), its partials summed on the host in a fixed order (synchronises)
int dot_multi_host(long L, const double* x, const double* B, int k, double* part, hipStream_t stream, double* out);
// certify.cpp: the fields of dpgo_cert_info and its lower bound from a certificate's quantities (ritz: theta's first 8)
void fill_cert_info(dpgo_cert_info* info, int iters, int restarts, int nl, double res, double lam_s, double theta_c,
                    double res_c, double coupling, const std::vector<double>& theta);

// exact.cpp: the exact preconditioner.  sync_chol brings the factor up to date with Q (symbolic build + upload on a
// new pattern, the numeric factorisation alone after a reweighting); exact_precond applies it:
// z = P_X(in (Q + 0.1 I)^-1) per agent, then projection + partials <z, rref>, |rref|^2 (pass rref = in).
int sync_chol(dpgo_hip_problem h);
int exact_precond(dpgo_hip_problem h, const double* in, double* z_out, double* delta_out, const double* X,
                  const double* rref, double* partials, int flag);
}  // namespace dpgo

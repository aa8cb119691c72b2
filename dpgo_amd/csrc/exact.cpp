// Exact preconditioner, device side: the reference factorises P = Q + 0.1 I with CHOLMOD in
// setQ (src/QuadraticProblem.cpp:37-41).  Here the factor is built the first time the EXACT mode is used after a
// setQ, per agent (agents are independent blocks, handled in parallel host threads), as nested-dissection
// supernodes (chol.cpp).  The index tables of the sweeps and of the device factorisation come from the pure host
// builder (sn_schedule.cpp); this unit reads the options, uploads the tables and panels, and issues the launches:
// one work list per tree level shared by the batch (level l of every agent runs in one launch per sweep).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <stdexcept>
#include <thread>
#include <type_traits>

#include "cert_host.h"
#include "problem_internal.h"

namespace dpgo {

static_assert(sizeof(SnPair) == sizeof(int2) && alignof(SnPair) == alignof(int) && offsetof(SnPair, y) == offsetof(int2, y),
              "the schedule's item pairs are uploaded as the kernels' int2");

namespace {

constexpr long kMaxCholDoubles = 3L << 30;  // 24 GiB of panels per handle

bool env_on(const char* name) {  // a default-on switch: off only as NAME=0
  const char* e = std::getenv(name);
  return !(e && e[0] == '0');
}

// The builder's options: the one place the exact path reads its levers, at every symbolic rebuild (tests set them
// per case).  DPGO_SN_FWD_SMALL=0: every forward item through k_sn_fwd; DPGO_SN_COMPACT=0: no compact copy of the
// narrow nodes; DPGO_FAC_TILED_MAX_NODES / _MIN_TILES restrict the tile-parallel levels (tests: small graphs);
// DPGO_PANEL_GUARD=1 (debug runs, read once per process): NaN gaps after every panel, checked by exact_precond
SnScheduleOptions schedule_options(bool device) {
  static const bool guard = std::getenv("DPGO_PANEL_GUARD") != nullptr;
  SnScheduleOptions o;
  o.fwd_small = env_on("DPGO_SN_FWD_SMALL");
  o.compact = env_on("DPGO_SN_COMPACT");
  o.guard = guard;
  if (const char* e = std::getenv("DPGO_FAC_TILED_MAX_NODES")) o.tiled_max_nodes = std::atoi(e);
  if (const char* e = std::getenv("DPGO_FAC_TILED_MIN_TILES")) o.tiled_min_tiles = std::atoi(e);
  o.device = device;
  return o;
}

bool verbose_chol() { return std::getenv("DPGO_VERBOSE_CHOL") != nullptr; }

// host threads for the per-agent factorisations: DPGO_CHOL_THREADS, else OMP_NUM_THREADS (the GPU box
// sets it to the per-GPU host share), else the hardware count, at most 16
int chol_threads(int K) {
  int t = 0;
  for (const char* var : {"DPGO_CHOL_THREADS", "OMP_NUM_THREADS"})
    if (const char* s = std::getenv(var)) {
      t = std::atoi(s);
      if (t > 0) break;
    }
  if (t <= 0) t = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  return std::max(1, std::min(t, K));
}

// The last device factorisation's time (fac_ev pair): resolved when it is asked for, so a refactorisation inside
// the solve loop never waits for the GPU
int resolve_factor_ms(dpgo_hip_problem h) {
  auto& ex = h->ex;
  if (!ex.factor_pending) return DPGO_HIP_OK;
  HIP_TRY(hipEventSynchronize(ex.fac_ev[1]));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, ex.fac_ev[0], ex.fac_ev[1]));
  ex.factor_ms = ms;
  ex.factor_pending = false;
  return DPGO_HIP_OK;
}

// The narrow supernodes' compact panels from the freshly factorised tiles (stream-ordered after the factor)
int compact_panels(dpgo_hip_problem h) {
  auto& ex = h->ex;
  if (!ex.compact || ex.citems_n == 0) return DPGO_HIP_OK;
  HIP_TRY(launch_sn_compact(h->b, ex.panel.p, ex.panel_off.p, ex.s.p, ex.t.p, ex.cpanel_off.p, ex.cpanel.p, ex.citems.p,
                            ex.citems_n, h->stream));
  return DPGO_HIP_OK;
}

// The device numeric factorisation: k_sn_factor level by level (deepest first) over the symbolic structure and
// the current edge-stream Q.  A non-positive pivot marks its agent in not_pd ([K], reset here); that agent's
// sweeps are skipped and its preconditioner output is its input, unprojected -- the reference's fallback per
// QuadraticProblem (src/QuadraticProblem.cpp:81-86), so the other agents of the batch keep their factors.  Nothing
// here waits for the GPU: the flags are read on the device by the sweeps, and by the host only when asked
// (dpgo_hip_exact_fallback_agents).
int device_factor(dpgo_hip_problem h) {
  auto& ex = h->ex;
  const int maxd = static_cast<int>(ex.level_off.size()) - 2;
  HIP_TRY(hipMemsetAsync(ex.not_pd.p, 0, sizeof(int) * h->K, h->stream));
  if (poison_enabled()) {  // debug: the frontal matrices and panels as nothing-written NaN before each factor
    for (auto& F : ex.fac_F) HIP_TRY(poison_fill(F.p, sizeof(double) * F.n, h->stream));
    HIP_TRY(poison_fill(ex.panel.p, sizeof(double) * ex.panel_doubles, h->stream));
  }
  for (auto& ev : ex.fac_ev)
    if (!ev) HIP_TRY(hipEventCreate(&ev));  // owned by the handle: no leak on an early error return
  hipEvent_t e0 = ex.fac_ev[0], e1 = ex.fac_ev[1];
  HIP_TRY(hipEventRecord(e0, h->stream));
  const bool verbose = verbose_chol();
  ScopedEvents lev(verbose ? maxd + 2 : 0);
  HIP_TRY(lev.create());
  // the matrix: Q + 0.1 I (the preconditioner), or S(X) + shift I through the certificate's diagonal blocks
  const double* diag = ex.use_cert_diag ? ex.cert_diag.p : h->diag.p;
  for (int dep = maxd; dep >= 0; --dep) {
    const int n0 = ex.level_off[dep], n1 = ex.level_off[dep + 1];
    SnFactorView v{ex.fac_nodes.p + n0, ex.s.p, ex.t.p, ex.fac_off.p, ex.panel_off.p, ex.poses_off.p, ex.poses.p,
                   ex.ch_off.p, ex.ch.p, ex.tp_off.p, ex.tp.p, ex.ent_off.p, ex.ent.p, ex.src.p, h->rec.p, diag, ex.shift,
                   ex.fac_F[dep & 1].p, ex.fac_F[(dep + 1) & 1].p, ex.panel.p, ex.node_agent.p, ex.not_pd.p};
    if (verbose) HIP_TRY(hipEventRecord(lev.ev[dep + 1], h->stream));
    if (dep < static_cast<int>(ex.fac_seq.size()) && !ex.fac_seq[dep].empty()) {
      for (const auto& fl : ex.fac_seq[dep])
        HIP_TRY(launch_sn_factor_tiled(h->b, v, fl.kind, fl.param, ex.titems.p + fl.off, fl.count, h->stream));
    } else {
      HIP_TRY(launch_sn_factor(h->b, v, n1 - n0, h->stream));
    }
  }
  if (verbose) HIP_TRY(hipEventRecord(lev.ev[0], h->stream));
  HIP_TRY(hipEventRecord(e1, h->stream));
  DPGO_TRY(compact_panels(h));  // after the factor's timing window: part of the sweeps' data, not the factorisation
  ex.factor_count += 1;
  ex.factor_pending = true;
  ex.state = 1;
  if (verbose) {
    DPGO_TRY(resolve_factor_ms(h));
    std::fprintf(stderr, "[dpgo_hip] exact preconditioner: device factorisation %.2f ms; per level (depth: nodes ms):",
                 ex.factor_ms);
    for (int dep = maxd; dep >= 0; --dep) {
      float lm = 0.f;
      HIP_TRY(hipEventElapsedTime(&lm, lev.ev[dep + 1], lev.ev[dep]));
      std::fprintf(stderr, " %d:%d %.1f", dep, ex.level_off[dep + 1] - ex.level_off[dep], static_cast<double>(lm));
    }
    std::fprintf(stderr, "\n");
  }
  return DPGO_HIP_OK;
}

// step 1: weights changed on the device -- bring the host measurement copy up to date
int refresh_host_weights(dpgo_hip_problem h) {
  if (!h->host_weights_stale) return DPGO_HIP_OK;
  std::vector<double> w(std::max<long>(h->num_edges, 1));
  HIP_TRY(hipMemcpyAsync(w.data(), h->w_dev_last, sizeof(double) * h->num_edges, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  long eg = 0;
  for (int a = 0; a < h->K; ++a) {
    HostEdges& E = h->e_agent[a];
    for (size_t e = 0; e < E.p1.size(); ++e, ++eg) {
      E.kw[e] = w[eg] * E.kappa0[e];
      E.tw[e] = w[eg] * E.tau0[e];
    }
  }
  h->host_weights_stale = false;
  return DPGO_HIP_OK;
}

// step 2: per-agent factor structure (device: symbolic only; host: the whole factorisation), host threads.
// host_ident: host factorisation, agents whose Q + 0.1 I met a non-positive pivot
int factor_agents(dpgo_hip_problem h, bool device, std::vector<SupernodalFactor>& Fs, std::vector<int>& host_ident) {
  const int b = h->b, K = h->K;
  Fs.assign(K, {});
  host_ident.assign(K, 0);
  std::vector<std::string> errs(K);
  std::vector<int> rcs(K, 0);
  {
    std::atomic<int> next{0}, done{0};
    const auto t0 = std::chrono::steady_clock::now();
    std::mutex log_mu;
    auto work = [&]() {
      for (int a = next++; a < K; a = next++) {
        try {
          HostBSR Q;
          agent_bsr(h, a, Q);
          rcs[a] = device ? supernodal_symbolic(h->n_agent[a], b, Q.rowptr, Q.col, kMaxCholDoubles, Fs[a], errs[a])
                          : supernodal_cholesky(h->n_agent[a], b, Q.rowptr, Q.col, Q.blocks, 0.1, kMaxCholDoubles, Fs[a],
                                                errs[a]);
        } catch (const std::bad_alloc&) {
          rcs[a] = -2;
          errs[a] = "exact preconditioner: out of host memory in the factorisation";
        } catch (const std::exception& ex) {
          rcs[a] = -1;
          errs[a] = std::string("exact preconditioner: ") + ex.what();
        }
        // a long factorisation reports progress (a silent process looks hung to a supervisor)
        const int k = ++done;
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (sec > 5.0) {
          std::lock_guard<std::mutex> lk(log_mu);
          std::fprintf(stderr, "[dpgo_hip] exact preconditioner: %d / %d agents factorised (%.1f s)\n", k, K, sec);
        }
      }
    };
    const int nt = chol_threads(K);
    std::vector<std::thread> pool;
    for (int i = 1; i < nt; ++i) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
  }
  long total = 0;
  for (int a = 0; a < K; ++a) {
    if (rcs[a] != 0) {
      if (errs[a].find("positive definite") == std::string::npos)
        return fail(rcs[a] == -2 ? DPGO_HIP_ENOMEM : DPGO_HIP_EINVAL, errs[a]);
      // src/QuadraticProblem.cpp:81-86, per QuadraticProblem: this agent's solves fail -> "Preconditioner failed",
      // out = in; the batch's other agents keep their factors.  The agent keeps its symbolic structure (its
      // supernodes are skipped by the sweeps, so its panels are never read).
      std::printf("[dpgo_hip] Preconditioner failed (agent %d: %s); using the identity for it.\n", a, errs[a].c_str());
      host_ident[a] = 1;
      HostBSR Q;
      agent_bsr(h, a, Q);
      std::string e2;
      Fs[a] = SupernodalFactor();
      if (supernodal_symbolic(h->n_agent[a], b, Q.rowptr, Q.col, kMaxCholDoubles, Fs[a], e2) != 0)
        return fail(DPGO_HIP_EINVAL, e2);
    }
    total += Fs[a].panel_doubles;
  }
  if (total > kMaxCholDoubles)
    return fail(DPGO_HIP_EINVAL, "exact preconditioner: the supernodal panels of the batch would exceed 24 GiB "
                                 "(use DPGO_PRECON_BLOCK_JACOBI for this size)");
  if (verbose_chol())
    std::fprintf(stderr, "[dpgo_hip] exact preconditioner: %d agents, %.3f GiB of supernodal panels\n", K,
                 8.0 * static_cast<double>(total) / (1024.0 * 1024.0 * 1024.0));
  return DPGO_HIP_OK;
}

// The host factor's panels go up through a pinned staging buffer, one agent at a time: one DMA per node from
// pinned memory instead of the runtime's pageable-copy path.  Each agent's host panels are released once copied.
int upload_host_panels(dpgo_hip_problem h, const SnSchedule& S, std::vector<SupernodalFactor>& Fs) {
  size_t stage_n = 0;
  for (const auto& F : Fs) {
    size_t na = 0;
    for (const auto& nd : F.nodes) na += nd.panel.size();
    stage_n = std::max(stage_n, na);
  }
  double* stage = nullptr;
  if (stage_n > 0 && hipHostMalloc(reinterpret_cast<void**>(&stage), sizeof(double) * stage_n) != hipSuccess)
    return fail(DPGO_HIP_ENOMEM, "pinned staging buffer for the panels");
  struct StageFree {
    double* p;
    ~StageFree() {
      if (p) (void)hipHostFree(p);
    }
  } stage_free{stage};
  int g = 0;
  for (auto& F : Fs) {
    size_t so = 0;
    for (auto& nd : F.nodes) {
      const auto& P = nd.panel;
      const long dst = S.panel_off[g++];
      if (P.empty()) continue;
      std::memcpy(stage + so, P.data(), sizeof(double) * P.size());
      HIP_TRY(hipMemcpyAsync(h->ex.panel.p + dst, stage + so, sizeof(double) * P.size(), hipMemcpyHostToDevice,
                             h->stream));
      so += P.size();
    }
    HIP_TRY(hipStreamSynchronize(h->stream));  // then release the agent's host panels (and reuse the stage)
    for (auto& nd : F.nodes) std::vector<double>().swap(nd.panel);
  }
  return DPGO_HIP_OK;
}

// step 4: the schedule's tables (and, host factorisation, the panels) to the device.  Every upload is ordered on
// h->stream (the handle's stream is non-blocking: a copy on the null stream is not ordered before the sweeps and
// factor kernels queued after it) and asynchronous: S must outlive the caller's stream synchronisation.
int upload_schedule(dpgo_hip_problem h, const SnSchedule& S, const SnScheduleOptions& opt,
                    std::vector<SupernodalFactor>& Fs, const std::vector<int>& host_ident) {
  auto& ex = h->ex;
  const bool device = opt.device, guard = opt.guard;
  auto up = [&](auto& d, const auto& v) -> int {
    using T = typename std::decay_t<decltype(v)>::value_type;
    static_assert(sizeof(T) == sizeof(*d.p), "host and device element of one size");
    HIP_TRY(d.ensure(std::max<size_t>(v.size(), 1)));
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(d.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, h->stream));
    return DPGO_HIP_OK;
  };
  HIP_TRY(hipStreamSynchronize(h->stream));
  // DPGO_PANEL_GUARD: besides the gap after every panel, 1 Mi doubles after the last; the whole buffer NaN (all-ones
  // bytes) first: the panels are written over it, the gaps keep it
  constexpr long kGuard = 1L << 20;
  const long po = S.po;
  HIP_TRY(ex.panel.ensure(std::max<long>(po, 1) + (guard ? kGuard : 0)));
  ex.guards = S.guards;
  if (guard) {
    HIP_TRY(hipMemsetAsync(ex.panel.p, 0xFF, sizeof(double) * (std::max<long>(po, 1) + kGuard), h->stream));
    ex.guards.emplace_back(std::max<long>(po, 1), kGuard);
  }
  if (device && poison_enabled()) HIP_TRY(poison_fill(ex.panel.p, sizeof(double) * po, h->stream));
  if (!device) DPGO_TRY(upload_host_panels(h, S, Fs));
  DPGO_TRY(up(ex.panel_off, S.panel_off));
  DPGO_TRY(up(ex.f_off, S.f_off));
  DPGO_TRY(up(ex.u_off, S.u_off));
  DPGO_TRY(up(ex.s, S.s));
  DPGO_TRY(up(ex.t, S.t));
  DPGO_TRY(up(ex.poses_off, S.poses_off));
  DPGO_TRY(up(ex.poses, S.poses));
  DPGO_TRY(up(ex.cpos_off, S.cpos_off));
  DPGO_TRY(up(ex.cpos, S.cpos));
  DPGO_TRY(up(ex.contrib, S.contrib));
  DPGO_TRY(up(ex.items, S.items));
  DPGO_TRY(up(ex.node_agent, S.node_agent));
  if (!device) DPGO_TRY(up(ex.not_pd, host_ident));
  ex.levels = S.levels;
  ex.compact = opt.compact;
  ex.sweep_bytes_fwd = S.sweep_bytes_fwd;
  ex.sweep_bytes_bwd = S.sweep_bytes_bwd;
  ex.citems_n = static_cast<int>(S.citems.size());
  DPGO_TRY(up(ex.cpanel_off, S.coff));
  DPGO_TRY(up(ex.citems, S.citems));
  HIP_TRY(ex.cpanel.ensure(std::max<long>(S.co, 1)));
  DPGO_TRY(up(ex.desc, S.desc));
  HIP_TRY(ex.F.ensure(std::max<long>(S.fo, 1)));
  HIP_TRY(ex.U.ensure(std::max<long>(S.uo, 1)));
  ex.panel_doubles = po;
  ex.nodes = S.nodes;
  ex.flops = S.flops;
  ex.inv_flops = S.inv_flops;
  if (!device) return compact_panels(h);
  DPGO_TRY(up(ex.titems, S.titems));
  if (verbose_chol()) {
    std::fprintf(stderr, "[dpgo_hip] exact preconditioner: device factorisation, %d levels, frontal buffers %.3f + %.3f GiB\n",
                 S.max_depth + 1, 8.0 * S.level_size[0] / (1 << 30), 8.0 * S.level_size[1] / (1 << 30));
    std::fprintf(stderr, "[dpgo_hip] exact preconditioner: tile-parallel levels:");
    for (int dep = 0; dep <= S.max_depth; ++dep)
      if (!S.fac_seq[dep].empty()) std::fprintf(stderr, " %d (%zu launches)", dep, S.fac_seq[dep].size());
    std::fprintf(stderr, ", %zu items\n", S.titems.size());
  }
  ex.level_off = S.level_off;
  ex.fac_seq = S.fac_seq;
  DPGO_TRY(up(ex.fac_nodes, S.fac_nodes));
  DPGO_TRY(up(ex.fac_off, S.fac_off));
  DPGO_TRY(up(ex.ch_off, S.ch_off));
  DPGO_TRY(up(ex.ch, S.ch));
  DPGO_TRY(up(ex.tp_off, S.tp_off));
  DPGO_TRY(up(ex.tp, S.tp));
  DPGO_TRY(up(ex.ent_off, S.ent_off));
  DPGO_TRY(up(ex.ent, S.ent));
  DPGO_TRY(up(ex.src, S.src));
  HIP_TRY(ex.not_pd.ensure(h->K));
  for (int q = 0; q < 2; ++q) HIP_TRY(ex.fac_F[q].ensure(std::max<long>(S.level_size[q], 1)));
  return DPGO_HIP_OK;
}

// The sweeps' view of the handle's factor; `flag` is the per-agent skip of the launch that consumes the sweep
SnView sn_view(dpgo_hip_problem h, int flag) {
  auto& ex = h->ex;
  SnView v{ex.panel.p,   ex.panel_off.p, ex.s.p, ex.t.p, ex.poses_off.p,  ex.poses.p, ex.f_off.p,
           ex.u_off.p,   ex.cpos_off.p,  ex.cpos.p, ex.contrib.p, ex.F.p, ex.U.p,     ex.node_agent.p,
           h->state.p,   flag,           ex.not_pd.p, ex.cpanel.p, ex.compact ? ex.cpanel_off.p : nullptr};
  v.desc = ex.desc.p;
  v.items_base = ex.items.p;
  return v;
}

// the forward sweep up the supernodal trees (in -> tA), one launch per level and kernel
int sweep_forward(dpgo_hip_problem h, const SnView& v, const double* in) {
  const int2* it = h->ex.items.p;
  for (int l = static_cast<int>(h->ex.levels.size()) - 1; l >= 0; --l) {
    const SnLevel& L = h->ex.levels[l];
    HIP_TRY(launch_sn_assemble(h->r, h->b, v, it + L.asm0, L.asm_n, in, h->stream));
    HIP_TRY(launch_sn_fwd_small(h->r, h->b, v, it + L.fws0, L.fws_n, h->tA.p, h->stream));
    HIP_TRY(launch_sn_fwd(h->r, h->b, v, it + L.fwd0, L.fwd_n, h->tA.p, h->stream));
  }
  return DPGO_HIP_OK;
}

// the backward sweep down the trees (tA -> tB)
int sweep_backward(dpgo_hip_problem h, const SnView& v) {
  const int2* it = h->ex.items.p;
  for (const SnLevel& L : h->ex.levels)
    HIP_TRY(launch_sn_bwd(h->r, h->b, v, it + L.bwd0, L.bwd_n, h->tA.p, h->tB.p, h->stream));
  return DPGO_HIP_OK;
}

// DPGO_PANEL_GUARD: every gap between the panels, and the one after them, untouched?
int check_guards(dpgo_hip_problem h) {
  const auto& ex = h->ex;
  HIP_TRY(hipStreamSynchronize(h->stream));
  long bad = 0, total = 0, first = -1;
  std::vector<unsigned long long> gbuf;
  for (const auto& gr : ex.guards) {
    gbuf.resize(gr.second);
    HIP_TRY(hipMemcpy(gbuf.data(), ex.panel.p + gr.first, sizeof(double) * gr.second, hipMemcpyDeviceToHost));
    for (long i = 0; i < gr.second; ++i)
      if (gbuf[i] != ~0ULL) {
        ++bad;
        if (first < 0) first = gr.first + i;
      }
    total += gr.second;
  }
  std::fprintf(stderr, "[dpgo_hip] panel guard: %ld of %ld guard doubles in %zu gaps changed (first at %ld)\n", bad, total,
               ex.guards.size(), first);
  return DPGO_HIP_OK;
}

}  // namespace

int sync_chol(dpgo_hip_problem h) {
  auto& ex = h->ex;
  if (ex.state != 0) return DPGO_HIP_OK;
  bool edges = true;
  for (int a = 0; a < h->K; ++a) edges = edges && h->q_fmt[a] == QFMT_EDGES;
  const bool device = edges && (h->tuning[TUNE_DEVICE_CHOL] > 0 || ex.force_device);
  if (device && ex.sym_ready) return device_factor(h);  // same pattern: only the numeric half again, never waits
  if (!device) DPGO_TRY(refresh_host_weights(h));
  std::vector<SupernodalFactor> Fs;
  std::vector<int> host_ident;
  DPGO_TRY(factor_agents(h, device, Fs, host_ident));
  const SnScheduleOptions opt = schedule_options(device);
  const SnSchedule S = build_sn_schedule(Fs, h->pose_off, h->n_agent, h->b, h->r, h->h_inc_ptr, h->h_inc, opt);
  const int rc = upload_schedule(h, S, opt, Fs, host_ident);
  // the uploaded host tables die with this frame: an asynchronous copy from pageable memory need not have read its
  // source when the call returns.  Only after a symbolic rebuild; refactorisations (sym_ready) never wait.
  const hipError_t synced = hipStreamSynchronize(h->stream);
  DPGO_TRY(rc);
  HIP_TRY(synced);
  if (!device) {
    ex.state = 1;
    return DPGO_HIP_OK;
  }
  ex.sym_ready = true;
  return device_factor(h);
}

// With a failed factorisation z = in, unprojected, as the reference.  Agents that `flag` skips (k_precond_finish
// leaves their z untouched) are skipped by the sweeps too: a tCG iteration streams only the panels of the agents
// still in tCG.
int exact_precond(dpgo_hip_problem h, const double* in, double* z_out, double* delta_out, const double* X,
                  const double* rref, double* partials, int flag) {
  DPGO_TRY(sync_chol(h));
  auto& ex = h->ex;
  const double* zraw = in;
  if (ex.state == 1) {
    const SnView v = sn_view(h, flag);
    if (poison_enabled())  // debug: frontal / update / sweep vectors as nothing-written NaN
      for (auto* B : {&ex.F, &ex.U, &h->tA, &h->tB}) HIP_TRY(poison_fill(B->p, sizeof(double) * B->n, h->stream));
    DPGO_TRY(sweep_forward(h, v, in));
    DPGO_TRY(sweep_backward(h, v));
    zraw = h->tB.p;
    if (!ex.guards.empty()) DPGO_TRY(check_guards(h));
  }
  auto c = make_ctx(h, flag, partials);
  HIP_TRY(launch_precond_finish(h->r, h->b, c, X, zraw, in, ex.state == 1 ? ex.not_pd.p : nullptr, rref,
                                ex.state == 1 ? 1 : 0, z_out, delta_out));
  return DPGO_HIP_OK;
}

// ---- certification by factorisation: S(X) + sigma I through the factor kernels above
namespace {

// The certificate's factor state stands in h->ex for one scope, so sync_chol, device_factor and the sweeps run on it
// unchanged; on every exit the preconditioner's state is back where it was
struct CertScope {
  dpgo_hip_problem h;
  explicit CertScope(dpgo_hip_problem hh) : h(hh) {
    std::swap(h->ex, h->cert);
    h->ex.use_cert_diag = h->ex.force_device = true;
  }
  ~CertScope() { std::swap(h->ex, h->cert); }
};

int cert_check(dpgo_hip_problem h, const double* X) {
  DPGO_TRY(check_handle(h));
  if (h->K != 1) return fail(DPGO_HIP_EINVAL, "certification needs a single-agent handle");
  if (!X) return fail(DPGO_HIP_EINVAL, "bad certification arguments");
  DPGO_TRY(problem_ready(h));
  if (h->q_fmt[0] != QFMT_EDGES)
    return fail(DPGO_HIP_EINVAL, "certification by factorisation needs an edge-stream Q (set_Q_edges)");
  return ensure_work_public(h);
}

// X to the device, Lambda(X) into h->S (the S the Riemannian Hessian uses), the certificate's diagonal blocks
int cert_begin(dpgo_hip_problem h, const double* X, DevBuf<double>& xdev) {
  HIP_TRY(xdev.ensure(h->vec_len()));
  HIP_TRY(hipMemcpyAsync(xdev.p, X, h->vec_bytes(), hipMemcpyHostToDevice, h->stream));
  DPGO_TRY(eval_at(h, xdev.p, h->tA.p, h->S.p, h->pa.p, FLAG_NONE));
  HIP_TRY(h->ex.cert_diag.ensure(static_cast<size_t>(h->N) * diag_width(h->d)));
  HIP_TRY(launch_cert_diag(h->b, static_cast<int>(h->N), h->diag.p, h->S.p, h->ex.cert_diag.p, h->stream));
  return DPGO_HIP_OK;
}

// one numeric factorisation of S(X) + sigma I (the symbolic analysis on the first call per pattern); the one wait
int cert_factor(dpgo_hip_problem h, double sigma, int* pd) {
  auto& ex = h->ex;
  ex.shift = sigma;
  ex.state = 0;
  DPGO_TRY(sync_chol(h));
  int bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, ex.not_pd.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *pd = bad == 0;
  return DPGO_HIP_OK;
}

}  // namespace

}  // namespace dpgo

using namespace dpgo;

extern "C" {

void dpgo_default_chol_cert_params(dpgo_chol_cert_params* p) {
  if (!p) return;
  p->ratio = 1.0 + 1.0 / 16.0;
  p->max_factorisations = 24;
  p->tol = 1e-8;
  p->max_iters = 200;
}

int dpgo_hip_certify_chol(dpgo_hip_problem h, const double* X, double sigma, int* pd) {
  DPGO_TRY(check_handle(h));
  if (!pd || !std::isfinite(sigma)) return fail(DPGO_HIP_EINVAL, "bad certification arguments");
  DPGO_TRY(cert_check(h, X));
  CertScope scope(h);
  DevBuf<double> xdev;
  DPGO_TRY(cert_begin(h, X, xdev));
  int ok = 0;
  DPGO_TRY(cert_factor(h, sigma, &ok));
  *pd = ok;
  return DPGO_HIP_OK;
}

int dpgo_hip_certify_chol_ex(dpgo_hip_problem h, const double* X, double eta, const dpgo_chol_cert_params* p,
                             double* lambda_min, double* eigvec, dpgo_chol_cert_info* info) {
  DPGO_TRY(check_handle(h));
  dpgo_chol_cert_params P;
  dpgo_default_chol_cert_params(&P);
  if (p) P = *p;
  if (!lambda_min || !std::isfinite(eta) || !(eta > 0.0) || !(P.ratio > 1.0) || P.max_factorisations < 2 ||
      !(P.tol > 0.0) || P.max_iters < 1)
    return fail(DPGO_HIP_EINVAL, "bad certification arguments");
  DPGO_TRY(cert_check(h, X));
  CertScope scope(h);
  auto& ex = h->ex;
  DevBuf<double> xdev;
  DPGO_TRY(cert_begin(h, X, xdev));
  dpgo_chol_cert_info I{};
  auto finish_info = [&]() -> int {
    DPGO_TRY(resolve_factor_ms(h));
    I.factor_ms = ex.factor_ms;
    I.panel_doubles = ex.panel_doubles;
    if (info) *info = I;
    return DPGO_HIP_OK;
  };
  int pd = 0;
  DPGO_TRY(cert_factor(h, eta, &pd));
  I.factorisations = 1;
  if (pd) {
    I.certified = 1;
    I.sigma_lo = I.sigma_hi = eta;
    DPGO_TRY(finish_info());
    *lambda_min = -eta;
    return DPGO_HIP_OK;
  }
  // the bracket's top: S = Q - Lambda >= -max_j |Lambda_j|_2 I since Q >= 0
  const long SW = (h->b - 1) * h->b / 2, D = h->b - 1;
  std::vector<double> Sh(h->s_len());
  HIP_TRY(hipMemcpyAsync(Sh.data(), h->S.p, sizeof(double) * Sh.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  double fmax = 0.0;
  for (long j = 0; j < h->N; ++j) {
    double acc = 0.0;
    long q = j * SW;
    for (long u = 0; u < D; ++u)
      for (long v = u; v < D; ++v, ++q) acc += (u == v ? 1.0 : 2.0) * Sh[q] * Sh[q];
    fmax = std::max(fmax, acc);
  }
  const double sigma_top = (1.0 + 1e-6) * std::sqrt(fmax) + eta;
  double lo = eta, hi = sigma_top;
  DPGO_TRY(cert_factor(h, hi, &pd));
  I.factorisations += 1;
  if (!pd)
    return fail(DPGO_HIP_EDEVICE, "certification: S(X) + sigma_top I is not positive definite (Q is not positive "
                                  "semidefinite, or the factorisation broke down)");
  bool at_hi = true;  // the factor in place is the one at `hi`
  while (hi / lo > P.ratio && I.factorisations < P.max_factorisations) {
    const double mid = std::sqrt(lo) * std::sqrt(hi);
    if (!(mid > lo && mid < hi)) break;
    DPGO_TRY(cert_factor(h, mid, &pd));
    I.factorisations += 1;
    (pd ? hi : lo) = mid;
    at_hi = pd != 0;
  }
  if (!at_hi) {  // the last trial failed: the factor at sigma_hi again (over any max_factorisations, by one)
    DPGO_TRY(cert_factor(h, hi, &pd));
    I.factorisations += 1;
    if (!pd) return fail(DPGO_HIP_EDEVICE, "certification: the factorisation at sigma_hi did not repeat");
  }
  I.sigma_lo = lo;
  I.sigma_hi = hi;
  // inverse iteration on row 0 of the lifted layout (rows 1.. are zero and stay zero: the solve acts row by row);
  // vy = [v | y = v S] so one launch_dot_multi gives <y, v> and <y, y>
  const long L = static_cast<long>(h->vec_len());
  const int r = h->r;
  DevBuf<double> vy, part, coef;
  HIP_TRY(vy.ensure(2 * static_cast<size_t>(L)));
  HIP_TRY(part.ensure(static_cast<size_t>(kDotBlocks) * 2));
  HIP_TRY(coef.ensure(1));
  double* v = vy.p;
  double* y = vy.p + L;
  {  // seeded start on row 0
    const std::vector<double> q0 = cert_start(CertStart::Row0Dense, L, r);
    HIP_TRY(hipMemcpyAsync(v, q0.data(), sizeof(double) * L, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  const SnView view = sn_view(h, FLAG_NONE);
  double lam = 0.0, res = 0.0;
  int it = 0;
  while (it < P.max_iters) {
    if (poison_enabled())  // debug: frontal / update / sweep vectors as nothing-written NaN
      for (auto* B : {&ex.F, &ex.U, &h->tA, &h->tB}) HIP_TRY(poison_fill(B->p, sizeof(double) * B->n, h->stream));
    DPGO_TRY(sweep_forward(h, view, v));
    DPGO_TRY(sweep_backward(h, view));
    ++it;
    double nn = 0.0;
    DPGO_TRY(dot_multi_host(L, h->tB.p, h->tB.p, 1, part.p, h->stream, &nn));
    if (!(nn > 0.0) || !std::isfinite(nn))
      return fail(DPGO_HIP_EDEVICE, "certification: the inverse iteration broke down");
    HIP_TRY(launch_scale(L, h->tB.p, 1.0 / std::sqrt(nn), v, h->stream));
    const SpmmArgs sa{v, nullptr, nullptr, nullptr, h->S.p, y, nullptr, nullptr, nullptr, PRECON_NONE};
    DPGO_TRY(spmm_launch(h, MODE_CERT, make_ctx(h, FLAG_NONE, nullptr), sa));
    double d2[2];
    DPGO_TRY(dot_multi_host(L, y, vy.p, 2, part.p, h->stream, d2));  // <y, v>, <y, y>
    lam = d2[0];
    // the residual y - lam v itself (|y|^2 - lam^2 cancels where the pair has converged)
    HIP_TRY(hipMemcpyAsync(coef.p, &lam, sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_axpy_multi(L, y, v, 1, coef.p, h->stream));
    double rr = 0.0;
    DPGO_TRY(dot_multi_host(L, y, y, 1, part.p, h->stream, &rr));
    res = std::sqrt(std::max(rr, 0.0));
    if (res <= P.tol * sigma_top) break;
  }
  I.invit_iters = it;
  I.residual = res;
  std::vector<double> ev;
  if (eigvec) {
    ev.resize(L);
    HIP_TRY(hipMemcpyAsync(ev.data(), v, sizeof(double) * L, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  DPGO_TRY(finish_info());
  if (eigvec) std::copy(ev.begin(), ev.end(), eigvec);
  *lambda_min = lam;
  return DPGO_HIP_OK;
}

int dpgo_hip_exact_factor_info(dpgo_hip_problem h, long long* nodes, int* levels, int* max_s_tiles,
                               long long* panel_doubles, double* factor_ms, int* factor_count) {
  DPGO_TRY(check_handle(h));
  if (!nodes || !levels || !max_s_tiles || !panel_doubles || !factor_ms || !factor_count)
    return fail(DPGO_HIP_EINVAL, "null argument");
  auto& ex = h->ex;
  const long nn = ex.nodes;
  *nodes = ex.panel_doubles > 0 ? nn : 0;
  *levels = static_cast<int>(ex.levels.size());
  *max_s_tiles = 0;
  if (*nodes > 0) {
    std::vector<int> s(nn);
    HIP_TRY(hipMemcpy(s.data(), ex.s.p, sizeof(int) * nn, hipMemcpyDeviceToHost));
    for (int v : s) *max_s_tiles = std::max(*max_s_tiles, sn_pad(v * h->b) / kSnTile);
  }
  *panel_doubles = ex.panel_doubles;
  DPGO_TRY(resolve_factor_ms(h));
  *factor_ms = ex.factor_ms;
  *factor_count = ex.factor_count;
  return DPGO_HIP_OK;
}

int dpgo_hip_exact_fallback_agents(dpgo_hip_problem h, int* flags, int* count) {
  DPGO_TRY(check_handle(h));
  if (!count) return fail(DPGO_HIP_EINVAL, "null argument");
  auto& ex = h->ex;
  std::vector<int> f(h->K, 0);
  if (ex.state == 1 && ex.not_pd.p && ex.not_pd.n >= static_cast<size_t>(h->K)) {
    HIP_TRY(hipMemcpyAsync(f.data(), ex.not_pd.p, sizeof(int) * h->K, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  } else if (ex.state == 2) {
    std::fill(f.begin(), f.end(), 1);
  }
  *count = 0;
  for (int a = 0; a < h->K; ++a) *count += f[a] != 0;
  if (flags) std::copy(f.begin(), f.end(), flags);
  return DPGO_HIP_OK;
}

int dpgo_hip_exact_sweep_bytes(dpgo_hip_problem h, double* fwd_bytes, double* bwd_bytes) {
  DPGO_TRY(check_handle(h));
  if (!fwd_bytes || !bwd_bytes) return fail(DPGO_HIP_EINVAL, "null argument");
  *fwd_bytes = h->ex.panel_doubles > 0 ? h->ex.sweep_bytes_fwd : 0.0;
  *bwd_bytes = h->ex.panel_doubles > 0 ? h->ex.sweep_bytes_bwd : 0.0;
  return DPGO_HIP_OK;
}

int dpgo_hip_exact_factor_flops(dpgo_hip_problem h, double* cholesky_flops, double* inverse_flops) {
  DPGO_TRY(check_handle(h));
  if (!cholesky_flops || !inverse_flops) return fail(DPGO_HIP_EINVAL, "null argument");
  *cholesky_flops = h->ex.panel_doubles > 0 ? h->ex.flops : 0.0;
  *inverse_flops = h->ex.panel_doubles > 0 ? h->ex.inv_flops : 0.0;
  return DPGO_HIP_OK;
}

int dpgo_hip_bench_precond(dpgo_hip_problem h, const double* V_dev, int reps, double* ms_fwd, double* ms_bwd,
                           double* panel_bytes) {
  DPGO_TRY(problem_ready(h));
  DPGO_TRY(ensure_work_public(h));
  if (reps <= 0 || !ms_fwd || !ms_bwd || !panel_bytes) return fail(DPGO_HIP_EINVAL, "bad argument");
  DPGO_TRY(sync_chol(h));
  *ms_fwd = *ms_bwd = 0.0;
  *panel_bytes = 8.0 * static_cast<double>(h->ex.panel_doubles);  // the stored tiles (dpgo_hip_exact_sweep_bytes: read)
  if (h->ex.state != 1) return DPGO_HIP_OK;
  const SnView v = sn_view(h, FLAG_NONE);
  ScopedEvents sev(3);  // destroyed on every return, the early HIP_TRY ones included
  HIP_TRY(sev.create());
  hipEvent_t* ev = sev.ev.data();
  double tf = 0.0, tb = 0.0;
  for (int i = 0; i < kBenchWarmup + reps; ++i) {  // untimed applications first (see dpgo_hip_bench_hvp)
    HIP_TRY(hipEventRecord(ev[0], h->stream));
    DPGO_TRY(sweep_forward(h, v, V_dev));
    HIP_TRY(hipEventRecord(ev[1], h->stream));
    DPGO_TRY(sweep_backward(h, v));
    HIP_TRY(hipEventRecord(ev[2], h->stream));
    HIP_TRY(hipEventSynchronize(ev[2]));
    if (i >= kBenchWarmup) {
      float a = 0.f, b = 0.f;
      HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
      HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
      tf += a;
      tb += b;
    }
  }
  *ms_fwd = tf / reps;
  *ms_bwd = tb / reps;
  return DPGO_HIP_OK;
}

}  // extern "C"

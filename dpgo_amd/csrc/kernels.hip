// fp64 HIP kernels for the DPGO RBCD hot path on gfx950 (MI355X).
//
// Reference semantics (file:line relative to the reference root):
//   QuadraticProblem f / EucGrad / EucHessianEta / PreConditioner / RieGrad
//                                   src/QuadraticProblem.cpp:50-101
//   LiftedSEManifold projection / QF retraction / polar project
//                                   src/manifold/LiftedSEManifold.cpp:16-45, src/DPGO_utils.cpp:494-500
//   ROPTLIB RTRNewton / tCG          SURVEY.md Appendix A.4 (restated; un-vendored dependency)
//
// Every kernel works on a *tile set*: tile t covers up to 64 consecutive poses of one agent
// (agents = independent RBCD blocks batched into one launch).  See dpgo_device.h for the
// pose-quad lane mapping.
#include <algorithm>

#include "dpgo_device.h"
#include "kernels.h"
#include "pcm_pair.h"

namespace dpgo {

__device__ __forceinline__ bool agent_skipped(const AgentState* state, int flag_kind, int round, int agent) {
  if (flag_kind == FLAG_NONE || state == nullptr) return false;
  const AgentState& s = state[agent];
  if (flag_kind == FLAG_RUN) return s.run_active == 0;
  if (flag_kind == FLAG_TCG) return s.tcg_active == 0;
  if (flag_kind == FLAG_TCG_MODE) return s.tcg_mode == 2;
  if (flag_kind == FLAG_MOVED) return s.runs > 0 && s.accepted && !s.gave_up;
  if (flag_kind == FLAG_TCG_CG) return s.tcg_mode != 0;
  if (flag_kind == FLAG_RUN_IMPL) return s.run_active == 0 || s.eta_implicit == 0;
  if (flag_kind == FLAG_RUN_EXPL) return s.run_active == 0 || s.eta_implicit != 0;
  if (flag_kind == FLAG_DECIDED)  // accepted / gave up in Run `round`, or never ran (round 0)
    return !(s.run_active == 0 && (s.runs == round + 1 || (round == 0 && s.runs == 0)));
  return false;
}
__device__ __forceinline__ bool tile_skipped(const LaunchCtx& c, int agent) {
  return agent_skipped(c.state, c.flag_kind, c.round, agent);
}

template <int R, int B>
__device__ __forceinline__ void select_col(const double (&F)[R][B], int k, double (&c)[R]) {
  // Per-lane column pick.  The empty asm pins the candidates as SSA registers so the compiler
  // cannot fold the selects into a dynamically indexed (scratch) load of the array.
#pragma unroll
  for (int a = 0; a < R; ++a) {
    double v0 = F[a][0], v1 = F[a][1], v2 = F[a][2];
    double v3 = B > 3 ? F[a][B > 3 ? 3 : 0] : v0;
    asm("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));
    c[a] = (k & 2) ? ((k & 1) ? v3 : v2) : ((k & 1) ? v1 : v0);
  }
}

template <int R>
__device__ __forceinline__ void store_vec(double* __restrict__ P, long off, bool ok,
                                          const double (&c)[R]) {
  if (ok) {
#pragma unroll
    for (int a = 0; a < R; ++a) P[off + a] = c[a];
  }
}

// coherent: agent-scope (L2-bypassing) stores, read by a fused finalize in the same launch
template <int NQ>
__device__ __forceinline__ void block_partials(double (&v)[NQ], double* __restrict__ partials,
                                               int tile, bool coherent = false) {
  __shared__ double red[4][NQ > 0 ? NQ : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NQ; ++q) v[q] = wave_sum(v[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) red[wave][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double t = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
      if (coherent)
        __hip_atomic_store(&partials[tile * kPartialStride + q], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else
        partials[tile * kPartialStride + q] = t;
    }
  }
}

// One plain partial (slot 0) and ND double-double partials (high parts at slots slot[q], low parts kDdLo
// slots later), reduced in double-double over the wave and the block in block_partials' order.
struct DdSlots {
  int s[6];
};
constexpr DdSlots kSlots123456{{1, 2, 3, 4, 5, 6}};
constexpr DdSlots kSlots2356{{2, 3, 5, 6, 0, 0}};
template <int ND>
__device__ __forceinline__ void block_partials_dd_at(double v0, dd (&v)[ND], DdSlots slot, double* __restrict__ partials,
                                                     int tile, bool coherent = false) {
  __shared__ double red[4][1 + 2 * ND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v0 = wave_sum(v0);
#pragma unroll
  for (int q = 0; q < ND; ++q) v[q] = wave_sum_dd(v[q]);
  if (lane == 0) {
    red[wave][0] = v0;
#pragma unroll
    for (int q = 0; q < ND; ++q) {
      red[wave][1 + 2 * q] = v[q].hi;
      red[wave][2 + 2 * q] = v[q].lo;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    auto put = [&](int slot, double t) {
      if (coherent)
        __hip_atomic_store(&partials[tile * kPartialStride + slot], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else
        partials[tile * kPartialStride + slot] = t;
    };
    put(0, ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]);
#pragma unroll
    for (int q = 0; q < ND; ++q) {
      dd t{red[0][1 + 2 * q], red[0][2 + 2 * q]};
#pragma unroll
      for (int w = 1; w < 4; ++w) t = dd_add(t, {red[w][1 + 2 * q], red[w][2 + 2 * q]});
      put(slot.s[q], t.hi);
      put(slot.s[q] + kDdLo, t.lo);
    }
  }
}
template <int ND>
__device__ __forceinline__ void block_partials_dd(double v0, dd (&v)[ND], double* __restrict__ partials, int tile,
                                                  bool coherent = false) {
  block_partials_dd_at<ND>(v0, v, kSlots123456, partials, tile, coherent);
}

// block_partials_dd_at through LDS: every lane's double-double values go to `scratch` (2 ND kThreads
// doubles, the SpMM's record stage, dead after the edge loop) and wave w reduces quantities w, w + 4:
// one quantity per wave instead of every quantity on every wave.  Fixed order (lanes l, l + 128, l + 64,
// l + 192, then the wave tree), so the totals are reproducible; v0 takes block_partials' path (bitwise).
template <int ND>
__device__ __forceinline__ void block_partials_dd_lds(double v0, dd (&v)[ND], DdSlots slot, double* __restrict__ partials,
                                                      int tile, bool coherent, double* scratch) {
  __shared__ double red0[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v0 = wave_sum(v0);
  __syncthreads();  // every wave is past its edge loop: the record stage is free
  if (lane == 0) red0[wave] = v0;
#pragma unroll
  for (int q = 0; q < ND; ++q) {
    scratch[(2 * q) * kThreads + threadIdx.x] = v[q].hi;
    scratch[(2 * q + 1) * kThreads + threadIdx.x] = v[q].lo;
  }
  __syncthreads();
  auto put = [&](int sl, double t) {
    if (coherent)
      __hip_atomic_store(&partials[tile * kPartialStride + sl], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      partials[tile * kPartialStride + sl] = t;
  };
#pragma unroll
  for (int q0 = 0; q0 < ND; q0 += 4) {
    const int q = q0 + wave;  // wave-uniform
    if (q < ND) {
      auto at = [&](int i) { return dd{scratch[(2 * q) * kThreads + i], scratch[(2 * q + 1) * kThreads + i]}; };
      const dd x = wave_sum_dd(dd_add(dd_add(at(lane), at(lane + 128)), dd_add(at(lane + 64), at(lane + 192))));
      if (lane == 0) {
        int sl = slot.s[0];
#pragma unroll
        for (int u = 1; u < ND; ++u) sl = q == u ? slot.s[u] : sl;
        put(sl, x.hi);
        put(sl + kDdLo, x.lo);
      }
    }
  }
  if (threadIdx.x == 0) put(0, ((red0[0] + red0[1]) + red0[2]) + red0[3]);
}

// One plain partial v0 (block_partials' path and order, bitwise what the single-quantity passes write to slot 0)
// and NQ further quantities v[i] to slot sl[i], double-double where isdd[i] (low part kDdLo slots later), plain
// otherwise (v[i].lo ignored).  Every lane's values go through `scratch` (the SpMM's record stage, dead after the
// edge loop) and wave w reduces items w, w + 4, ...: one quantity per wave, each in its own arithmetic (a plain
// quantity costs a plain wave sum, not a double-double one).  Callers list the double-double items first so
// they land on different waves.  Fixed order throughout, so the totals are reproducible.
template <int NQ>
__device__ __forceinline__ void block_partials_mixed(double v0, const dd (&v)[NQ], const int (&sl)[NQ],
                                                     const bool (&isdd)[NQ], double* __restrict__ partials, int tile,
                                                     bool coherent, double* scratch) {
  __shared__ double red0[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v0 = wave_sum(v0);
  __syncthreads();  // every wave is past its edge loop: the record stage is free
  if (lane == 0) red0[wave] = v0;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    scratch[(2 * i) * kThreads + threadIdx.x] = v[i].hi;
    if (isdd[i]) scratch[(2 * i + 1) * kThreads + threadIdx.x] = v[i].lo;
  }
  __syncthreads();
  auto put = [&](int s, double t) {
    if (coherent)
      __hip_atomic_store(&partials[tile * kPartialStride + s], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      partials[tile * kPartialStride + s] = t;
  };
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    if (wave != (i & 3)) continue;  // wave-uniform
    const double* hi = scratch + (2 * i) * kThreads;
    if (isdd[i]) {
      const double* lo = scratch + (2 * i + 1) * kThreads;
      auto at = [&](int t) { return dd{hi[t], lo[t]}; };
      const dd x = wave_sum_dd(dd_add(dd_add(at(lane), at(lane + 128)), dd_add(at(lane + 64), at(lane + 192))));
      if (lane == 0) {
        put(sl[i], x.hi);
        put(sl[i] + kDdLo, x.lo);
      }
    } else {
      const double x = wave_sum((hi[lane] + hi[lane + 128]) + (hi[lane + 64] + hi[lane + 192]));
      if (lane == 0) put(sl[i], x);
    }
  }
  if (threadIdx.x == 0) put(0, ((red0[0] + red0[1]) + red0[2]) + red0[3]);
}

// block_partials_dd's layout from plain partials (v[0] plain, v[1 .. ND] the high parts, low parts zero)
template <int ND>
__device__ __forceinline__ void block_partials_lo0(double (&v)[13], double* __restrict__ partials, int tile,
                                                   bool coherent) {
  static_assert(1 + ND <= 13, "slots");
  double w[1 + ND];
#pragma unroll
  for (int q = 0; q <= ND; ++q) w[q] = v[q];
  block_partials<1 + ND>(w, partials, tile, coherent);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < ND; ++q) {
      if (coherent)
        __hip_atomic_store(&partials[tile * kPartialStride + 1 + q + kDdLo], 0.0, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      else
        partials[tile * kPartialStride + 1 + q + kDdLo] = 0.0;
    }
  }
}

// Per-lane sum of products for the merged tCG partials.  DPGO_MERGED_DD: 2 = dd_fma per term (exact
// products, double-double sums), 1 = Ogita-Rump-Oishi Dot2 (running sum by TwoSum, the product and sum
// errors gathered in one plain double: the same twice-the-working-precision result for a handful of
// terms at 10 instead of 13 flops a term), 0 = plain FMA chains (no low parts).
#ifndef DPGO_MERGED_DD
#define DPGO_MERGED_DD 2
#endif
constexpr bool kMergedDd = DPGO_MERGED_DD != 0;
struct DotAcc {
  double p = 0.0, s = 0.0;
  __device__ __forceinline__ void add(double a, double b) {
    if constexpr (DPGO_MERGED_DD == 0) {
      p = fma(a, b, p);
    } else if constexpr (DPGO_MERGED_DD == 1) {
      const double h = a * b;
      const double e = __builtin_fma(a, b, -h);
      const dd t = dd_two_sum(p, h);
      p = t.hi;
      s += t.lo + e;
    } else {
      const dd x = dd_fma({p, s}, a, b);
      p = x.hi;
      s = x.lo;
    }
  }
  __device__ __forceinline__ dd val() const {
    if constexpr (DPGO_MERGED_DD == 1) return dd_two_sum(p, s);
    return {p, s};
  }
};

// Column dot product of one lane (R terms): double-double (DotAcc) or a plain FMA chain (low part zero)
template <bool DD, int R>
__device__ __forceinline__ dd lane_dot(const double (&u)[R], const double (&v)[R]) {
  if constexpr (DD) {
    DotAcc t;
#pragma unroll
    for (int a = 0; a < R; ++a) t.add(u[a], v[a]);
    return t.val();
  } else {
    double t = 0.0;
#pragma unroll
    for (int a = 0; a < R; ++a) t = fma(u[a], v[a], t);
    return {t, 0.0};
  }
}

struct PoseLane {
  int lane, wave, k, tile, agent, pslot;
  long j;
  bool ok;
  int kk;  // column this lane owns (k < B) else -1
};

// The tile this block works on (tile_of_block, kernels.h; grid = the launch's tiles).  XCD: the kernel was remapped
// before the unified map (the edge-stream SpMM), so it follows tile_of_block whatever LaunchCtx::order says; the
// others only with ORDER_UNIFIED (order 0: tile = block).  Block-uniform scalar arithmetic.
template <bool XCD = false>
__device__ __forceinline__ int launch_tile(const LaunchCtx& c) {
  const int b = static_cast<int>(blockIdx.x);
  if (!XCD && (c.order & ORDER_UNIFIED) == 0) return b;
  return tile_of_block(b, static_cast<int>(gridDim.x), c.order & ORDER_REVERSE);
}

template <int B, bool XCD = false>
__device__ __forceinline__ PoseLane pose_lane(const LaunchCtx& c) {
  PoseLane p;
  p.lane = threadIdx.x & 63;
  p.wave = threadIdx.x >> 6;
  p.k = p.lane & 3;
  p.tile = launch_tile<XCD>(c);
  p.agent = c.tile_agent[p.tile];
  p.pslot = p.wave * kPosesPerWave + (p.lane >> 2);
  p.ok = p.pslot < c.tile_count[p.tile];
  p.j = static_cast<long>(c.tile_start[p.tile]) + p.pslot;
  p.kk = p.k < B ? p.k : -1;
  return p;
}

// ------------------------------------------------------------------------------------------
// X.Q SpMM over the symmetric block-sparse connection Laplacian with fused epilogues.
//   MODE_XQ    out = in Q                                   (EucHessianEta, :68-73)
//   MODE_XQ_G  out = in Q + G                               (EucGrad, :62-66)
//   MODE_EVAL  g = P_X(in Q + G), S = sym(Y^T (XQ+G)_Y), f and |g|^2 partials
//                                                           (f :50-60, RieGrad :89-97)
//   MODE_HESS  out = P_X(in Q - [in_Y S | 0]), <in, out> partial (Riemannian Hessian, A.3)
// BSR storage: block-row j lists neighbours i with block (j,i) of Q column-major, which is
// block (i,j) row-major (Q symmetric), so lane k streams row k of Q_ij: Y_j += X_i[:,k] Q_ij[k,:].
// ------------------------------------------------------------------------------------------
// Lane k of the pose quad accumulates sum_i X_i[:,k] (x) Q_ij[k,:] over block-row j.  UNR
// neighbours are processed per step with every load issued before the FMAs (memory-level
// parallelism: the column-index load and the dependent X gather of UNR neighbours overlap).
template <int R, int B, int UNR, bool NT>
__device__ __forceinline__ void spmm_accumulate(const QView& q, const double* __restrict__ in, long j, int k,
                                                double (&acc)[R][B]) {
  const int beg = q.rowptr[j], end = q.rowptr[j + 1];
  int nz = beg;
  auto load_blk = [&](int z, double (&bb)[B]) {
    const double* brow = q.blocks + static_cast<long>(z) * (B * B) + k * B;
    if constexpr (B == 4) {
      f64x2 b0, b1;
      if constexpr (NT) {
        b0 = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(brow));
        b1 = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(brow) + 1);
      } else {
        b0 = reinterpret_cast<const f64x2*>(brow)[0];
        b1 = reinterpret_cast<const f64x2*>(brow)[1];
      }
      bb[0] = b0.x; bb[1] = b0.y; bb[2] = b1.x; bb[3] = b1.y;
    } else {
#pragma unroll
      for (int cc = 0; cc < B; ++cc) bb[cc] = NT ? __builtin_nontemporal_load(brow + cc) : brow[cc];
    }
  };
  if constexpr (UNR > 1) {
    for (; nz + UNR <= end; nz += UNR) {
      long ii[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) ii[u] = q.col[nz + u];
      double bb[UNR][B], xx[UNR][R];
#pragma unroll
      for (int u = 0; u < UNR; ++u) load_blk(nz + u, bb[u]);
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const double* xk = in + ii[u] * (R * B) + k * R;
#pragma unroll
        for (int a = 0; a < R; ++a) xx[u][a] = xk[a];
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u)
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
          for (int cc = 0; cc < B; ++cc) acc[a][cc] = fma(xx[u][a], bb[u][cc], acc[a][cc]);
    }
  }
  for (; nz < end; ++nz) {
    const long i = q.col[nz];
    double bb[B], xx[R];
    load_blk(nz, bb);
    const double* xk = in + i * (R * B) + k * R;
#pragma unroll
    for (int a = 0; a < R; ++a) xx[a] = xk[a];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int cc = 0; cc < B; ++cc) acc[a][cc] = fma(xx[a], bb[cc], acc[a][cc]);
  }
}

// ------------------------------------------------------------------------------------------
// Edge-stream form of the same product (QFMT_EDGES).  For an edge e = (p1 -> p2) with
// T = [R t; 0 1], Omega = diag(k I_d, tau) and M = T Omega (src/DPGO_utils.cpp:214-286):
//   Q_{p1 p2} = -M,  Q_{p2 p1} = -M^T,  Q_{p1 p1} += T Omega T^T,  Q_{p2 p2} += Omega.
// Lane k of pose j's quad needs row k of the block (other, j):
//   j == p2 (incoming): block (p1, p2) = -M    -> row k of M     (offsets 4k + c)
//   j == p1 (outgoing): block (p2, p1) = -M^T  -> column k of M  (offsets 4c + k)
// so every lane issues the same four scalar loads with a per-incidence stride and the loop has no
// cross-lane traffic, no selects and no divergence.  The diagonal blocks are read once per pose.
// ------------------------------------------------------------------------------------------

// Per tile, the incidence entries and the records of the edges first visited by the tile (one
// contiguous id range, see QView) are staged in LDS with wide coalesced loads: the record stream
// leaves HBM at full occupancy-independent MLP instead of one dependent miss per incidence.
// Tiles whose lists do not fit fall back to global loads.
constexpr int kIncStage = 512;
// round 5's SpMM prologue: tile descriptors (LaunchCtx::tile_meta) and the stage loads issued together
#ifndef DPGO_STAGE_V5
#define DPGO_STAGE_V5 1
#endif
constexpr bool kStageV5 = DPGO_STAGE_V5 != 0;
// A/B builds only (-DDPGO_STAGE_DMA=1 -DDPGO_LDS_REC_PAD=0): the standalone X.Q's stage by LDS-DMA (global_load_lds:
// no VGPR destination, no ds_write pass).  Its LDS image is lane-linear, so the records lose their padding double
// (the 4-way bank conflicts the pad removed come back) -- DESIGN.md section 3.5 has the measurement.
#ifndef DPGO_STAGE_DMA
#define DPGO_STAGE_DMA 0
#endif
constexpr bool kStageDma = DPGO_STAGE_DMA != 0;
typedef __attribute__((address_space(3))) void lds_void_t;
#ifndef DPGO_BUFFER_GATHER
#define DPGO_BUFFER_GATHER 1
#endif
constexpr bool kBufferGather = DPGO_BUFFER_GATHER != 0;
constexpr bool kHalfStaged = false;  // LDS stage for the half passes (MODE_F / MODE_QF)
template <int D>
constexpr int rec_stage() { return D == 3 ? 200 : 256; }

// packed upper-triangle index of (u, v) in a symmetric B x B block
template <int B>
__host__ __device__ constexpr int sym_index(int u, int v) {
  return u <= v ? u * B - u * (u - 1) / 2 + (v - u) : v * B - v * (v - 1) / 2 + (u - v);
}

// S = sym(Y^T EG_Y) per pose, stored as its packed upper triangle (sym_index<D>)
__host__ __device__ constexpr int s_width(int d) { return d * (d + 1) / 2; }

// packed index of the block-Jacobi inverse (same packing as the diagonal blocks)
template <int B>
__host__ __device__ constexpr int minv_index(int u, int v) { return sym_index<B>(u, v); }

// acc (lane k: X_i[:,k] (x) Q_ij[k,:]) over incidences [z0, z1) of one pose.  Two register sets
// ping-pong so the record row/column + X column of incidence z+1 are in flight while incidence z
// is consumed; every load is unconditional (the index is clamped) so the compiler waits only for
// the stage it consumes.  INC_LDS: entries from the LDS stage (ds_read: waiting for them never
// drains in-flight global loads).  REC_LDS: records from the LDS stage (id - e0), else global.
// LDS stride of a staged edge record: one double of padding, so the records the 16 poses of a wave read at
// once start on different banks (a 128-byte stride put all of them on two bank offsets: 4-way conflicts)
#ifndef DPGO_LDS_REC_PAD
#define DPGO_LDS_REC_PAD 1
#endif
__host__ __device__ constexpr int lds_rec_stride(int b) { return edge_rec_width(b - 1) + DPGO_LDS_REC_PAD; }

// Raw buffer loads for the edge loop's gathers.  They are intrinsic calls, not IR loads: plain loads feeding
// the loop-carried register stage are folded by the optimizer into ONE load of a phi of the two addresses,
// issued right before its FMAs (no gather in flight while the previous incidence is consumed: a full L2/HBM
// latency per incidence); the intrinsics keep the stage's loads where the source puts them.  The range is
// 4 GiB per buffer (32-bit offsets): the launcher checks it (buffer_gather_ok).
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), static_cast<short>(0), -1, 0x00020000);
}
template <int N>
__device__ __forceinline__ void buf_load_f64(__amdgpu_buffer_rsrc_t r, unsigned off, double (&v)[N]) {
#pragma unroll
  for (int a = 0; a + 1 < N; a += 2) {
    const f64x2 t = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(r, off + 8u * a, 0, 0));
    v[a] = t.x;
    v[a + 1] = t.y;
  }
  if constexpr (N % 2 == 1)
    v[N - 1] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, off + 8u * (N - 1), 0, 0));
}

template <int R, int B, bool INC_LDS, bool REC_LDS, bool BUF = kBufferGather>
__device__ __forceinline__ void edge_loop(const QView& q, const double* __restrict__ in, int kc, int z0, int z1,
                                          const int2* s_inc, int i0, const double* s_rec, int e0,
                                          double (&acc)[R][B]) {
  constexpr int RW = edge_rec_width(B - 1);
  struct Stage {
    double m[B];
    double x[R];
  };
  const __amdgpu_buffer_rsrc_t rin = buf_rsrc(in), rrec = buf_rsrc(q.rec);
  auto fetch = [&](int z, Stage& st) {
    int2 ie;
    if constexpr (INC_LDS)
      ie = s_inc[z - i0];
    else
      ie = q.inc[z];
    const bool outg = (ie.x & 1) != 0;
    const int off = outg ? kc : 4 * kc;  // column kc of M (outgoing) / row kc (incoming)
    const int stride = outg ? 4 : 1;
    if constexpr (REC_LDS) {
      const double* mr = s_rec + ((ie.x >> 1) - e0) * lds_rec_stride(B) + off;
#pragma unroll
      for (int c = 0; c < B; ++c) st.m[c] = mr[c * stride];
    } else if constexpr (BUF) {
      const unsigned mo = 8u * (static_cast<unsigned>(ie.x >> 1) * RW + off);
#pragma unroll
      for (int c = 0; c < B; ++c)
        st.m[c] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rrec, mo + 8u * c * stride, 0, 0));
    } else {
      const double* mr = q.rec + static_cast<long>(ie.x >> 1) * RW + off;
#pragma unroll
      for (int c = 0; c < B; ++c) st.m[c] = mr[c * stride];
    }
    if constexpr (BUF) {
      buf_load_f64<R>(rin, 8u * (static_cast<unsigned>(ie.y) * (R * B) + kc * R), st.x);
    } else {
      const double* xk = in + static_cast<long>(ie.y) * (R * B) + kc * R;
#pragma unroll
      for (int a = 0; a < R; ++a) st.x[a] = xk[a];
    }
  };
  auto consume = [&](const Stage& st) {
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int c = 0; c < B; ++c) acc[a][c] = fma(-st.x[a], st.m[c], acc[a][c]);
  };
  if (z0 >= z1) return;
  Stage sa, sb;
  fetch(z0, sa);
  for (int nz = z0; nz < z1; nz += 2) {
    fetch(min(nz + 1, z1 - 1), sb);
    consume(sa);
    if (nz + 1 >= z1) break;
    fetch(min(nz + 2, z1 - 1), sa);
    consume(sb);
  }
}

// edge_loop for b = 4 with the XOR-rotated accumulator (quad_reduce_scatter_rot): lane kc accumulates column
// s ^ kc in slot s, so it reads the record entries in that order.  Row kc of M (incoming) is at offsets
// 4 kc + (s ^ kc) = 5 kc ^ s, column kc (outgoing) at kc + 4 (s ^ kc) = 5 kc ^ 4 s.  The stage of incidence z + 1
// is issued before incidence z is consumed and no branch separates the two (a loop exit between them let the
// compiler sink the next gather below the FMAs that should hide it); an odd tail is consumed after the loop.
template <int R, bool INC_LDS, bool REC_LDS>
__device__ __forceinline__ void edge_loop_rot(const QView& q, const double* __restrict__ in, int kc, int z0, int z1,
                                              const int2* s_inc, int i0, const double* s_rec, int e0,
                                              double (&acc)[R][4]) {
  constexpr int B = 4, RW = edge_rec_width(3);
  struct Stage {
    double m[B];
    double x[R];
  };
  const __amdgpu_buffer_rsrc_t rin = buf_rsrc(in), rrec = buf_rsrc(q.rec);
  const int k5 = 5 * kc;
  auto fetch = [&](int z, Stage& st) {
    int2 ie;
    if constexpr (INC_LDS)
      ie = s_inc[z - i0];
    else
      ie = q.inc[z];
    const int sh = (ie.x & 1) << 1;  // outgoing: stride 4 between the slots' entries
    if constexpr (REC_LDS) {
      const double* mr = s_rec + ((ie.x >> 1) - e0) * lds_rec_stride(B);
#pragma unroll
      for (int s = 0; s < B; ++s) st.m[s] = mr[k5 ^ (s << sh)];
    } else {
      const unsigned mo = 8u * static_cast<unsigned>(ie.x >> 1) * RW;
#pragma unroll
      for (int s = 0; s < B; ++s)
        st.m[s] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                                                 rrec, mo + 8u * static_cast<unsigned>(k5 ^ (s << sh)), 0, 0));
    }
    buf_load_f64<R>(rin, 8u * (static_cast<unsigned>(ie.y) * (R * B) + kc * R), st.x);
  };
  auto consume = [&](const Stage& st) {
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int s = 0; s < B; ++s) acc[a][s] = fma(-st.x[a], st.m[s], acc[a][s]);
  };
  if (z0 >= z1) return;
  Stage sa, sb;
  fetch(z0, sa);
  int nz = z0;
  for (; nz + 1 < z1; nz += 2) {
    fetch(nz + 1, sb);
    consume(sa);
    fetch(min(nz + 2, z1 - 1), sa);
    consume(sb);
  }
  if (nz < z1) consume(sa);
}

// One pipeline over every incidence of a pose (b = 4, rotated accumulator, staged tile): positions p < L1 are
// incidences a0 + p, the rest b0 + (p - L1), in that order -- the order of the separate loops it replaces, so the
// sums are bitwise theirs.  A record whose id is below the tile's first-visit range (a second visit) is read
// from HBM / L2, the others from the LDS stage; one two-stage pipeline instead of one per record source, so only
// the pose's first gather waits a full memory latency.
#ifndef DPGO_UNI_UNROLLED
#define DPGO_UNI_UNROLLED 1
#endif
constexpr bool kUniUnrolled = DPGO_UNI_UNROLLED != 0;
constexpr int kUniMax = 8;  // incidences per pose handled straight-line (a 3D lattice pose has at most 6)
#ifndef DPGO_UNI_AHEAD
#define DPGO_UNI_AHEAD 1
#endif
constexpr int kUniAhead = DPGO_UNI_AHEAD;  // straight-line loop: incidences fetched ahead of the one consumed
#ifndef DPGO_XQ_AHEAD
#define DPGO_XQ_AHEAD 3
#endif
constexpr int kXqAhead = DPGO_XQ_AHEAD;  // the same for the standalone X.Q (MODE_XQ / MODE_XQ_G)
template <int R, int AHEAD = kUniAhead>
__device__ __forceinline__ void edge_loop_uni(const QView& q, const double* __restrict__ in, int kc, int a0, int L1,
                                              int b0, int L2, const int2* s_inc, int i0, const double* s_rec, int e0,
                                              double (&acc)[R][4]) {
  constexpr int B = 4, RW = edge_rec_width(3);
  struct Stage {
    double m[B];
    double x[R];
  };
  const __amdgpu_buffer_rsrc_t rin = buf_rsrc(in), rrec = buf_rsrc(q.rec);
  const int k5 = 5 * kc, n = L1 + L2;
  auto fetch = [&](int pos, Stage& st) {
    const int z = pos < L1 ? a0 + pos : b0 + (pos - L1);
    const int2 ie = s_inc[z - i0];
    const int sh = (ie.x & 1) << 1;  // outgoing: stride 4 between the slots' entries
    const int id = ie.x >> 1;
    if (id >= e0) {
      const double* mr = s_rec + (id - e0) * lds_rec_stride(B);
#pragma unroll
      for (int s = 0; s < B; ++s) st.m[s] = mr[k5 ^ (s << sh)];
    } else {
      const unsigned mo = 8u * static_cast<unsigned>(id) * RW;
#pragma unroll
      for (int s = 0; s < B; ++s)
        st.m[s] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(
                                                 rrec, mo + 8u * static_cast<unsigned>(k5 ^ (s << sh)), 0, 0));
    }
    buf_load_f64<R>(rin, 8u * (static_cast<unsigned>(ie.y) * (R * B) + kc * R), st.x);
  };
  auto consume = [&](const Stage& st) {
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int s = 0; s < B; ++s) acc[a][s] = fma(-st.x[a], st.m[s], acc[a][s]);
  };
  if (n <= 0) return;
  if (kUniUnrolled && n <= kUniMax) {
    // Straight-line for the usual degrees: every stage its own registers, each written once and read once.  In the
    // two-stage loop the fetch into the reused stage is a phi of its LDS and global branches, and the register
    // allocator copies it at the back edge -- a copy that waits for the next incidence's record loads, so the
    // second-visit gathers never overlapped the loop's FMAs.
    Stage st[kUniMax];
#pragma unroll
    for (int q = 0; q < AHEAD; ++q)
      if (q < n) fetch(q, st[q]);
#pragma unroll
    for (int q = 0; q < kUniMax; ++q) {
      if (q + AHEAD < kUniMax) {
        if (q + AHEAD < n) fetch(q + AHEAD, st[q + AHEAD < kUniMax ? q + AHEAD : q]);
      }
      if (q < n) consume(st[q]);
    }
    return;
  }
  Stage sa, sb;
  fetch(0, sa);
  int p = 0;
  for (; p + 1 < n; p += 2) {
    fetch(p + 1, sb);
    consume(sa);
    fetch(min(p + 2, n - 1), sa);
    consume(sb);
  }
  if (p < n) consume(sa);
}

// Row kc of the pose's packed diagonal block in the rotated slot order (slot s = column s ^ kc), b = 4
__device__ __forceinline__ void diag_row_rot(const QView& q, long j, int kc, double (&dk)[4]) {
  constexpr int DW = diag_width(3);
  const double* dj = q.diag + j * DW;
  // packed upper-triangle index of (kc, c), c = s ^ kc: sym_index<4> restated without a dynamic table
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int c = s ^ kc;
    const int u = kc < c ? kc : c, v = kc < c ? c : kc;
    dk[s] = dj[u * 4 - u * (u - 1) / 2 + (v - u)];
  }
}

template <int R, int B, bool INC_LDS, bool REC_LDS, bool ROT>
__device__ __forceinline__ void edge_loop_any(const QView& q, const double* __restrict__ in, int kc, int z0, int z1,
                                              const int2* s_inc, int i0, const double* s_rec, int e0,
                                              double (&acc)[R][B]) {
  if constexpr (ROT) {
    static_assert(B == 4, "rotated accumulator: b = 4 only");
    edge_loop_rot<R, INC_LDS, REC_LDS>(q, in, kc, z0, z1, s_inc, i0, s_rec, e0, acc);
  } else {
    edge_loop<R, B, INC_LDS, REC_LDS>(q, in, kc, z0, z1, s_inc, i0, s_rec, e0, acc);
  }
}

// Block row j of X.Q for the edge-stream form: off-diagonal incidences (second visits through
// L2 first, then first visits from the LDS stage), then + X_j[:,k] (x) Q_jj[k,:].  The whole quad
// runs together; lane 3 of a d = 2 quad mirrors lane 0 and its acc is dropped.
//
// HALF (the f-only evaluation): tr(X Q X^T) = sum_j <X_j, X_j Q_jj> + 2 sum_edges <X_j, X_i Q_ij>, so
// each edge is needed once: only the first visits of pose j (ids [rec_first[j], rec_first[j+1]),
// all staged in LDS, the last entries of j's ascending list) are accumulated and the diagonal term
// enters with weight 1/2; then f_j = <X_j, acc_j> + <G_j, X_j>.  No second-visit record loads and
// half the neighbour gathers.
// NODIAG (the first-step quadratic form, MODE_QF / MODE_HESS_QF): the half sum without the diagonal
// term (added after the quad reduction, qf_first_step_dhd); the lane-3 mirror of a d = 2 quad is zeroed.
template <int R, int B, bool STAGED, bool HALF = false, bool NODIAG = false, bool ROT = false, bool UNI = false,
          int AHEAD = kUniAhead>
__device__ __forceinline__ void spmm_accumulate_edges(const QView& q, const double* __restrict__ in, long j,
                                                      int k, int beg, int end, const int2* s_inc, int i0,
                                                      const double* s_rec, int e0, double (&acc)[R][B],
                                                      double (&xown)[R]) {
  constexpr int DW = diag_width(B - 1);
  const int kc = k < B ? k : 0;
  if constexpr (HALF) {
    const int rf = q.rec_first[j];
    if constexpr (STAGED) {
      int mid = end;  // first visits of j are the largest ids of its list
      while (mid > beg && (s_inc[mid - 1 - i0].x >> 1) >= rf) --mid;
      edge_loop_any<R, B, true, true, ROT>(q, in, kc, mid, end, s_inc, i0, s_rec, e0, acc);
    } else {
      int mid = end;
      while (mid > beg && (q.inc[mid - 1].x >> 1) >= rf) --mid;
      edge_loop_any<R, B, false, false, ROT>(q, in, kc, mid, end, s_inc, i0, s_rec, e0, acc);
    }
  } else if constexpr (STAGED && UNI && ROT) {  // one pipeline over [beg, end), the record source per incidence
    edge_loop_uni<R, AHEAD>(q, in, kc, beg, end - beg, beg, 0, s_inc, i0, s_rec, e0, acc);
  } else if constexpr (STAGED) {
    int mid = beg;  // ids ascend: the second visits (ids below the tile's range) come first
    while (mid < end && (s_inc[mid - i0].x >> 1) < e0) ++mid;
    edge_loop_any<R, B, true, false, ROT>(q, in, kc, beg, mid, s_inc, i0, s_rec, e0, acc);
    edge_loop_any<R, B, true, true, ROT>(q, in, kc, mid, end, s_inc, i0, s_rec, e0, acc);
  } else {
    edge_loop_any<R, B, false, false, ROT>(q, in, kc, beg, end, s_inc, i0, s_rec, e0, acc);
  }
  double xj[R], dk[B];
  const double* pj = in + j * (R * B) + kc * R;
#pragma unroll
  for (int a = 0; a < R; ++a) xj[a] = pj[a];
  if constexpr (ROT) {
    double d4[4];
    diag_row_rot(q, j, kc, d4);
#pragma unroll
    for (int c = 0; c < B; ++c) dk[c] = d4[c < 4 ? c : 0];
  } else {
    const double* dj = q.diag + j * DW;
#pragma unroll
    for (int c = 0; c < B; ++c) {
      int o = sym_index<B>(0, c);
      if (kc == 1) o = sym_index<B>(1, c);
      if (kc == 2) o = sym_index<B>(2, c);
      if (B > 3 && kc == 3) o = sym_index<B>(B > 3 ? 3 : 0, c);
      dk[c] = dj[o];
    }
  }
  const bool act = k < B;
#pragma unroll
  for (int a = 0; a < R; ++a) xown[a] = act ? xj[a] : 0.0;  // column k of in_j (load_col), for the epilogues
  if constexpr (NODIAG) {
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int c = 0; c < B; ++c) acc[a][c] = act ? acc[a][c] : 0.0;
    return;
  }
#pragma unroll
  for (int a = 0; a < R; ++a) xj[a] = HALF ? 0.5 * xj[a] : xj[a];
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int c = 0; c < B; ++c) acc[a][c] = act ? fma(xj[a], dk[c], acc[a][c]) : 0.0;
}

// Row kc of the pose's packed symmetric diagonal block Q_jj (static indices only).
template <int B>
__device__ __forceinline__ void diag_row(const QView& q, long j, int kc, double (&dk)[B]) {
  constexpr int DW = diag_width(B - 1);
  const double* dj = q.diag + j * DW;
#pragma unroll
  for (int c = 0; c < B; ++c) {
    int o = sym_index<B>(0, c);
    if (kc == 1) o = sym_index<B>(1, c);
    if (kc == 2) o = sym_index<B>(2, c);
    if (B > 3 && kc == 3) o = sym_index<B>(B > 3 ? 3 : 0, c);
    dk[c] = dj[o];
  }
}

// column k of the quad-reduced running sum (the lane-3 mirror of a d = 2 quad masked out; for d = 3
// every lane is active and acc is reduced in place, no copy held across the edge loop)
template <int R, int B, bool ROT = false>
__device__ __forceinline__ void snapshot_half(const double (&acc)[R][B], int k, bool act, double (&qch)[R]) {
  if constexpr (ROT) {
    (void)act;
    (void)k;
    double a4[R][4];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) a4[a][c] = acc[a][c < B ? c : 0];
    quad_reduce_scatter_rot<R>(a4, qch);
  } else if constexpr (B == 4) {
    (void)act;
    quad_reduce_scatter<R, B>(acc, k, qch);
  } else {
    double half[R][B];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int c = 0; c < B; ++c) half[a][c] = act ? acc[a][c] : 0.0;
    quad_reduce_scatter<R, B>(half, k, qch);
  }
}

// MODE_HESS / MODE_HESS_QF accumulation of a block row of V.Q: the pose's own first visits (ids >=
// rec_first[j], the tail of its ascending list) first and from zero -- exactly the sum the MODE_QF pass
// forms -- then the other incidences, then the diagonal.  SNAP (MODE_HESS_QF): that first-visit sum
// is reduce-scattered into qch on the way (bitwise the QF pass's), so one pass gives Hess[V] and the
// first step's d_Hd; MODE_HESS runs the same order, so both passes give bitwise the same Hess[V].
// SV (second-visit staging): s_inc holds QView::inc_sv, whose record fields are tile-local LDS slots
// (second visits 0 .. sv_ns - 1, first visit id -> sv_ns + id - e0), so every incidence reads its record
// from LDS; the phase boundaries move to slot space and the order of additions is unchanged.
template <int R, int B, bool STAGED, bool SNAP, bool SV = false, bool ROT = false, bool UNI = false>
__device__ __forceinline__ void spmm_accumulate_edges_hq(const QView& q, const double* __restrict__ in, long j,
                                                         int k, int beg, int end, const int2* s_inc, int i0,
                                                         const double* s_rec, int e0, double (&acc)[R][B],
                                                         double (&xown)[R], double (&qch)[R], int sv_ns = 0) {
  const int kc = k < B ? k : 0;
  const bool act = k < B;
  const int rf = SV ? sv_ns + q.rec_first[j] - e0 : q.rec_first[j];
  int midh = end;
  if constexpr (STAGED) {
    const int bnd = SV ? sv_ns : e0, rbase = SV ? 0 : e0;
    int mid = beg;  // second visits (ids below the tile's range) | first visits of earlier poses of the tile
    while (mid < end && (s_inc[mid - i0].x >> 1) < bnd) ++mid;
    while (midh > mid && (s_inc[midh - 1 - i0].x >> 1) >= rf) --midh;
    if constexpr (UNI && ROT && !SV) {  // one pipeline: own first visits, then [beg, midh)
      if constexpr (SNAP) {
        edge_loop_uni<R>(q, in, kc, midh, end - midh, beg, 0, s_inc, i0, s_rec, e0, acc);
        snapshot_half<R, B, ROT>(acc, k, act, qch);
        edge_loop_uni<R>(q, in, kc, beg, midh - beg, beg, 0, s_inc, i0, s_rec, e0, acc);
      } else {
        edge_loop_uni<R>(q, in, kc, midh, end - midh, beg, midh - beg, s_inc, i0, s_rec, e0, acc);
      }
    } else {
      edge_loop_any<R, B, true, true, ROT>(q, in, kc, midh, end, s_inc, i0, s_rec, rbase, acc);
      if constexpr (SNAP) snapshot_half<R, B, ROT>(acc, k, act, qch);
      edge_loop_any<R, B, true, SV, ROT>(q, in, kc, beg, mid, s_inc, i0, s_rec, rbase, acc);
      edge_loop_any<R, B, true, true, ROT>(q, in, kc, mid, midh, s_inc, i0, s_rec, rbase, acc);
    }
  } else {
    while (midh > beg && (q.inc[midh - 1].x >> 1) >= rf) --midh;
    edge_loop_any<R, B, false, false, ROT>(q, in, kc, midh, end, s_inc, i0, s_rec, e0, acc);
    if constexpr (SNAP) snapshot_half<R, B, ROT>(acc, k, act, qch);
    edge_loop_any<R, B, false, false, ROT>(q, in, kc, beg, midh, s_inc, i0, s_rec, e0, acc);
  }
  double xj[R], dk[B];
  const double* pj = in + j * (R * B) + kc * R;
#pragma unroll
  for (int a = 0; a < R; ++a) xj[a] = pj[a];
  if constexpr (ROT) {
    double d4[4];
    diag_row_rot(q, j, kc, d4);
#pragma unroll
    for (int c = 0; c < B; ++c) dk[c] = d4[c < 4 ? c : 0];
  } else {
    diag_row<B>(q, j, kc, dk);
  }
#pragma unroll
  for (int a = 0; a < R; ++a) xown[a] = act ? xj[a] : 0.0;
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int c = 0; c < B; ++c) acc[a][c] = act ? fma(xj[a], dk[c], acc[a][c]) : 0.0;
}

// The first tCG step's d_Hd = <V, Hess[V]> = <V, VQ> - <V_Y, V_Y S> (A.3; P_X self-adjoint on tangent V)
// from the first-visit half sum: <V, VQ> = sum_j <V_j, 2 h_j + V_j Q_jj>, h_j = sum over j's first
// visits.  One formula for MODE_QF and MODE_HESS_QF, so an agent's first step does not depend on
// which of the two its batch ran.
template <int R, int B>
__device__ __forceinline__ double qf_first_step_dhd(const QView& q, long j, int k, bool ok, const double (&vcol)[R],
                                                    const double (&qch)[R], const double (&S)[B - 1][B - 1]) {
  constexpr int D = B - 1;
  const int kc = k < B ? k : 0;
  double dk[B];
  if (ok) {
    diag_row<B>(q, j, kc, dk);
  } else {
#pragma unroll
    for (int c = 0; c < B; ++c) dk[c] = 0.0;
  }
  double Vf[R][B], Vy[R][D], w[R], hc[R];
  quad_gather<R, B>(vcol, Vf);
  quad_gather_y<R, D>(vcol, Vy);
#pragma unroll
  for (int a = 0; a < R; ++a) {
    double dg = 0.0;  // column k of V_j Q_jj
#pragma unroll
    for (int u = 0; u < B; ++u) dg = fma(Vf[a][u], dk[u], dg);
    w[a] = fma(2.0, qch[a], dg);
  }
  sub_y_times_col<R, D>(Vy, S, k, w, hc);
  double dpart = 0.0;
#pragma unroll
  for (int a = 0; a < R; ++a) dpart = fma(vcol[a], hc[a], dpart);
  return dpart;
}

// SpMM variants: neighbours per step, non-temporal block loads, XCD tile remap
constexpr int var_unr(int v) { return v == 2 || v == 5 ? 2 : (v == 3 || v == 4) ? 4 : 1; }
constexpr bool var_nt(int v) { return v == 1; }  // default-policy loads measured faster (tools/spmm_ab.py)
constexpr bool var_xcd(int v) { return v == 4 || v == 5 || v == 6; }
// edge-stream variants: bit 0 = XCD-aware tile remap, bits 1-2 = register budget (minimum waves per
// SIMD requested from the compiler: 0 -> none, 1 -> 4, 2 -> 5, 3 -> 6), bit 3 = the epilogue's own-pose
// operands (X, S, Minv, G slot) loaded before the edge loop, their latency hidden behind it
constexpr bool evar_xcd(int v) { return (v & 1) != 0; }
constexpr int evar_waves(int v) { return ((v >> 1) & 3) == 0 ? 1 : 3 + ((v >> 1) & 3); }
constexpr bool evar_pre(int v) { return (v & 8) != 0; }
// bit 4: the merged tCG epilogue's operands (r_j, the Minv column) also loaded before the edge loop
constexpr bool evar_pre_r(int v) { return (v & 16) != 0; }
// bit 5: second-visit records staged in LDS with the first visits (QView::sv_*, the HESS passes)
constexpr bool evar_sv(int v) { return (v & 32) != 0; }
// bit 6 (round 4): the merged tCG partials in the precision kMergedDdSlots states, reduced one quantity per wave
// with plain quantities on plain paths
constexpr bool evar_v2(int v) { return (v & 64) != 0; }
// bit 7 (round 4): the XOR-rotated accumulator (quad_reduce_scatter_rot: no column selects in the quad reduction;
// b = 4), bitwise the plain one
constexpr bool evar_rot(int v) { return (v & 128) != 0; }
// bit 8 (round 4, with bit 7): one edge-loop pipeline per pose over both record sources (edge_loop_uni)
constexpr bool evar_uni(int v) { return (v & 256) != 0; }
constexpr int kSvStage = 376;  // records staged per tile with second visits: 3 blocks of ~53 KB LDS per CU


// column k of the packed block-Jacobi inverse (row-major b x b)
template <int B>
__device__ __forceinline__ void minv_col(const double* __restrict__ Minv, long j, int k, bool ok, double (&mk)[B]) {
#pragma unroll
  for (int u = 0; u < B; ++u) mk[u] = ok ? Minv[j * diag_width(B - 1) + minv_index<B>(u, k < B ? k : 0)] : 0.0;
}

// Column k of z = Prec(v) = P_X(v Minv) from column k of v (the quad holds the pose), Yx = the pose's
// Y block on every lane (quad_gather_y of X): the EVAL_TCG epilogue's formula.
template <int R, int B>
__device__ __forceinline__ void precond_col_mk(const double (&Yx)[R][B - 1], const double (&mk)[B], int k, int pmode,
                                               const double (&vc)[R], double (&zc)[R]) {
  constexpr int D = B - 1;
  if (pmode == PRECON_NONE) {
#pragma unroll
    for (int a = 0; a < R; ++a) zc[a] = vc[a];
    return;
  }
  double Vf[R][B];
  quad_gather<R, B>(vc, Vf);
  double zq[R];
#pragma unroll
  for (int a = 0; a < R; ++a) {
    double sacc = 0.0;
#pragma unroll
    for (int u = 0; u < B; ++u) sacc = fma(Vf[a][u], mk[u], sacc);
    zq[a] = sacc;
  }
  double S3[D][D];
  sym_ytm_cols<R, D>(Yx, zq, S3);
  sub_y_times_col<R, D>(Yx, S3, k, zq, zc);
}

template <int R, int B>
__device__ __forceinline__ void precond_col(const double (&Yx)[R][B - 1], const double* __restrict__ Minv, long j,
                                            int k, bool ok, int pmode, const double (&vc)[R], double (&zc)[R]) {
  double mk[B];
  if (pmode != PRECON_NONE) minv_col<B>(Minv, j, k, ok, mk);
  precond_col_mk<R, B>(Yx, mk, k, pmode, vc, zc);
}

// ------------------------------------------------------------------------------------------
// Per-agent finalize: reduce tile partials in a fixed order, run the scalar logic of the
// RTR / tCG state machine (A.4) on device.
// ------------------------------------------------------------------------------------------
// Next per-iteration trace record of the agent (zeroed, status -1), or nullptr when tracing is off or
// the agent's buffer is full (trace_n still counts, so the host sees the overflow).
__device__ __forceinline__ double* trace_record(const FinalizeArgs& f, int agent, AgentState& s, int op) {
  if (f.trace == nullptr) return nullptr;
  const int i = s.trace_n++;
  if (i >= f.trace_cap) return nullptr;
  double* t = f.trace + (static_cast<long>(agent) * f.trace_cap + i) * kTraceWidth;
#pragma unroll
  for (int q = 0; q < kTraceWidth; ++q) t[q] = 0.0;
  t[TR_OP] = op;
  t[TR_STATUS] = -1.0;
  return t;
}

// Cumulative statistics at the start of an optimize call (OP_EVAL_INIT / OP_EVAL_TCG_INIT).
__device__ __forceinline__ void count_call(const FinalizeArgs& f, int agent, AgentState& s) {
  const bool en = f.agent_enabled ? f.agent_enabled[agent] != 0 : true;
  if (!en) return;
  s.st_calls += 1;
  if (!s.run_active) s.st_early += 1;
}

// Reduced totals: pa's quantities first, then pb's, and pc's at the fixed slots kPcSlot.. (static register
// indices in the scalar logic, whatever nq_a / nq_b are).
constexpr int kPcSlot = kMaxTot - 1;
__device__ __forceinline__ const double* part_src(const FinalizeArgs& f, int q, int& qq) {
  if (f.rz_pc && (q == 1 || q == 4)) {
    qq = q == 1 ? 1 : 2;
    return f.pc;
  }
  if (q < f.nq_a) {
    qq = q;
    return f.pa;
  }
  if (q < f.nq_a + f.nq_b && q < kPcSlot) {
    qq = q - f.nq_a;
    return f.pb;
  }
  if (q >= kPcSlot && q - kPcSlot < f.nq_c) {
    qq = q - kPcSlot;
    return f.pc;
  }
  return nullptr;
}

// Merged tCG: fold the previous k_tcg_updir's <eta_old, Hdelta> (pc) into <eta, Heta> with that
// iteration's step and d_Hd -- OP_TCG_CHECK's recurrence, one launch later.
__device__ __forceinline__ void fold_eta_heta(const FinalizeArgs& f, const double (&tot)[kMaxTot], AgentState& s) {
  if (!s.eh_pending || f.nq_c < 1) return;
  s.eh_pending = 0;
  s.eta_Heta += s.step * (2.0 * tot[kPcSlot] + s.step * s.d_Hd);
}

// tCG step test (A.4 steps 1-3) on d_Hd = <delta, Hess[delta]>: alpha, the trust-region / negative
// curvature test, tau.  Shared by OP_TCG_STEP and the merged OP_TCG_STEP_CHECK.
__device__ __forceinline__ void tcg_step_test(const FinalizeArgs& f, int agent, double d_Hd, AgentState& s) {
  const OptScalars& o = f.opt;
  s.d_Hd = d_Hd;
  const double alpha = s.z_r / d_Hd;
  const double e_Pe_new = s.e_Pe + 2.0 * alpha * s.e_Pd + alpha * alpha * s.d_Pd;
  const double D2 = s.Delta * s.Delta;
  s.alpha = alpha;
  s.tcg_iters += 1;
  if (s.tcg_iters == 1 && o.first_full) s.st_first_full += 1;
  double* tr = trace_record(f, agent, s, OP_TCG_STEP);
  if (tr) {
    tr[TR_J] = s.tcg_iters - 1;
    tr[TR_DHD] = d_Hd;
    tr[TR_ALPHA] = alpha;
    tr[TR_DELTA] = s.Delta;
    tr[TR_RUN] = s.runs;
    tr[TR_ZR] = s.z_r;           // <z, r> the step uses
    tr[TR_NORM_R] = s.norm_r0;   // |r_0| of this tCG
  }
  if (d_Hd <= 0.0 || e_Pe_new >= D2) {
    const double tau = (-s.e_Pd + sqrt(s.e_Pd * s.e_Pd + s.d_Pd * (D2 - s.e_Pe))) / s.d_Pd;
    s.tau = tau;
    s.step = tau;
    s.tcg_mode = 1;
    s.tcg_status = d_Hd <= 0.0 ? TCG_NEGCURVTURE : TCG_EXCREGION;
    s.tcg_active = 0;
    if (tr) {
      tr[TR_TAU] = tau;
      tr[TR_STATUS] = s.tcg_status;
    }
    if (s.tcg_iters == 1) {
      // first step on the boundary (the common RBCD case): eta = tau delta and Heta = tau Hdelta
      // stay implicit.  delta = -z, so <g, eta> = -tau <z, g> and <eta, Heta> = tau^2 <delta, Hdelta>
      // (the same products as the explicit dots up to rounding)
      s.eta_implicit = 1;
      s.g_eta = -tau * s.z_r;
      s.eta_Heta = tau * tau * d_Hd;
      s.st_implicit += 1;
    }
  } else {
    s.e_Pe = e_Pe_new;
    s.step = alpha;
    s.tcg_mode = 0;
    s.st_cg_steps += 1;
  }
}

// |r_0| min(|r_0|^theta, kappa), the stopping test's threshold, once per tCG (A.4)
__device__ __forceinline__ void set_r_stop(const OptScalars& o, AgentState& s) {
  const double r0t = pow(s.norm_r0, o.theta);
  s.r_stop = s.norm_r0 * fmin(r0t, o.kappa);
  s.r_stop_lcon = o.kappa < r0t ? 1 : 0;
}

// tCG stopping test after a CG step (A.4 step 5) on |r_new|^2 and <z_new, r_new>: LCON / SCON exit, or
// beta and the e_Pd / d_Pd recurrences.  Shared by OP_TCG_CHECK and the merged ops.
__device__ __forceinline__ void tcg_stop_test(const FinalizeArgs& f, int agent, double norm_r2, double z_r_new,
                                              AgentState& s) {
  const OptScalars& o = f.opt;
  const double norm_r = sqrt(norm_r2);
  const int j = s.tcg_iters - 1;
  double* tr = trace_record(f, agent, s, OP_TCG_CHECK);
  if (tr) {
    tr[TR_J] = j;
    tr[TR_NORM_R] = norm_r;
    tr[TR_RUN] = s.runs;
  }
  if (j >= o.min_inner && norm_r <= s.r_stop) {
    s.tcg_status = s.r_stop_lcon ? TCG_LCON : TCG_SCON;
    s.tcg_active = 0;
    if (tr) tr[TR_STATUS] = s.tcg_status;
    return;
  }
  const double beta = z_r_new / s.z_r;
  if (tr) {
    tr[TR_ZR] = z_r_new;
    tr[TR_BETA] = beta;
  }
  s.beta = beta;
  s.e_Pd = beta * (s.e_Pd + s.alpha * s.d_Pd);
  s.d_Pd = z_r_new + beta * beta * s.d_Pd;
  s.z_r = z_r_new;
}

// Merged stopping test: |r_{j+1}|^2 and <z_{j+1}, r_{j+1}> as one-step polynomials in alpha over the
// HESS_M partials of r_j and Hdelta_j (r_{j+1} = r_j + alpha Hd, z_{j+1} = z_j + alpha Prec(Hd)):
//   tot[1] |r|^2, tot[2] <r,Hd>, tot[3] |Hd|^2, tot[4] <z,r>, tot[5] 2<z,Hd>, tot[6] <Minv Hd, Hd>.
// The base terms are recomputed from the stored r_j every iteration, so rounding does not accumulate.
// The partials arrive as double-double (tot = high, lo = low parts) and the polynomials are evaluated in
// double-double: their terms cancel by the tCG's residual drop, and exact terms leave only the final
// rounding (the classic sequence's direct inner products of r', z' agree to a few ulps).
__device__ __forceinline__ void merged_stop_test(const FinalizeArgs& f, int agent, const double (&tot)[kMaxTot],
                                                 const double (&lo)[kMaxTot], AgentState& s) {
  s.eh_pending = 1;  // the k_tcg_updir that applies this step leaves <eta_old, Hdelta> in pc
  if (s.tcg_mode != 0) return;
  const double a = s.step;
  const dd t1{tot[1], lo[1]}, t2{tot[2], lo[2]}, t3{tot[3], lo[3]}, t4{tot[4], lo[4]}, t5{tot[5], lo[5]},
      t6{tot[6], lo[6]};
  const dd n = dd_add(t1, dd_mul_d(dd_add(dd_mul_d(t2, 2.0), dd_mul_d(t3, a)), a));
  const dd z = dd_add(t4, dd_mul_d(dd_add(t5, dd_mul_d(t6, a)), a));
  tcg_stop_test(f, agent, fmax(dd_val(n), 0.0), dd_val(z), s);
}

// PGOAgentStatus after an update (src/PGOAgent.cpp:700-716): relativeChange = sqrt(|X - XPrev|^2 / n),
// readyToTerminate with GNC's converged-loop-closure ratio
__device__ __forceinline__ void set_status(const FinalizeArgs& f, int agent, double d2, AgentState& s) {
  const OptScalars& o = f.opt;
  const double rc = sqrt(d2 / static_cast<double>(f.agent_num_poses[agent]));
  const double ratio = f.conv_ratio ? f.conv_ratio[agent] : 1.0;
  s.status_rel_change = rc;
  s.ready = (rc > o.rel_tol || ratio < o.min_ratio) ? 0 : 1;
}

// The RTR / tCG scalar logic of one agent on its reduced partials tot[] (one thread).
// OPC >= 0: the op is known at compile time (a specialised k_finalize carries only that op's logic)
template <int OPC = -1>
__device__ __forceinline__ void finalize_scalar(const FinalizeArgs& f, int agent, const double (&tot)[kMaxTot],
                                                const double (&lo)[kMaxTot], AgentState& s) {
  const int nq = f.nq_a + f.nq_b;
  const OptScalars& o = f.opt;
  const bool filtered = (f.agent_filter == 1 && !s.eta_implicit) || (f.agent_filter == 2 && s.eta_implicit);
  switch (filtered ? -1 : (OPC >= 0 ? OPC : f.op)) {
    case OP_EVAL_INIT: {  // after EVAL at the initial iterate
      s.f1 = tot[0];
      s.ngf = sqrt(tot[1]);
      s.f_init = s.f1;
      s.ngf_init = s.ngf;
      s.f2 = s.f1;
      s.ngf2 = s.ngf;
      s.Delta = o.Delta0;
      s.Delta_max = o.Delta_max;
      s.run_active = f.agent_enabled ? (f.agent_enabled[agent] != 0 && !(s.ngf < o.tol)) : !(s.ngf < o.tol);
      count_call(f, agent, s);
      s.accepted = 0;
      s.runs = 0;
      s.outer_iters = 0;
      s.gave_up = 0;
      s.tcg_status = -1;
      s.tcg_iters = 0;
      s.tcg_active = 0;
      s.tcg_mode = 2;
      s.eta_implicit = 0;
      s.eh_pending = 0;
      break;
    }
    case OP_EVAL: {
      s.f1 = tot[0];
      s.ngf = sqrt(tot[1]);
      break;
    }
    case OP_EVAL_TCG_INIT: {  // OP_EVAL_INIT, then OP_TCG_INIT with <z, g> = tot[2], |r|^2 = |g|^2
      s.f1 = tot[0];
      s.ngf = sqrt(tot[1]);
      s.f_init = s.f1;
      s.ngf_init = s.ngf;
      s.f2 = s.f1;
      s.ngf2 = s.ngf;
      s.Delta = o.Delta0;
      s.Delta_max = o.Delta_max;
      s.run_active = f.agent_enabled ? (f.agent_enabled[agent] != 0 && !(s.ngf < o.tol)) : !(s.ngf < o.tol);
      count_call(f, agent, s);
      s.accepted = 0;
      s.runs = 0;
      s.outer_iters = 0;
      s.gave_up = 0;
      s.tcg_status = -1;
      s.tcg_iters = 0;
      s.copy_pending = 0;
      s.tcg_mode = 2;
      s.eta_implicit = 0;
      s.eh_pending = 0;
      if (!s.run_active) {
        s.tcg_active = 0;
        break;
      }
      s.z_r = tot[2];
      s.d_Pd = s.z_r;
      s.e_Pe = 0.0;
      s.e_Pd = 0.0;
      s.norm_r0 = sqrt(tot[1]);
      set_r_stop(o, s);
      s.tcg_active = 1;
      s.tcg_status = TCG_MAXITER;
      s.eta_Heta = 0.0;
      break;
    }
    case OP_TCG_INIT: {
      s.copy_pending = 0;
      s.eta_implicit = 0;
      s.eh_pending = 0;
      if (!s.run_active) {
        s.tcg_active = 0;
        s.tcg_mode = 2;
        break;
      }
      s.z_r = tot[0];
      s.d_Pd = s.z_r;
      s.e_Pe = 0.0;
      s.e_Pd = 0.0;
      s.norm_r0 = sqrt(tot[1]);
      set_r_stop(o, s);
      s.tcg_active = 1;
      s.tcg_mode = 2;
      s.tcg_status = TCG_MAXITER;
      s.tcg_iters = 0;
      s.eta_Heta = 0.0;
      break;
    }
    case OP_TCG_STEP: {  // after k_spmm<HESS>: tot[0] = <delta, H delta>
      if (!s.tcg_active) {
        s.tcg_mode = 2;
        break;
      }
      tcg_step_test(f, agent, tot[0], s);
      break;
    }
    case OP_TCG_CHECK: {  // after k_tcg_update: tot[0] = <z,r>, tot[1] = |r|^2, tot[2] = <eta_old, Hdelta>
      if (s.tcg_mode == 2 || s.eta_implicit) break;
      s.eta_Heta += s.step * (2.0 * tot[2] + s.step * s.d_Hd);  // <eta, Heta> after eta += step delta
      if (s.tcg_mode != 0) break;
      tcg_stop_test(f, agent, tot[1], tot[0], s);
      break;
    }
    case OP_TCG_STEP_CHECK: {  // merged iteration after k_spmm<HESS_M>: tot[0] = d_Hd, tot[1..6] (merged_stop_test)
      fold_eta_heta(f, tot, s);
      if (!s.tcg_active) {
        s.tcg_mode = 2;
        break;
      }
      // <z_j, r_j> recomputed from the stored r_j; the first step keeps EVAL_TCG's <z, g> (the same inner
      // product as a plain sum: a first step decided by MODE_QF uses that one, bitwise the same step)
      if (s.tcg_iters > 0) s.z_r = tot[4] + lo[4];
      tcg_step_test(f, agent, tot[0], s);
      if (s.eta_implicit) break;
      merged_stop_test(f, agent, tot, lo, s);
      break;
    }
    case OP_TCG_CHECK_M: {  // after k_spmm<HESS_M> over the agents a MODE_QF step test sent on a CG step
      if (s.tcg_mode != 0 || s.eta_implicit) break;
      merged_stop_test(f, agent, tot, lo, s);
      break;
    }
    case OP_RHO: {  // pa: <g,eta> [, <eta,HV>, |x2 - ref|^2, |x1 - ref|^2]; pb: f(x2), |grad(x2)|^2
      if (o.tail_fused && s.eh_pending && f.nq_c >= 1) s.st_tail += 1;  // the step k_retract applied
      fold_eta_heta(f, tot, s);
      if (!s.run_active) break;
      const bool sfold = o.status_fold && f.nq_a == 4;  // pa carries the status partials (slots 2, 3)
      s.tcg_active = 0;
      s.tcg_mode = 2;
      if (!s.eta_implicit) s.g_eta = tot[0];
      // selects between register copies (pinned by the empty asm): a select between two elements of tot[] is folded
      // into a dynamically indexed load, which puts tot[] in scratch memory -- and a kernel that needs scratch can
      // make the queue drain while the runtime sizes its scratch
      double t2 = tot[2], t3 = tot[3], t4 = tot[4], t5 = tot[5];
      asm("" : "+v"(t2), "+v"(t3), "+v"(t4), "+v"(t5));
      s.f2 = sfold ? t4 : t2;
      s.ngf2 = sqrt(sfold ? t5 : t3);
      const double denom = -s.g_eta - 0.5 * s.eta_Heta;
      s.rho = (s.f1 - s.f2) / denom;
      s.accepted = s.rho > 0.1 ? 1 : 0;
      double* tr = trace_record(f, agent, s, OP_RHO);
      if (tr) {
        tr[TR_J] = s.outer_iters;
        tr[TR_F1] = s.f1;
        tr[TR_F2] = s.f2;
        tr[TR_RHO] = s.rho;
        tr[TR_DELTA] = s.Delta;
        tr[TR_ACCEPTED] = s.accepted;
        tr[TR_NGF] = s.ngf;
        tr[TR_STATUS] = s.tcg_status;
        tr[TR_RUN] = s.runs;
        tr[TR_ALPHA] = s.tcg_iters;  // inner iterations of this Run
      }
      s.st_runs += 1;
      s.st_tcg_iters += s.tcg_iters;
#pragma unroll
      for (int q = 0; q < 5; ++q)  // static indices: the state stays in registers
        s.st_status[q] += s.tcg_status == q ? 1 : 0;  // static indices (no scratch, see above)
      if (s.rho < 0.25) {
        s.Delta = 0.25 * s.Delta;
      } else if (s.rho > 0.75 && (s.tcg_status == TCG_EXCREGION || s.tcg_status == TCG_NEGCURVTURE)) {
        s.Delta = fmin(2.0 * s.Delta, s.Delta_max);
      }
      s.outer_iters += 1;
      s.copy_pending = o.single_run ? 0 : s.accepted;
      if (o.single_run) {
        // QuadraticOptimizer::trustRegion Max_Iteration == 1 wrapper (src/QuadraticOptimizer.cpp:92-110)
        s.runs += 1;
        if (s.accepted) {
          s.run_active = 0;
        } else if (s.runs - 1 > 10) {
          s.gave_up = 1;
          s.run_active = 0;
          s.st_gave_up += 1;
        } else {
          const double radius = s.Delta_max / 4.0;
          s.Delta = radius;
          s.Delta_max = radius;
        }
        // the output is decided (accepted -> x2, gave up -> the input): its status from the retraction's
        // partials (a retry Run decides later)
        if (sfold && !s.run_active) set_status(f, agent, s.accepted && !s.gave_up ? t2 : t3, s);
      } else {
        if (s.accepted) {
          s.f1 = s.f2;
          s.ngf = s.ngf2;
        }
        if (s.ngf < o.tol || s.outer_iters >= o.max_iter) s.run_active = 0;
      }
      break;
    }
    case OP_REL_CHANGE: {
      s.rel_change = sqrt(tot[0] / static_cast<double>(f.agent_num_poses[agent]));
      break;
    }
    case OP_STATUS: {  // PGOAgent::iterate status (src/PGOAgent.cpp:700-716), tot[0] = |X - XPrev|^2
      set_status(f, agent, tot[0], s);
      break;
    }
    case OP_SUM: {
      f.out_sums[agent * 4 + 0] = tot[0];
      if (nq > 1) f.out_sums[agent * 4 + 1] = tot[1];
      if (nq > 2) f.out_sums[agent * 4 + 2] = tot[2];
      if (nq > 3) f.out_sums[agent * 4 + 3] = tot[3];
      break;
    }
    default:
      break;
  }
  if (f.pub != nullptr) {
    // word = tag << 3 | never << 2 | cg << 1 | flag (rho test only: cg = this Run's tCG took more than one
    // step, never = the agent did not run in this call)
    const int flag = f.pub_kind == 1 ? s.tcg_active : s.run_active;
    const int cg = f.pub_kind == 2 && s.tcg_iters > 1 ? 2 : 0;
    const int never = f.pub_kind == 2 && s.runs == 0 && !s.run_active ? 4 : 0;
    __hip_atomic_store(&f.pub[agent], (f.pub_tag << 3) | never | cg | (flag ? 1 : 0), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}


// Both reductions below evaluate the classic 256-wide LDS halving tree over per-thread serial sums
// (thread t sums tiles t, t + 256, ...; then pairs t, t + w for w = 128 .. 1), so fused and separate
// finalizes give bitwise the same sums.
static_assert(kThreads == 256, "the finalize reductions restate a 256-thread reduction tree");

// Fused path (one wave of the last-arriving SpMM block): lane l plays threads l, l + 64, l + 128,
// l + 192 (the two cross-wave levels in registers) and the six in-wave levels are shuffles (lane t
// adds lane t + w: the same pairs in the same order).  No LDS and no barrier; the state is read and
// written in place (a register copy would cost the SpMM ~50 VGPRs and a wave per SIMD of occupancy).
__device__ __forceinline__ void finalize_agent(const FinalizeArgs& f, int agent) {
  // One reduction body for every quantity (a rolled loop over q, totals through LDS): this code sits inside
  // every fusable SpMM, and eight unrolled copies of it (plain and double-double) tripled those kernels' code.
  __shared__ double s_tot[2 * kMaxTot];
  const int l = static_cast<int>(threadIdx.x) & 63;
  const int t0 = f.agent_tile_off[agent], t1 = f.agent_tile_off[agent + 1];
  auto ld = [&](const double* src, int t, int slot) {
    return f.coherent ? __hip_atomic_load(&src[t * kPartialStride + slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                      : src[t * kPartialStride + slot];
  };
#pragma unroll 1
  for (int q = 0; q < kMaxTot; ++q) {
    int qq = 0;
    const double* src = part_src(f, q, qq);
    double th = 0.0, tl = 0.0;
    if (src != nullptr) {
      if ((f.dd_mask >> q) & 1) {  // double-double quantity: the same tree in double-double
        dd a4[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          dd sv{0.0, 0.0};
          for (int t = t0 + l + 64 * v; t < t1; t += kThreads) sv = dd_add(sv, {ld(src, t, qq), ld(src, t, qq + kDdLo)});
          a4[v] = sv;
        }
        const dd x = wave_sum_dd(dd_add(dd_add(a4[0], a4[2]), dd_add(a4[1], a4[3])));
        th = x.hi;
        tl = x.lo;
      } else {
        double a4[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          double sv = 0.0;
          for (int t = t0 + l + 64 * v; t < t1; t += kThreads) sv += ld(src, t, qq);
          a4[v] = sv;
        }
        th = wave_sum((a4[0] + a4[2]) + (a4[1] + a4[3]));  // lane 0's halving tree
      }
    }
    if (l == 0) {
      s_tot[q] = th;
      s_tot[kMaxTot + q] = tl;
    }
  }
  if (l != 0) return;
  double tot[kMaxTot], lo[kMaxTot];
#pragma unroll
  for (int q = 0; q < kMaxTot; ++q) {
    tot[q] = s_tot[q];
    lo[q] = s_tot[kMaxTot + q];
  }
  finalize_scalar(f, agent, tot, lo, f.state[agent]);
}

template <int NQ>
__device__ void prologue_finalize(const FinalizeArgs& f, int agent, int* arrive, AgentState& sh);
__device__ void finalize_arrive(const FinalizeArgs& f, int agent, int* arrive, const AgentState& sh);

// Fused finalize (SpmmArgs::fin_arrive): every block of the launch arrives once per agent tile, after
// its partial is written (release: fence, then the count); the block that completes its agent's
// count runs the agent's finalize on wave 0 (acquire fence first) and resets the count.  Skipped
// tiles arrive too, so every agent is finalized exactly as by a separate k_finalize launch.
// fin_mode 1: device-scope fences around the count (each writes back the XCD's L2: slow).
// fin_mode 2: partials are agent-scope stores (block_partials coherent) that complete before the count
// (s_waitcnt vmcnt(0)); the finalize reads them with agent-scope loads; no cache maintenance.
__device__ __forceinline__ void spmm_arrive(const SpmmArgs& a, int agent) {
  if (a.fin_arrive == nullptr) return;
  __shared__ int s_last;
  __syncthreads();
  if (threadIdx.x == 0) {
    if (a.fin_mode == 2)
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this block's partial stores are acknowledged
    else
      __threadfence();
    const int n = a.fin.agent_tile_off[agent + 1] - a.fin.agent_tile_off[agent];
    const int old = atomicAdd(&a.fin_arrive[agent], 1);
    s_last = old == n - 1 ? 1 : 0;
    if (s_last) atomicExch(&a.fin_arrive[agent], 0);
  }
  __syncthreads();
  if (s_last == 0 || threadIdx.x >= 64) return;
  if (a.fin_mode != 2) __threadfence();
  finalize_agent(a.fin, agent);
}

template <int R, int B, int MODE, int VAR = 0, int FMT = QFMT_BSR>
__global__ __launch_bounds__(kThreads, FMT == QFMT_EDGES ? evar_waves(VAR) : 1) void k_spmm(LaunchCtx c, QView q,
                                                                                          SpmmArgs args) {
  const double* __restrict__ in = args.in;
  const int* __restrict__ gidx = args.gidx;
  const double* __restrict__ gblk = args.gblk;
  const double* __restrict__ X = args.X;
  const double* __restrict__ S_in = args.S_in;
  double* __restrict__ out = args.out;
  double* __restrict__ S_out = args.S_out;
  constexpr int D = B - 1;
  const PoseLane p = pose_lane<B, FMT == QFMT_EDGES ? evar_xcd(VAR) : var_xcd(VAR)>(c);
  constexpr bool ROT = FMT == QFMT_EDGES && B == 4 && evar_rot(VAR);
  constexpr bool UNI = ROT && evar_uni(VAR);
  // A staged edge-stream tile with its descriptor (LaunchCtx::tile_meta) decides its skip only after its stage loads
  // are issued: the agent's flag (a scalar load that depends on the tile's agent) then waits in parallel with them
  // instead of ahead of them.  A skipped tile's stage is read and dropped.
  constexpr bool kStageFmt = FMT == QFMT_EDGES && !(MODE == MODE_F || MODE == MODE_QF) &&
                             !(mode_hess(MODE) && evar_sv(VAR));
  const bool skip = tile_skipped(c, p.agent);
  const bool late_skip = kStageFmt && kStageV5 && c.tile_meta != nullptr;
  if (skip && !late_skip) {
    if constexpr (spmm_fusable(MODE)) spmm_arrive(args, p.agent);
    return;
  }

  // epilogue operands issued ahead of the edge loop (edge-stream variant bit 3)
  constexpr bool PRE = FMT == QFMT_EDGES && evar_pre(VAR);
  constexpr bool PRE_S = PRE && (mode_hess(MODE) || MODE == MODE_QF || MODE == MODE_CERT);
  constexpr bool PRE_X = PRE && mode_hess(MODE);
  constexpr bool PRE_M = PRE && MODE == MODE_EVAL_TCG;
  constexpr bool PRE_R = PRE && mode_merged(MODE) && evar_pre_r(VAR);
  double pre_x[R], pre_s[s_width(D)], pre_m[B], pre_r[R], pre_mk[B];
  int pre_slot = -1;
  if constexpr (PRE_R) {
    load_col<R, B>(args.rvec, p.j, p.k, p.ok, pre_r);
    if (args.pmode != PRECON_NONE) minv_col<B>(args.Minv, p.j, p.k, p.ok, pre_mk);
  }
  if constexpr (PRE_X) load_col_y<R, B>(X, p.j, p.k, p.ok, pre_x);  // X enters HESS only through its Y block
  if constexpr (PRE_S) {
#pragma unroll
    for (int q = 0; q < s_width(D); ++q) pre_s[q] = p.ok ? S_in[p.j * s_width(D) + q] : 0.0;
  }
  if constexpr (PRE_M) {
    if (args.pmode != PRECON_NONE) {
#pragma unroll
      for (int u = 0; u < B; ++u)
        pre_m[u] = p.ok ? args.Minv[p.j * diag_width(B - 1) + minv_index<B>(u, p.k < B ? p.k : 0)] : 0.0;
    }
    if (p.ok && p.k < B && gidx != nullptr) pre_slot = gidx[p.j];
  }

  double acc[R][B];
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int cc = 0; cc < B; ++cc) acc[a][cc] = 0.0;
  double* red_scratch = nullptr;  // merged tCG partials' LDS scratch (the record stage, after the edge loop)

  // column k of in_j: the edge stream reads it for the diagonal term and hands it to the epilogues
  double xin[R];
#pragma unroll
  for (int a = 0; a < R; ++a) xin[a] = 0.0;
  double qch[R];  // MODE_HESS_QF (edge stream): column k of the first-visit half sum
#pragma unroll
  for (int a = 0; a < R; ++a) qch[a] = 0.0;
  if constexpr (FMT == QFMT_EDGES) {
    // The half (each-edge-once) passes read only the tile's first-visit records, each exactly once and
    // as whole 128-byte lines per pose quad: they skip the LDS stage (less LDS, more resident waves).
    constexpr bool HALF = MODE == MODE_F || MODE == MODE_QF;
    constexpr bool STAGE = !HALF || kHalfStaged;
    constexpr bool SVS = STAGE && mode_hess(MODE) && evar_sv(VAR);
    constexpr int RW = edge_rec_width(B - 1), NREC = SVS ? kSvStage : STAGE ? rec_stage<B - 1>() : 2;
    constexpr int NINC = STAGE ? kIncStage : 2;
    __shared__ int2 s_inc[NINC];
    __shared__ int s_ptr[kTilePoses + 1];
    __shared__ int s_e[4];
    constexpr int RS = lds_rec_stride(B);
    __shared__ double s_recd[NREC * RS];
    if constexpr (STAGE && mode_merged(MODE)) {
      static_assert(NREC * RS >= 2 * 6 * kThreads, "the record stage doubles as the merged partials' scratch");
      red_scratch = s_recd;
    }
    const int t0 = c.tile_start[p.tile], cnt = c.tile_count[p.tile];
    int i0, ni, e0, ne;
    if (late_skip) {  // the stage ranges from the tile descriptor: the pointers below load in parallel with them
      const int4 tm = c.tile_meta[p.tile];
      i0 = tm.x;
      ni = tm.y;
      e0 = tm.z;
      ne = tm.w;
      if (static_cast<int>(threadIdx.x) <= cnt) s_ptr[threadIdx.x] = q.inc_ptr[t0 + threadIdx.x];
    } else {
      if (static_cast<int>(threadIdx.x) <= cnt) s_ptr[threadIdx.x] = q.inc_ptr[t0 + threadIdx.x];
      if (threadIdx.x < 2) s_e[threadIdx.x] = q.rec_first[t0 + (threadIdx.x ? cnt : 0)];
      if (SVS && threadIdx.x >= 2 && threadIdx.x < 4) s_e[threadIdx.x] = q.sv_ptr[p.tile + threadIdx.x - 2];
      __syncthreads();
      i0 = s_ptr[0];
      ni = s_ptr[cnt] - i0;
      e0 = s_e[0];
      ne = s_e[1] - e0;
    }
    const int sv0 = SVS ? s_e[2] : 0, ns = SVS ? s_e[3] - s_e[2] : 0;
    const bool staged = STAGE && ni <= NINC && ns + ne <= NREC;
    if (staged) {
      if constexpr (SVS) {
        for (int x = threadIdx.x; x < ni; x += kThreads) s_inc[x] = q.inc_sv[i0 + x];
        // second-visit records gathered whole (RW / 2 lanes per record, 16-byte loads), first visits after
        const f64x2* all = reinterpret_cast<const f64x2*>(q.rec);
        for (int x = threadIdx.x; x < ns * (RW / 2); x += kThreads) {
          const int rr = x / (RW / 2), w = x - rr * (RW / 2);
          const f64x2 v = all[static_cast<long>(q.sv_ids[sv0 + rr]) * (RW / 2) + w];
          s_recd[rr * RS + 2 * w] = v.x;
          s_recd[rr * RS + 2 * w + 1] = v.y;
        }
        const f64x2* src = all + static_cast<long>(e0) * (RW / 2);
        for (int x = threadIdx.x; x < ne * (RW / 2); x += kThreads) {
          const int rr = x / (RW / 2), w = x - rr * (RW / 2);
          const f64x2 v = src[x];
          s_recd[(ns + rr) * RS + 2 * w] = v.x;
          s_recd[(ns + rr) * RS + 2 * w + 1] = v.y;
        }
      } else if constexpr (kStageDma && (MODE == MODE_XQ || MODE == MODE_XQ_G)) {
        static_assert(RS == RW, "LDS-DMA staging writes the records lane-linearly: build with DPGO_LDS_REC_PAD=0");
        const int lane = static_cast<int>(threadIdx.x) & 63, wave = static_cast<int>(threadIdx.x) >> 6;
        const int nw = 2 * ni;  // incidences as 4-byte words (int2 entries need only 4-byte alignment)
        const int* isrc = reinterpret_cast<const int*>(q.inc + i0);
        for (int w0 = wave * 64; w0 < nw; w0 += kThreads)
          __builtin_amdgcn_global_load_lds(isrc + min(w0 + lane, nw - 1),
                                           (lds_void_t*)(reinterpret_cast<int*>(s_inc) + w0), 4, 0, 0);
        const int nc = ne * (RW / 2);  // records as 16-byte chunks
        const f64x2* rsrc = reinterpret_cast<const f64x2*>(q.rec) + static_cast<long>(e0) * (RW / 2);
        for (int c0 = wave * 64; c0 < nc; c0 += kThreads)
          __builtin_amdgcn_global_load_lds(rsrc + min(c0 + lane, nc - 1), (lds_void_t*)(s_recd + 2 * c0), 16, 0, 0);
      } else if constexpr (!kStageV5) {  // round 4's stage loop (A/B builds only, -DDPGO_STAGE_V5=0)
        for (int x = threadIdx.x; x < ni; x += kThreads) s_inc[x] = q.inc[i0 + x];
        const f64x2* src = reinterpret_cast<const f64x2*>(q.rec) + static_cast<long>(e0) * (RW / 2);
        for (int x = threadIdx.x; x < ne * (RW / 2); x += kThreads) {
          const int rr = x / (RW / 2), w = x - rr * (RW / 2);
          const f64x2 v = src[x];
          s_recd[rr * RS + 2 * w] = v.x;
          s_recd[rr * RS + 2 * w + 1] = v.y;
        }
      } else {
        // two phases: every stage load of the thread in flight at once, then the LDS writes (a load / wait / write
        // loop costs one memory latency per trip: up to 2 + 7 of them per tile)
        constexpr int KI = (NINC + kThreads - 1) / kThreads, KR = (NREC * (RW / 2) + kThreads - 1) / kThreads;
        int2 iv[KI];
        f64x2 rv[KR];
        const f64x2* src = reinterpret_cast<const f64x2*>(q.rec) + static_cast<long>(e0) * (RW / 2);
        const int nr = ne * (RW / 2);
#pragma unroll
        for (int u = 0; u < KI; ++u) {
          const int x = static_cast<int>(threadIdx.x) + u * kThreads;
          if (x < ni) iv[u] = q.inc[i0 + x];
        }
#pragma unroll
        for (int u = 0; u < KR; ++u) {
          const int x = static_cast<int>(threadIdx.x) + u * kThreads;
          if (x < nr) rv[u] = src[x];
        }
#pragma unroll
        for (int u = 0; u < KI; ++u) {
          const int x = static_cast<int>(threadIdx.x) + u * kThreads;
          if (x < ni) s_inc[x] = iv[u];
        }
#pragma unroll
        for (int u = 0; u < KR; ++u) {
          const int x = static_cast<int>(threadIdx.x) + u * kThreads;
          if (x < nr) {
            const int rr = x / (RW / 2), w = x - rr * (RW / 2);
            s_recd[rr * RS + 2 * w] = rv[u].x;
            s_recd[rr * RS + 2 * w + 1] = rv[u].y;
          }
        }
      }
    }
    if (late_skip && skip) {  // uniform over the block: every thread leaves here
      if constexpr (kStageDma) __builtin_amdgcn_s_waitcnt(0);  // no LDS-DMA write may outlive the workgroup
      if constexpr (spmm_fusable(MODE)) spmm_arrive(args, p.agent);
      return;
    }
    if constexpr (STAGE) {
      __syncthreads();
    } else {
      if (late_skip) __syncthreads();  // (never: late_skip needs the stage) s_ptr written above
    }
    constexpr bool NODIAG = MODE == MODE_QF;
    if (p.ok) {
      const double* s_rec = s_recd;
      if constexpr (mode_hess(MODE)) {
        constexpr bool SNAP = mode_snap(MODE);
        if (staged)
          spmm_accumulate_edges_hq<R, B, true, SNAP, SVS, ROT, UNI>(q, in, p.j, p.k, s_ptr[p.pslot],
                                                                    s_ptr[p.pslot + 1], s_inc, i0, s_rec, e0, acc,
                                                                    xin, qch, ns);
        else
          spmm_accumulate_edges_hq<R, B, false, SNAP, false, ROT>(q, in, p.j, p.k, s_ptr[p.pslot],
                                                                  s_ptr[p.pslot + 1], s_inc, i0, s_rec, e0, acc, xin,
                                                                  qch);
      } else if (staged) {
        // the standalone X.Q gathers three incidences ahead (135 VGPRs, 3 waves): 97.8-97.9 us against 98.2-99.5 (two
        // ahead, 4 waves) and 98.8-99.2 (one ahead, 4 waves), profiles/r05o_xq_*.json -- about 1 %; the in-step modes
        // (HESS_M: a wave lost for the deeper prefetch costs more, profiles/r05i_ab_uni_ahead*.json) one ahead
        constexpr int kAhead = (MODE == MODE_XQ || MODE == MODE_XQ_G) ? kXqAhead : kUniAhead;
        spmm_accumulate_edges<R, B, true, HALF, NODIAG, ROT, UNI, kAhead>(q, in, p.j, p.k, s_ptr[p.pslot],
                                                                  s_ptr[p.pslot + 1], s_inc, i0, s_rec, e0, acc, xin);
      } else {
        spmm_accumulate_edges<R, B, false, HALF, NODIAG, ROT>(q, in, p.j, p.k, s_ptr[p.pslot], s_ptr[p.pslot + 1],
                                                              s_inc, i0, s_rec, e0, acc, xin);
      }
    }
  } else {
    if (p.ok && p.k < B) spmm_accumulate<R, B, var_unr(VAR), var_nt(VAR)>(q, in, p.j, p.k, acc);
    if constexpr (MODE != MODE_XQ && MODE != MODE_XQ_G) load_col<R, B>(in, p.j, p.k, p.ok, xin);
  }
  // lane k keeps column k of the block row only (quad reduce-scatter; same additions, same
  // order as a quad all-reduce, so bitwise identical to it) and the epilogues work column-locally
  double qc[R];
  if constexpr (ROT) {
    double a4[R][4];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) a4[a][cc] = acc[a][cc < B ? cc : 0];
    quad_reduce_scatter_rot<R>(a4, qc);
  } else {
    quad_reduce_scatter<R, B>(acc, p.k, qc);
  }

  const long off = p.j * (R * B) + p.k * R;
  const bool own = p.ok && p.k < B;

  if constexpr (MODE == MODE_XQ) {
    store_vec<R>(out, off, own, qc);
  } else if constexpr (MODE == MODE_XQ_G) {
    if (own && gidx != nullptr) {
      const int slot = gidx[p.j];
      if (slot >= 0) {
#pragma unroll
        for (int a = 0; a < R; ++a) qc[a] += gblk[static_cast<long>(slot) * (R * B) + p.k * R + a];
      }
    }
    store_vec<R>(out, off, own, qc);
  } else if constexpr (MODE == MODE_EVAL || MODE == MODE_F || MODE == MODE_EVAL_TCG) {
    double xcol[R], gcol[R];
    if (X == in) {  // the evaluation point is the SpMM input (always, through eval_at)
#pragma unroll
      for (int a = 0; a < R; ++a) xcol[a] = xin[a];
    } else {
      load_col<R, B>(X, p.j, p.k, p.ok, xcol);
    }
#pragma unroll
    for (int a = 0; a < R; ++a) gcol[a] = 0.0;
    if (own && gidx != nullptr) {
      const int slot = PRE_M ? pre_slot : gidx[p.j];
      if (slot >= 0) {
#pragma unroll
        for (int a = 0; a < R; ++a) gcol[a] = gblk[static_cast<long>(slot) * (R * B) + p.k * R + a];
      }
    }
    double fpart = 0.0;
    // edge-stream MODE_F accumulates the half sum (spmm_accumulate_edges HALF): qc already carries the 1/2
    constexpr double kq = (MODE == MODE_F && FMT == QFMT_EDGES) ? 1.0 : 0.5;
#pragma unroll
    for (int a = 0; a < R; ++a) fpart = fma(fma(kq, qc[a], gcol[a]), xcol[a], fpart);
    if constexpr (MODE == MODE_F) {  // f only (QuadraticProblem::f, :50-60)
      double parts[2] = {own ? fpart : 0.0, 0.0};
      block_partials<2>(parts, c.partials, p.tile, args.fin_mode == 2);
    } else {
      double eg[R];  // column k of the Euclidean gradient XQ + G
#pragma unroll
      for (int a = 0; a < R; ++a) eg[a] = qc[a] + gcol[a];
      double Yf[R][D];
      quad_gather_y<R, D>(xcol, Yf);
      double S[D][D];
      sym_ytm_cols<R, D>(Yf, eg, S);  // S = sym(Y^T EG_Y), on every lane of the quad
      double gc[R];
      sub_y_times_col<R, D>(Yf, S, p.k, eg, gc);  // column k of P_X(EG)
      double gpart = 0.0;
#pragma unroll
      for (int a = 0; a < R; ++a) gpart = fma(gc[a], gc[a], gpart);
      if (out != nullptr) store_vec<R>(out, off, own, gc);
      if (p.ok && p.k == 0 && S_out != nullptr) {
#pragma unroll
        for (int u = 0; u < D; ++u)
#pragma unroll
          for (int v = u; v < D; ++v) S_out[p.j * s_width(D) + sym_index<D>(u, v)] = S[u][v];
      }
      if constexpr (MODE == MODE_EVAL_TCG) {
        // tCG start fused in (A.4, k_tcg_init): z = Prec(g) = P_X(g Minv), delta = -z, <z, g>
        double zc[R];
        if (args.pmode == PRECON_NONE) {
#pragma unroll
          for (int a = 0; a < R; ++a) zc[a] = gc[a];
        } else {
          double Gf[R][B];
          quad_gather<R, B>(gc, Gf);
          double mk[B];  // column k of Minv (row-major b x b)
#pragma unroll
          for (int u = 0; u < B; ++u)
            mk[u] = PRE_M ? pre_m[u]
                          : (p.ok ? args.Minv[p.j * diag_width(B - 1) + minv_index<B>(u, p.k < B ? p.k : 0)] : 0.0);
          double zq[R];
#pragma unroll
          for (int a = 0; a < R; ++a) {
            double sacc = 0.0;
#pragma unroll
            for (int u = 0; u < B; ++u) sacc = fma(Gf[a][u], mk[u], sacc);
            zq[a] = sacc;
          }
          double S3[D][D];
          sym_ytm_cols<R, D>(Yf, zq, S3);
          sub_y_times_col<R, D>(Yf, S3, p.k, zq, zc);
        }
        double zr = 0.0, dc[R];
#pragma unroll
        for (int a = 0; a < R; ++a) {
          zr = fma(zc[a], gc[a], zr);
          dc[a] = -zc[a];
        }
        store_vec<R>(args.delta, off, own, dc);
        double parts[3] = {own ? fpart : 0.0, own ? gpart : 0.0, own ? zr : 0.0};
        block_partials<3>(parts, c.partials, p.tile, args.fin_mode == 2);
      } else {
        // third partial <G, X>: the central cost of a partitioned graph is sum_agents f - <G, X> / 2
        // (each shared edge's cross term enters both endpoint agents' linear terms)
        double gx = 0.0;
#pragma unroll
        for (int a = 0; a < R; ++a) gx = fma(gcol[a], xcol[a], gx);
        double parts[3] = {own ? fpart : 0.0, own ? gpart : 0.0, own ? gx : 0.0};
        block_partials<3>(parts, c.partials, p.tile, args.fin_mode == 2);
      }
    }
  } else if constexpr (MODE == MODE_CERT) {
    // certificate matrix S(X) = Q - Lambda(X), Lambda_j = [S_j 0; 0 0] (S_j = sym(Y_j^T EG_Y))
    double vcol[R];
#pragma unroll
    for (int a = 0; a < R; ++a) vcol[a] = xin[a];
    double S[D][D];
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
      for (int v = 0; v < D; ++v)
        S[u][v] = PRE_S ? pre_s[sym_index<D>(u, v)] : (p.ok ? S_in[p.j * s_width(D) + sym_index<D>(u, v)] : 0.0);
    double Vf[R][D], hc[R];
    quad_gather_y<R, D>(vcol, Vf);
    sub_y_times_col<R, D>(Vf, S, p.k, qc, hc);
    store_vec<R>(out, off, own, hc);
  } else if constexpr (MODE == MODE_QF) {
    // d_Hd = <V, Hess[V]> = <V, VQ> - <V_Y, V_Y S> for a tangent V (A.3; P_X is self-adjoint), without
    // forming Hess[V].  The edge stream accumulates each edge once (HALF), so <V, VQ> = 2 sum_j <V_j, acc_j>.
    double vcol[R];
#pragma unroll
    for (int a = 0; a < R; ++a) vcol[a] = xin[a];
    double S[D][D];
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
      for (int v = 0; v < D; ++v)
        S[u][v] = PRE_S ? pre_s[sym_index<D>(u, v)] : (p.ok ? S_in[p.j * s_width(D) + sym_index<D>(u, v)] : 0.0);
    double dpart = 0.0;
    if constexpr (FMT == QFMT_EDGES) {
      // qc: the first-visit half sum without the diagonal (NODIAG)
      dpart = qf_first_step_dhd<R, B>(q, p.j, p.k, p.ok, vcol, qc, S);
    } else {  // BSR: the full row, <V, VQ> = sum_j <V_j, (VQ)_j>
      double Vf[R][D], hc[R];
      quad_gather_y<R, D>(vcol, Vf);
      sub_y_times_col<R, D>(Vf, S, p.k, qc, hc);
#pragma unroll
      for (int a = 0; a < R; ++a) dpart = fma(vcol[a], hc[a], dpart);
    }
    double parts[1] = {own ? dpart : 0.0};
    block_partials<1>(parts, c.partials, p.tile, args.fin_mode == 2);
  } else if constexpr (mode_hess(MODE)) {
    double vcol[R], xcol[R];
#pragma unroll
    for (int a = 0; a < R; ++a) vcol[a] = xin[a];
    if constexpr (PRE_X) {
#pragma unroll
      for (int a = 0; a < R; ++a) xcol[a] = pre_x[a];
    } else {
      load_col_y<R, B>(X, p.j, p.k, p.ok, xcol);
    }
    double S[D][D];
#pragma unroll
    for (int u = 0; u < D; ++u)
#pragma unroll
      for (int v = 0; v < D; ++v)
        S[u][v] = PRE_S ? pre_s[sym_index<D>(u, v)] : (p.ok ? S_in[p.j * s_width(D) + sym_index<D>(u, v)] : 0.0);
    double dpart = 0.0;
    if constexpr (mode_snap(MODE) && FMT == QFMT_EDGES) {  // the first step's d_Hd by the MODE_QF formula
      dpart = qf_first_step_dhd<R, B>(q, p.j, p.k, p.ok, vcol, qch, S);  // (first: its temporaries die here)
      __builtin_amdgcn_sched_barrier(0);
    }
    double h1[R], hc[R];
    {
      double Vf[R][D];
      quad_gather_y<R, D>(vcol, Vf);
      sub_y_times_col<R, D>(Vf, S, p.k, qc, h1);  // VQ - V_Y S
    }
    __builtin_amdgcn_sched_barrier(0);  // V's gathered rows die before X's are gathered (register peak)
    double Xf[R][D];
    quad_gather_y<R, D>(xcol, Xf);
    double S2[D][D];
    sym_ytm_cols<R, D>(Xf, h1, S2);
    sub_y_times_col<R, D>(Xf, S2, p.k, h1, hc);  // tangent projection at X
    if constexpr (!mode_snap(MODE)) {
#pragma unroll
      for (int a = 0; a < R; ++a) dpart = fma(vcol[a], hc[a], dpart);
    } else if constexpr (FMT != QFMT_EDGES) {  // BSR MODE_QF's: <V, h1>, h1 = VQ - V_Y S
#pragma unroll
      for (int a = 0; a < R; ++a) dpart = fma(vcol[a], h1[a], dpart);
    }
    store_vec<R>(out, off, own, hc);
    if constexpr (mode_merged(MODE)) {
      // phase fence: the merged operands are loaded only after the Hessian column is out, so the HESS
      // epilogue's temporaries are dead (otherwise the scheduler hoists these loads above it and HESS_QF_M
      // needs 210 VGPRs, 2 waves / SIMD)
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      // Merged tCG iteration: the stopping test and beta of this iteration are decided with the step
      // test, before r is updated, from one-step polynomials in alpha (r' = r + alpha Hd, z' = z + alpha
      // Prec(Hd)): |r|^2, <r,Hd>, |Hd|^2, <z,r>, 2<z,Hd>, <Hd Minv, Hd> (the last two use <Prec(Hd), r> =
      // <z, Hd> and P_X self-adjoint on the tangent Hd).  z = P_X(r Minv) is formed here and in
      // k_tcg_updir (precond_col), never stored.
      double rcol[R], zc[R], mk[B];
      if constexpr (PRE_R) {
#pragma unroll
        for (int a = 0; a < R; ++a) rcol[a] = pre_r[a];
#pragma unroll
        for (int u = 0; u < B; ++u) mk[u] = pre_mk[u];
      } else {
        load_col<R, B>(args.rvec, p.j, p.k, p.ok, rcol);
        if (args.pmode != PRECON_NONE) minv_col<B>(args.Minv, p.j, p.k, p.ok, mk);
      }
      if constexpr (mode_snap(MODE)) {
        // the first tCG step only (HESS_QF_M): z_0 = -delta_0 exactly (EVAL_TCG formed delta_0 = -Prec(g)
        // with this formula), so <z_0, r_0> is bitwise EVAL_TCG's <z, g> and no Prec(r) is formed
#pragma unroll
        for (int a = 0; a < R; ++a) zc[a] = -vcol[a];
      } else {
        precond_col_mk<R, B>(Xf, mk, p.k, args.pmode, rcol, zc);
      }
      if constexpr (FMT == QFMT_EDGES && evar_v2(VAR)) {
        // Per-quantity precision (kMergedDdSlots): double-double (exact products, compensated sums) for the
        // sums whose terms cancel across poses and feed beta; plain FMA chains for the rest.  |r_j|^2 and
        // <z_j, r_j> only when no k_tcg_updir left them (args.rz_own: the first iteration).
        constexpr bool DD_RH = (kMergedDdSlots & 0x04) != 0, DD_HH = (kMergedDdSlots & 0x08) != 0,
                       DD_ZH = (kMergedDdSlots & 0x20) != 0, DD_MH = (kMergedDdSlots & 0x40) != 0;
        const bool rz = mode_snap(MODE) || args.rz_own != 0;
        const dd rh = lane_dot<DD_RH, R>(rcol, hc), hh = lane_dot<DD_HH, R>(hc, hc), zh = lane_dot<DD_ZH, R>(zc, hc);
        dd mh{0.0, 0.0};
        if (args.pmode == PRECON_NONE) {
          mh = DD_MH == DD_HH ? hh : lane_dot<DD_MH, R>(hc, hc);
        } else {
          // <Hd Minv, Hd> of the pose, column-locally: lane k adds Minv_kk |h_k|^2 and Minv_{k,k^x} <h_k, h_{k^x}>
          // for x = 1, 2, 3 (one partner column at a time, no full-pose gather)
          const int kc = p.k < B ? p.k : 0;
          const bool act = p.k < B;
          double mkk = 0.0;
#pragma unroll
          for (int u = 0; u < B; ++u) mkk = kc == u ? mk[u] : mkk;
          const dd h2 = DD_MH == DD_HH ? hh : lane_dot<DD_MH, R>(hc, hc);
          mh = act ? (DD_MH ? dd_mul_d(h2, mkk) : dd{h2.hi * mkk, 0.0}) : dd{0.0, 0.0};
          auto pair = [&](int x, const double (&hq)[R]) {
            const int pk = p.k ^ x;
            double m = 0.0;
#pragma unroll
            for (int u = 0; u < B; ++u) m = pk == u ? mk[u] : m;  // Minv_{pk, k} = column k's entry pk
            if (pk >= B || !act) m = 0.0;
            const dd t = lane_dot<DD_MH, R>(hc, hq);
            mh = DD_MH ? dd_add(mh, dd_mul_d(t, m)) : dd{fma(t.hi, m, mh.hi), 0.0};
          };
          double hq[R];
#pragma unroll
          for (int a = 0; a < R; ++a) hq[a] = dpp_f64<0xB1>(hc[a]);  // quad_perm [1,0,3,2]: partner k^1
          pair(1, hq);
#pragma unroll
          for (int a = 0; a < R; ++a) hq[a] = dpp_f64<0x4E>(hc[a]);  // [2,3,0,1]: k^2
          pair(2, hq);
#pragma unroll
          for (int a = 0; a < R; ++a) hq[a] = dpp_f64<0x1B>(hc[a]);  // [3,2,1,0]: k^3
          pair(3, hq);
        }
        const dd zero{0.0, 0.0};
        const dd zh2 = own ? (DD_ZH ? dd{2.0 * zh.hi, 2.0 * zh.lo} : dd{2.0 * zh.hi, 0.0}) : zero;
        if (rz) {
          const dd rr = lane_dot<true, R>(rcol, rcol), zr = lane_dot<true, R>(zc, rcol);
          // double-double items first (one per wave), then the plain ones
          constexpr int sl[6] = {1, 4, 5, 6, 3, 2};
          constexpr bool isdd[6] = {true, true, DD_ZH, DD_MH, DD_HH, DD_RH};
          const dd v[6] = {own ? rr : zero, own ? zr : zero, zh2, own ? mh : zero, own ? hh : zero, own ? rh : zero};
          block_partials_mixed<6>(own ? dpart : 0.0, v, sl, isdd, c.partials, p.tile, args.fin_mode == 2,
                                  red_scratch);
        } else {  // slots 1 and 4 are not read (FinalizeArgs::rz_pc)
          constexpr int sl[4] = {5, 6, 3, 2};
          constexpr bool isdd[4] = {DD_ZH, DD_MH, DD_HH, DD_RH};
          const dd v[4] = {zh2, own ? mh : zero, own ? hh : zero, own ? rh : zero};
          block_partials_mixed<4>(own ? dpart : 0.0, v, sl, isdd, c.partials, p.tile, args.fin_mode == 2,
                                  red_scratch);
        }
      } else {
      // double-double partials (exact products, compensated sums): the stopping test combines them as
      // polynomials in alpha whose terms cancel by the residual drop (merged_stop_test)
      // |r_j|^2 and <z_j, r_j> only when no k_tcg_updir left them (args.rz_own: the first iteration)
      // <r, Hd> enters only |r'|^2, i.e. the stopping test, whose bar is relative to |r_0| (a plain sum is exact
      // enough there); <z', r'> (beta, which steers the next direction) keeps every term exact
      DotAcc rr_, hh_, zr_, zh_;
      double rh_p = 0.0;
      const bool rz = mode_snap(MODE) || args.rz_own != 0;  // (the first iteration's kernel: always)
#pragma unroll
      for (int a = 0; a < R; ++a) {
        rh_p = fma(rcol[a], hc[a], rh_p);
        hh_.add(hc[a], hc[a]);
        zh_.add(zc[a], hc[a]);
      }
      if (rz) {
#pragma unroll
        for (int a = 0; a < R; ++a) {
          rr_.add(rcol[a], rcol[a]);
          zr_.add(zc[a], rcol[a]);
        }
      }
      const dd rr = rr_.val(), rh{rh_p, 0.0}, hh = hh_.val(), zr = zr_.val(), zh = zh_.val();
      dd mh{0.0, 0.0};
      if (args.pmode == PRECON_NONE) {
        mh = hh;
      } else {
        // <Hd Minv, Hd> of the pose, column-locally: lane k adds Minv_kk |h_k|^2 and Minv_{k,k^x} <h_k, h_{k^x}>
        // for x = 1, 2, 3 (each off-diagonal pair once from either lane): one partner column at a time (no
        // full-pose gather: HESS_QF_M's registers)
        const int kc = p.k < B ? p.k : 0;
        const bool act = p.k < B;
        auto pair = [&](int x, const double (&hp)[R]) {
          const int pk = p.k ^ x;
          double m = 0.0;
#pragma unroll
          for (int u = 0; u < B; ++u) m = pk == u ? mk[u] : m;  // Minv_{pk, k} = column k's entry pk
          if (pk >= B || !act) m = 0.0;
          DotAcc t;
#pragma unroll
          for (int a = 0; a < R; ++a) t.add(hc[a], hp[a]);
          mh = kMergedDd ? dd_add(mh, dd_mul_d(t.val(), m)) : dd{fma(t.val().hi, m, mh.hi), 0.0};
        };
        double mkk = 0.0;
#pragma unroll
        for (int u = 0; u < B; ++u) mkk = kc == u ? mk[u] : mkk;
        mh = act ? (kMergedDd ? dd_mul_d(hh, mkk) : dd{hh.hi * mkk, 0.0}) : dd{0.0, 0.0};
        double hp[R];
#pragma unroll
        for (int a = 0; a < R; ++a) hp[a] = dpp_f64<0xB1>(hc[a]);  // quad_perm [1,0,3,2]: partner k^1
        pair(1, hp);
#pragma unroll
        for (int a = 0; a < R; ++a) hp[a] = dpp_f64<0x4E>(hc[a]);  // [2,3,0,1]: k^2
        pair(2, hp);
#pragma unroll
        for (int a = 0; a < R; ++a) hp[a] = dpp_f64<0x1B>(hc[a]);  // [3,2,1,0]: k^3
        pair(3, hp);
      }
      const dd zero{0.0, 0.0};
      dd parts[6] = {own ? rr : zero, own ? rh : zero, own ? hh : zero, own ? zr : zero,
                     own ? dd{2.0 * zh.hi, 2.0 * zh.lo} : zero, own ? mh : zero};
      if constexpr (kMergedDd) {
        if (red_scratch != nullptr) {
          if (rz) {
            block_partials_dd_lds<6>(own ? dpart : 0.0, parts, kSlots123456, c.partials, p.tile, args.fin_mode == 2,
                                     red_scratch);
          } else {  // slots 1 and 4 are not read (FinalizeArgs::rz_pc)
            dd p4[4] = {parts[1], parts[2], parts[4], parts[5]};
            block_partials_dd_lds<4>(own ? dpart : 0.0, p4, kSlots2356, c.partials, p.tile, args.fin_mode == 2,
                                     red_scratch);
          }
        } else if (rz) {
          block_partials_dd<6>(own ? dpart : 0.0, parts, c.partials, p.tile, args.fin_mode == 2);
        } else {
          dd p4[4] = {parts[1], parts[2], parts[4], parts[5]};
          block_partials_dd_at<4>(own ? dpart : 0.0, p4, kSlots2356, c.partials, p.tile, args.fin_mode == 2);
        }
      } else {  // plain sums, low parts written as zero (the finalize reads the same layout)
        double pl[13] = {own ? dpart : 0.0};
#pragma unroll
        for (int q = 0; q < 6; ++q) pl[1 + q] = parts[q].hi;
        block_partials_lo0<6>(pl, c.partials, p.tile, args.fin_mode == 2);
      }
      }  // v1 partials
    } else {
      double parts[1] = {own ? dpart : 0.0};
      block_partials<1>(parts, c.partials, p.tile, args.fin_mode == 2);
    }
  }
  if constexpr (spmm_fusable(MODE)) spmm_arrive(args, p.agent);
}

// Everything below k_spmm except its mode instantiations is compiled once (the TU without
// DPGO_SPMM_TU); the SpMM modes are instantiated in parallel TUs (kernels.hip -DDPGO_SPMM_TU=1..5).
#ifndef DPGO_SPMM_TU

// ------------------------------------------------------------------------------------------
// Block-Jacobi preconditioner applied to a full pose: z = P_X(v (Q_jj + 0.1 I)^-1)
// (block-diagonal stand-in for src/QuadraticProblem.cpp:75-87).
// Minv stored per pose as its packed upper triangle (diag_width doubles, like Q_jj): the inverse of
// the symmetric Q_jj + 0.1 I is symmetric, so 80 instead of 128 bytes per pose (d = 3) are read.
// ------------------------------------------------------------------------------------------
template <int R, int B>
__device__ __forceinline__ void precond_pose(const double (&Xf)[R][B], const double* __restrict__ Minv,
                                             long j, bool ok, int mode, const double (&v)[R][B],
                                             double (&z)[R][B]) {
  if (mode == PRECON_NONE) {
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int cc = 0; cc < B; ++cc) z[a][cc] = v[a][cc];
    return;
  }
  double M[B][B];
#pragma unroll
  for (int u = 0; u < B; ++u)
#pragma unroll
    for (int w = 0; w < B; ++w) M[u][w] = ok ? Minv[j * diag_width(B - 1) + minv_index<B>(u, w)] : 0.0;
#pragma unroll
  for (int a = 0; a < R; ++a)
#pragma unroll
    for (int cc = 0; cc < B; ++cc) {
      double s = 0.0;
#pragma unroll
      for (int u = 0; u < B; ++u) s = fma(v[a][u], M[u][cc], s);
      z[a][cc] = s;
    }
  tangent_project_pose<R, B>(Xf, z);
}

// tCG start (A.4): eta = 0, Heta = 0, r = grad, z = Prec(r), delta = -z; partials <z,r>, |r|^2.
// eta, Heta and r are not materialised here: the first k_tcg_update reads r from grad and treats
// eta / Heta as zero, so this pass only writes delta.
template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_tcg_init(LaunchCtx c, const double* __restrict__ X,
                                                       const double* __restrict__ Minv, int pmode,
                                                       const double* __restrict__ g,
                                                       double* __restrict__ delta) {
  const PoseLane p = pose_lane<B>(c);
  if (tile_skipped(c, p.agent)) return;
  const bool own = p.ok && p.k < B;
  const long off = p.j * (R * B) + p.k * R;
  double gcol[R], xcol[R];
  load_col<R, B>(g, p.j, p.k, p.ok, gcol);
  load_col<R, B>(X, p.j, p.k, p.ok, xcol);
  double Gf[R][B], Xf[R][B], Zf[R][B];
  quad_gather<R, B>(gcol, Gf);
  quad_gather<R, B>(xcol, Xf);
  precond_pose<R, B>(Xf, Minv, p.j, p.ok, pmode, Gf, Zf);
  double zc[R], dc[R];
  select_col<R, B>(Zf, p.k, zc);
  double zr = 0.0, rr = 0.0;
#pragma unroll
  for (int a = 0; a < R; ++a) {
    zr = fma(zc[a], gcol[a], zr);
    rr = fma(gcol[a], gcol[a], rr);
    dc[a] = -zc[a];
  }
  store_vec<R>(delta, off, own, dc);
  double parts[2] = {own ? zr : 0.0, own ? rr : 0.0};
  block_partials<2>(parts, c.partials, p.tile);
}

// tCG step (A.4 steps 1-3, 5 first half): eta += s delta; for a CG step (mode 0) also r += alpha Hdelta
// and z = Prec(r) with partials <z,r>, |r|^2.  Heta is never formed: the third partial <eta_old, Hdelta>
// lets OP_TCG_CHECK carry <eta, Heta> as a scalar, <eta + s delta, H(eta + s delta)> = <eta, Heta>
// + s (2 <eta, Hdelta> + s <delta, Hdelta>) (H self-adjoint on the tangent space), which is all the rho
// test reads of it (src/QuadraticOptimizer.cpp via ROPTLIB RTRNewton).
template <int R, int B, bool FUSED>
__global__ __launch_bounds__(kThreads) void k_tcg_update(LaunchCtx c, const double* __restrict__ X,
                                                         const double* __restrict__ Minv, int pmode,
                                                         const double* __restrict__ delta,
                                                         const double* __restrict__ Hdelta,
                                                         double* __restrict__ eta, const double* r_in, double* r,
                                                         double* __restrict__ z, int first, FinalizeArgs fin,
                                                         int* arrive) {
  const PoseLane p = pose_lane<B>(c);
  const bool own = p.ok && p.k < B;
  const long off = p.j * (R * B) + p.k * R;
  int mode;
  double step;
  double dcol[R], hcol[R], ecol[R];
  __shared__ AgentState sh;  // FUSED: this block's copy of the agent's state after the step test
  if constexpr (FUSED) {
    // The step test (OP_TCG_STEP on the HESS partials) runs here instead of a k_finalize launch.  Only
    // an agent still in tCG can take a step: its operands are requested before the test so their
    // latency overlaps it.
    const bool pre = fin.state[p.agent].tcg_active != 0;
#pragma unroll
    for (int a = 0; a < R; ++a) dcol[a] = hcol[a] = ecol[a] = 0.0;
    if (pre) {
      load_col<R, B>(delta, p.j, p.k, p.ok, dcol);
      load_col<R, B>(Hdelta, p.j, p.k, p.ok, hcol);
      if (!first) load_col<R, B>(eta, p.j, p.k, p.ok, ecol);
    }
    prologue_finalize<1>(fin, p.agent, arrive, sh);
    if (sh.tcg_mode == 2 || sh.eta_implicit) {
      finalize_arrive(fin, p.agent, arrive, sh);
      return;
    }
    mode = sh.tcg_mode;
    step = sh.step;
  } else {
    if (tile_skipped(c, p.agent)) return;  // FLAG_TCG_MODE: skips mode 2
    const AgentState& st = c.state[p.agent];
    if (st.eta_implicit) return;  // first-step boundary exit: eta stays implicit (k_retract)
    mode = st.tcg_mode;
    step = st.step;
    load_col<R, B>(delta, p.j, p.k, p.ok, dcol);
    load_col<R, B>(Hdelta, p.j, p.k, p.ok, hcol);
    if (first) {  // eta = 0 at the start of tCG
#pragma unroll
      for (int a = 0; a < R; ++a) ecol[a] = 0.0;
    } else {
      load_col<R, B>(eta, p.j, p.k, p.ok, ecol);
    }
  }
  double eh = 0.0;  // <eta_old, Hdelta> (eta_old = 0 on the first step)
#pragma unroll
  for (int a = 0; a < R; ++a) eh = fma(ecol[a], hcol[a], eh);
#pragma unroll
  for (int a = 0; a < R; ++a) ecol[a] = fma(step, dcol[a], ecol[a]);
  store_vec<R>(eta, off, own, ecol);
  double zr = 0.0, rr = 0.0;
  if (mode == 0) {  // a boundary step ends tCG: r / z untouched (uniform per agent)
    double rcol[R], xcol[R];
    load_col<R, B>(r_in, p.j, p.k, p.ok, rcol);  // r_in = grad on the first step
    load_col<R, B>(X, p.j, p.k, p.ok, xcol);
#pragma unroll
    for (int a = 0; a < R; ++a) rcol[a] = fma(step, hcol[a], rcol[a]);
    double Rf[R][B], Xf[R][B], Zf[R][B];
    quad_gather<R, B>(rcol, Rf);
    quad_gather<R, B>(xcol, Xf);
    precond_pose<R, B>(Xf, Minv, p.j, p.ok, pmode, Rf, Zf);
    double zc[R];
    select_col<R, B>(Zf, p.k, zc);
#pragma unroll
    for (int a = 0; a < R; ++a) {
      zr = fma(zc[a], rcol[a], zr);
      rr = fma(rcol[a], rcol[a], rr);
    }
    store_vec<R>(r, off, own, rcol);
    store_vec<R>(z, off, own, zc);
  }
  double parts[3] = {own ? zr : 0.0, own ? rr : 0.0, own ? eh : 0.0};
  block_partials<3>(parts, c.partials, p.tile);
  if constexpr (FUSED) finalize_arrive(fin, p.agent, arrive, sh);
}

// delta = -z + beta delta for agents whose tCG continues (A.4 step 5).  FUSED: the stopping test and
// beta (OP_TCG_CHECK on the update's partials) run here instead of a k_finalize launch.
template <int R, int B, bool FUSED>
__global__ __launch_bounds__(kThreads) void k_tcg_dir(LaunchCtx c, const double* __restrict__ z,
                                                      double* __restrict__ delta, FinalizeArgs fin, int* arrive) {
  const PoseLane p = pose_lane<B>(c);
  const bool own = p.ok && p.k < B;
  const long off = p.j * (R * B) + p.k * R;
  if constexpr (FUSED) {
    __shared__ AgentState sh;
    const bool pre = own && fin.state[p.agent].tcg_active != 0;  // only a CG step can continue
    double zc[R], dc[R];
    if (pre) {
#pragma unroll
      for (int a = 0; a < R; ++a) {
        zc[a] = z[off + a];
        dc[a] = delta[off + a];
      }
    }
    prologue_finalize<3>(fin, p.agent, arrive, sh);
    if (pre && sh.tcg_active) {
      const double beta = sh.beta;
#pragma unroll
      for (int a = 0; a < R; ++a) delta[off + a] = fma(beta, dc[a], -zc[a]);
    }
    finalize_arrive(fin, p.agent, arrive, sh);
  } else {
    if (tile_skipped(c, p.agent)) return;  // FLAG_TCG
    const double beta = c.state[p.agent].beta;
    if (!own) return;
#pragma unroll
    for (int a = 0; a < R; ++a) delta[off + a] = fma(beta, delta[off + a], -z[off + a]);
  }
}

// Merged tCG iteration, after OP_TCG_STEP_CHECK (A.4 steps 4-6 of the classic update / direction pair):
// eta += step delta with the partial <eta_old, Hdelta> (folded into <eta, Heta> by the next finalize);
// for agents whose tCG continues r += alpha Hdelta, z = P_X(r Minv) (precond_col, not stored) and
// delta = -z + beta delta.  first: eta = 0 and r_in = grad; last: tCG ends here (MAXITER), no r / delta.
template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_tcg_updir(LaunchCtx c, const double* __restrict__ X,
                                                        const double* __restrict__ Minv, int pmode,
                                                        double* __restrict__ delta, const double* __restrict__ Hdelta,
                                                        double* __restrict__ eta, const double* r_in, double* rv,
                                                        int first, int last) {
  const PoseLane p = pose_lane<B>(c);
  if (tile_skipped(c, p.agent)) return;  // FLAG_TCG_MODE: no step pending
  const AgentState& st = c.state[p.agent];
  if (st.eta_implicit) return;  // first-step boundary exit: eta stays implicit (k_retract)
  const bool own = p.ok && p.k < B;
  const long off = p.j * (R * B) + p.k * R;
  const double step = st.step;
  const bool cont = st.tcg_mode == 0 && st.tcg_active != 0 && !last;
  double dcol[R], hcol[R], ecol[R];
  load_col<R, B>(delta, p.j, p.k, p.ok, dcol);
  load_col<R, B>(Hdelta, p.j, p.k, p.ok, hcol);
  if (first) {
#pragma unroll
    for (int a = 0; a < R; ++a) ecol[a] = 0.0;
  } else {
    load_col<R, B>(eta, p.j, p.k, p.ok, ecol);
  }
  double eh = 0.0;
#pragma unroll
  for (int a = 0; a < R; ++a) eh = fma(ecol[a], hcol[a], eh);
#pragma unroll
  for (int a = 0; a < R; ++a) ecol[a] = fma(step, dcol[a], ecol[a]);
  store_vec<R>(eta, off, own, ecol);
  dd rz[2] = {{0.0, 0.0}, {0.0, 0.0}};
  if (cont) {  // uniform per agent
    constexpr int D = B - 1;
    const double beta = st.beta;
    double rcol[R], xcol[R];
    load_col<R, B>(r_in, p.j, p.k, p.ok, rcol);
    load_col_y<R, B>(X, p.j, p.k, p.ok, xcol);  // only X's Y block enters Prec
#pragma unroll
    for (int a = 0; a < R; ++a) rcol[a] = fma(step, hcol[a], rcol[a]);
    double Yx[R][D], zc[R], dn[R];
    quad_gather_y<R, D>(xcol, Yx);
    precond_col<R, B>(Yx, Minv, p.j, p.k, p.ok, pmode, rcol, zc);
#pragma unroll
    for (int a = 0; a < R; ++a) dn[a] = fma(beta, dcol[a], -zc[a]);
    store_vec<R>(rv, off, own, rcol);
    store_vec<R>(delta, off, own, dn);
    if (own) {  // |r_{j+1}|^2, <z_{j+1}, r_{j+1}> for the next iteration's stopping test (FinalizeArgs::rz_pc)
#pragma unroll
      for (int a = 0; a < R; ++a) {
        rz[0] = dd_fma(rz[0], rcol[a], rcol[a]);
        rz[1] = dd_fma(rz[1], zc[a], rcol[a]);
      }
    }
  }
  block_partials_dd<2>(own ? eh : 0.0, rz, c.partials, p.tile);
}

// x2 = R_x1(scale * eta) (QF retraction, A.2) with partials <g,eta> and, when HV is given, <eta,HV>
// (the tCG carries <eta, Heta> as a scalar and passes none).  For agents whose eta is implicit
// (AgentState::eta_implicit) and delta_impl is given, eta = step delta is formed here (the same fma the
// update kernel would have stored) and the dots come from OP_TCG_STEP instead.
// TAIL (merged tCG, TUNE_TAIL_FUSE): the last tCG iteration's k_tcg_updir is not launched and its step is applied
// here, for the agents it would have visited (a step pending: tcg_mode != 2 and eta not implicit, the state after
// the same finalize): V holds eta_old, eta = fma(step, delta, eta_old) stays in registers and is not stored, and
// the <eta_old, Hdelta> partial goes to tail.peh in k_tcg_updir's layout -- the same fma sequences on the same
// operands.  Agents that stopped earlier read their final eta from V as before and leave tail.peh alone.
template <int R, int B, bool TAIL>
__global__ __launch_bounds__(kThreads) void k_retract(LaunchCtx c, const double* __restrict__ X,
                                                      const double* __restrict__ V, double scale,
                                                      double* __restrict__ out,
                                                      const double* __restrict__ g,
                                                      const double* __restrict__ HV,
                                                      const double* __restrict__ delta_impl,
                                                      const double* __restrict__ status_ref, RetractTail tail) {
  constexpr int D = B - 1;
  const PoseLane p = pose_lane<B>(c);
  if (tile_skipped(c, p.agent)) return;
  const bool own = p.ok && p.k < B;
  const long off = p.j * (R * B) + p.k * R;
  const bool impl = delta_impl != nullptr && c.state != nullptr && c.state[p.agent].eta_implicit;
  double xcol[R], vcol[R];
  load_col<R, B>(X, p.j, p.k, p.ok, xcol);
  bool pend = false;  // uniform per tile
  if constexpr (TAIL) pend = c.state[p.agent].tcg_mode != 2 && !c.state[p.agent].eta_implicit;
  if (TAIL && pend) {
    const double step = c.state[p.agent].step;
    double dcol[R], hcol[R];
    load_col<R, B>(tail.delta, p.j, p.k, p.ok, dcol);
    load_col<R, B>(tail.Hdelta, p.j, p.k, p.ok, hcol);
    if (tail.first) {  // eta = 0 at the start of tCG
#pragma unroll
      for (int a = 0; a < R; ++a) vcol[a] = 0.0;
    } else {
      load_col<R, B>(V, p.j, p.k, p.ok, vcol);
    }
    double eh = 0.0;  // <eta_old, Hdelta>
#pragma unroll
    for (int a = 0; a < R; ++a) eh = fma(vcol[a], hcol[a], eh);
#pragma unroll
    for (int a = 0; a < R; ++a) vcol[a] = fma(step, dcol[a], vcol[a]);
    dd rz[2] = {{0.0, 0.0}, {0.0, 0.0}};  // no next iteration: as k_tcg_updir's last
    block_partials_dd<2>(own ? eh : 0.0, rz, tail.peh, p.tile);
  } else if (impl) {
    const double step = c.state[p.agent].step;
    load_col<R, B>(delta_impl, p.j, p.k, p.ok, vcol);
#pragma unroll
    for (int a = 0; a < R; ++a) vcol[a] = fma(step, vcol[a], 0.0);
  } else {
    load_col<R, B>(V, p.j, p.k, p.ok, vcol);
  }
  double mcol[R];
#pragma unroll
  for (int a = 0; a < R; ++a) mcol[a] = fma(scale, vcol[a], xcol[a]);
  double Mf[R][B];
  quad_gather<R, B>(mcol, Mf);
  qf_inplace<R, D>(Mf);
  double oc[R];
  select_col<R, B>(Mf, p.k, oc);
  store_vec<R>(out, off, own, oc);
  if (g != nullptr) {
    double ge = 0.0, eh = 0.0;
    if (!impl) {
      double gcol[R];
      load_col<R, B>(g, p.j, p.k, p.ok, gcol);
#pragma unroll
      for (int a = 0; a < R; ++a) ge = fma(gcol[a], vcol[a], ge);
      if (HV != nullptr) {
        double hcol[R];
        load_col<R, B>(HV, p.j, p.k, p.ok, hcol);
#pragma unroll
        for (int a = 0; a < R; ++a) eh = fma(vcol[a], hcol[a], eh);
      }
    }
    if (status_ref != nullptr) {  // |out - ref|^2, |X - ref|^2: the status of either outcome (k_sqdiff's sums)
      double d2 = 0.0, d1 = 0.0;
      if (own) {
#pragma unroll
        for (int a = 0; a < R; ++a) {
          const double rf = status_ref[off + a];
          const double e2 = oc[a] - rf, e1 = xcol[a] - rf;
          d2 = fma(e2, e2, d2);
          d1 = fma(e1, e1, d1);
        }
      }
      double parts[4] = {own ? ge : 0.0, own ? eh : 0.0, d2, d1};
      block_partials<4>(parts, c.partials, p.tile);
    } else {
      double parts[2] = {own ? ge : 0.0, own ? eh : 0.0};
      block_partials<2>(parts, c.partials, p.tile);
    }
  }
}

// out = P_X(V) (ROPTLIB ProductManifold::Projection, A.2)
template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_tangent(LaunchCtx c, const double* __restrict__ X,
                                                      const double* __restrict__ V,
                                                      double* __restrict__ out) {
  const PoseLane p = pose_lane<B>(c);
  if (tile_skipped(c, p.agent)) return;
  const bool own = p.ok && p.k < B;
  const long off = p.j * (R * B) + p.k * R;
  double xcol[R], vcol[R];
  load_col<R, B>(X, p.j, p.k, p.ok, xcol);
  load_col<R, B>(V, p.j, p.k, p.ok, vcol);
  double Xf[R][B], Vf[R][B];
  quad_gather<R, B>(xcol, Xf);
  quad_gather<R, B>(vcol, Vf);
  tangent_project_pose<R, B>(Xf, Vf);
  double oc[R];
  select_col<R, B>(Vf, p.k, oc);
  store_vec<R>(out, off, own, oc);
}

// out = P_X(V Minv) (QuadraticProblem::PreConditioner, block-Jacobi)
template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_precond(LaunchCtx c, const double* __restrict__ X,
                                                      const double* __restrict__ Minv, int pmode,
                                                      const double* __restrict__ V,
                                                      double* __restrict__ out) {
  const PoseLane p = pose_lane<B>(c);
  if (tile_skipped(c, p.agent)) return;
  const bool own = p.ok && p.k < B;
  const long off = p.j * (R * B) + p.k * R;
  double xcol[R], vcol[R];
  load_col<R, B>(X, p.j, p.k, p.ok, xcol);
  load_col<R, B>(V, p.j, p.k, p.ok, vcol);
  double Xf[R][B], Vf[R][B], Zf[R][B];
  quad_gather<R, B>(xcol, Xf);
  quad_gather<R, B>(vcol, Vf);
  precond_pose<R, B>(Xf, Minv, p.j, p.ok, pmode, Vf, Zf);
  double oc[R];
  select_col<R, B>(Zf, p.k, oc);
  store_vec<R>(out, off, own, oc);
}

// a0 A + b0 B as one rounded product and one fma, in this order: the fused passes (NEXT below and in k_polar_vnext)
// form a later launch's combination ahead of time and must round as that launch does
__device__ __forceinline__ double comb_xv(double a0, double av, double b0, double bv) { return fma(b0, bv, a0 * av); }

// out = LiftedSEManifold::project(ca A + cb B) (or A + cb (B - C)) with per-agent (or scalar)
// coefficients.  A tile's 64 poses are one contiguous span of 64 r b doubles: the combination is
// elementwise, so it is formed while the span streams through LDS with fully coalesced loads; then
// thread t polar-projects pose t from LDS (row stride r b + 1 doubles: conflict-free b64 reads) and
// the span streams back out coalesced (optionally to a second destination).
// (src/manifold/LiftedSEManifold.cpp:34-45; Nesterov updateY/updateV src/PGOAgent.cpp:1075-1091)
// NEXT (TUNE_NEXT_Y; the a0 A + b0 B form only): two more outputs of the same pass, ynext = project(sa2 out + sb2 B)
// and xprev = out -- what a second launch with A = out and xcopy = xprev would compute, by the same comb_xv.
template <int R, int B, bool NEXT>
__global__ __launch_bounds__(64) void k_polar_comb(LaunchCtx c, const double* __restrict__ A,
                                                   const double* __restrict__ Bv,
                                                   const double* __restrict__ ca,
                                                   const double* __restrict__ cb,
                                                   double* __restrict__ out,
                                                   const double* __restrict__ Cv, double sa,
                                                   double sb, double* __restrict__ out2,
                                                   double* __restrict__ xcopy, double sa2, double sb2,
                                                   double* __restrict__ ynext, double* __restrict__ xprev) {
  constexpr int D = B - 1;
  constexpr int PW = R * B;
  constexpr int PS = PW + 1;
  __shared__ double sm[64 * PS];
  const int tile = launch_tile(c);
  const int agent = c.tile_agent[tile];
  if (tile_skipped(c, agent)) return;
  const int count = c.tile_count[tile];
  const long base = static_cast<long>(c.tile_start[tile]) * PW;
  const int total = count * PW;
  const double a0 = ca ? ca[agent] : sa;
  const double b0 = cb ? cb[agent] : sb;
  const int t = static_cast<int>(threadIdx.x);
  // elementwise combination (updateV: V + gamma (X - Y), src/PGOAgent.cpp:1086-1091; updateY:
  // (1 - alpha) X + alpha V, :1077-1084; plain project: a0 A)
  auto comb = [&](double av, double bv, double cv) {
    return Cv != nullptr ? av + b0 * (bv - cv) : (Bv != nullptr ? comb_xv(a0, av, b0, bv) : a0 * av);
  };
  auto project_span = [&]() {
    if (t < count) {
      double M[R][B];
      double* ps = sm + t * PS;
#pragma unroll
      for (int cc = 0; cc < D; ++cc)
#pragma unroll
        for (int a = 0; a < R; ++a) M[a][cc] = ps[cc * R + a];
#pragma unroll
      for (int a = 0; a < R; ++a) M[a][D] = 0.0;
      polar_fast<R, D>(M);  // the translation column passes through unchanged (stays in LDS)
#pragma unroll
      for (int cc = 0; cc < D; ++cc)
#pragma unroll
        for (int a = 0; a < R; ++a) ps[cc * R + a] = M[a][cc];
    }
  };
  constexpr bool kVec = PW % 2 == 0;  // 16-byte chunks need an even pose width (aligned spans)
  if (kVec && count == 64) {
    // full tile: 64 r b doubles = 16-byte chunks, all loads in flight before the LDS writes
    constexpr int NV = PW / 2;  // 16-byte chunks per lane
    const double2* A2 = reinterpret_cast<const double2*>(A + base);
    const double2* B2 = reinterpret_cast<const double2*>((Bv ? Bv : A) + base);
    const double2* C2 = reinterpret_cast<const double2*>((Cv ? Cv : A) + base);
    double2 va[NV], vb[NV], vc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) va[i] = A2[t + 64 * i];
    if (xcopy != nullptr) {  // XPrev = X (the A operand), written from the registers just loaded
      double2* XC = reinterpret_cast<double2*>(xcopy + base);
#pragma unroll
      for (int i = 0; i < NV; ++i) XC[t + 64 * i] = va[i];
    }
    if (Bv != nullptr) {
#pragma unroll
      for (int i = 0; i < NV; ++i) vb[i] = B2[t + 64 * i];
    }
    if (Cv != nullptr) {
#pragma unroll
      for (int i = 0; i < NV; ++i) vc[i] = C2[t + 64 * i];
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int x = 2 * (t + 64 * i);  // PW is even: a chunk never straddles two poses
      double* dst = sm + (x / PW) * PS + x % PW;
      dst[0] = comb(va[i].x, Bv ? vb[i].x : 0.0, Cv ? vc[i].x : 0.0);
      dst[1] = comb(va[i].y, Bv ? vb[i].y : 0.0, Cv ? vc[i].y : 0.0);
    }
  } else {
    for (int x = t; x < total; x += 64) {
      const double av = A[base + x];
      if (xcopy != nullptr) xcopy[base + x] = av;
      sm[(x / PW) * PS + x % PW] = comb(av, Bv ? Bv[base + x] : 0.0, Cv ? Cv[base + x] : 0.0);
    }
  }
  __syncthreads();
  project_span();
  __syncthreads();
  if (kVec && count == 64) {
    constexpr int NV = PW / 2;
    double2 vo[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int x = 2 * (t + 64 * i);
      const double* src = sm + (x / PW) * PS + x % PW;
      vo[i] = make_double2(src[0], src[1]);
    }
    double2* O2 = reinterpret_cast<double2*>(out + base);
#pragma unroll
    for (int i = 0; i < NV; ++i) O2[t + 64 * i] = vo[i];
    if (out2 != nullptr) {  // second copy (Nesterov iterate(false): X = Y)
      double2* P2 = reinterpret_cast<double2*>(out2 + base);
#pragma unroll
      for (int i = 0; i < NV; ++i) P2[t + 64 * i] = vo[i];
    }
    if constexpr (NEXT) {
      // B again (the lines this block loaded above); each lane rewrites exactly the LDS words it read
      const double2* B2 = reinterpret_cast<const double2*>(Bv + base);
      if (xprev != nullptr) {
        double2* XP = reinterpret_cast<double2*>(xprev + base);
#pragma unroll
        for (int i = 0; i < NV; ++i) XP[t + 64 * i] = vo[i];
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int x = 2 * (t + 64 * i);
        double* dst = sm + (x / PW) * PS + x % PW;
        const double2 bv = B2[t + 64 * i];
        dst[0] = comb_xv(sa2, vo[i].x, sb2, bv.x);
        dst[1] = comb_xv(sa2, vo[i].y, sb2, bv.y);
      }
      __syncthreads();
      project_span();
      __syncthreads();
      double2* Y2 = reinterpret_cast<double2*>(ynext + base);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int x = 2 * (t + 64 * i);
        const double* src = sm + (x / PW) * PS + x % PW;
        Y2[t + 64 * i] = make_double2(src[0], src[1]);
      }
    }
  } else {
    for (int x = t; x < total; x += 64) {
      double* src = sm + (x / PW) * PS + x % PW;
      const double v = *src;
      out[base + x] = v;
      if (out2 != nullptr) out2[base + x] = v;
      if constexpr (NEXT) {
        if (xprev != nullptr) xprev[base + x] = v;
        *src = comb_xv(sa2, v, sb2, Bv[base + x]);
      }
    }
    if constexpr (NEXT) {
      __syncthreads();
      project_span();
      __syncthreads();
      for (int x = t; x < total; x += 64) ynext[base + x] = sm[(x / PW) * PS + x % PW];
    }
  }
}

// SE(d) rounding of lifted poses in the frame of an anchor pose A = [Y_a | p_a] (PGOAgent::getTrajectoryInGlobalFrame,
// src/PGOAgent.cpp:500-519; anchor = pose 0 of X: getTrajectoryInLocalFrame, :481-498): per pose j
//   R_j = projectToRotationGroup(Y_a^T Y_j),   t_j = Y_a^T p_j - Y_a^T p_a,
// written as [R_j | t_j], d x (d+1) column-major, pose-major.  A streaming pass with no tile set and no agent state:
// block k takes poses [64 k, 64 k + 64) -- one contiguous span of 64 r b doubles in, 64 d b doubles out.  As in
// k_polar_comb the span streams through LDS with coalesced loads (16-byte chunks on a full block when the span is
// aligned), thread t rounds pose t from LDS (row stride r b + 1 doubles: conflict-free b64 reads), and the rounded
// poses stream back out of the same LDS (row stride d b + 1) coalesced.
template <int R, int B>
__global__ __launch_bounds__(64) void k_round_se(long n, const double* __restrict__ X,
                                                 const double* __restrict__ anchor, double* __restrict__ T) {
  constexpr int D = B - 1;
  constexpr int PW = R * B, PS = PW + 1;
  constexpr int OW = D * B, OS = OW + 1;
  static_assert(OS <= PS, "the rounded poses reuse the staged span's LDS");
  __shared__ double sm[64 * PS];
  const int t = static_cast<int>(threadIdx.x);
  const long first = static_cast<long>(blockIdx.x) * 64;
  if (first >= n) return;
  const int count = n - first < 64 ? static_cast<int>(n - first) : 64;
  const double* src = X + first * PW;
  double* dst = T + first * OW;
  const int total = count * PW;
  const bool full = count == 64;
  if (PW % 2 == 0 && full && (reinterpret_cast<unsigned long>(src) & 15) == 0) {
    constexpr int NV = PW / 2;  // 16-byte chunks per lane (PW even: a chunk never straddles two poses)
    const double2* S2 = reinterpret_cast<const double2*>(src);
    double2 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = S2[t + 64 * i];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int x = 2 * (t + 64 * i);
      double* q = sm + (x / PW) * PS + x % PW;
      q[0] = v[i].x;
      q[1] = v[i].y;
    }
  } else {
    for (int x = t; x < total; x += 64) sm[(x / PW) * PS + x % PW] = src[x];
  }
  __syncthreads();
  const bool own = t < count;
  double W[D][D], tv[D];
  if (own) {
    const double* ps = sm + t * PS;
    // the anchor is read at block-uniform addresses: r b doubles, once per wave
    double ta[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
#pragma unroll
      for (int c = 0; c < D; ++c) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) s = fma(anchor[a * R + k], ps[c * R + k], s);
        W[a][c] = s;
      }
      double sp = 0.0, sa = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        sp = fma(anchor[a * R + k], ps[D * R + k], sp);
        sa = fma(anchor[a * R + k], anchor[D * R + k], sa);
      }
      tv[a] = sp;
      ta[a] = sa;
    }
#pragma unroll
    for (int a = 0; a < D; ++a) tv[a] -= ta[a];
  }
  __syncthreads();  // every pose of the span is in registers: its LDS now takes the rounded poses
  if (own) {
    rotation_project<D>(W);
    double* po = sm + t * OS;
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
      for (int a = 0; a < D; ++a) po[c * D + a] = W[a][c];
#pragma unroll
    for (int a = 0; a < D; ++a) po[D * D + a] = tv[a];
  }
  __syncthreads();
  if (full && (reinterpret_cast<unsigned long>(dst) & 15) == 0) {
    constexpr int NO = OW / 2;  // OW = d (d + 1) is even
    double2* O2 = reinterpret_cast<double2*>(dst);
#pragma unroll
    for (int i = 0; i < NO; ++i) {
      const int x = 2 * (t + 64 * i);
      const double* q = sm + (x / OW) * OS + x % OW;
      O2[t + 64 * i] = make_double2(q[0], q[1]);
    }
  } else {
    const int total_out = count * OW;
    for (int x = t; x < total_out; x += 64) dst[x] = sm[(x / OW) * OS + x % OW];
  }
}

// Rank staircase: lift the n poses X (R x B each) to rank R + 1 and move along the certificate's negative-curvature
// direction, X+ = Retr_[X; 0](alpha [0; v^T]) (build-defined; SE-Sync's saddle escape):
// per pose j with v_j = (v_Y (D), v_p) the pose's slice of the (D+1) n vector v,
//   out_j = [qf([Y_j; alpha v_Y^T]) | (p_j; alpha v_p)],   (R + 1) x B column-major,
// qf being k_retract's (qf_inplace).  v == nullptr is the plain lift [X; 0]: a relayout, no arithmetic on X's entries.
// k_round_se's shape: block k takes poses [64 k, 64 k + 64); the R B-wide span and the B-wide span of v stream
// through LDS coalesced (16-byte chunks where the span width is even, the block full and the span aligned, 8-byte
// otherwise), thread t works on pose t, and the (R + 1) B-wide result streams out of the same LDS.  Row strides are
// the span widths made odd (conflict-free b64 reads), at most (R + 1) B + 1 doubles.
template <int R, int B>
__global__ __launch_bounds__(64) void k_lift_escape(long n, const double* __restrict__ X,
                                                    const double* __restrict__ v, double alpha,
                                                    double* __restrict__ out) {
  constexpr int D = B - 1;
  constexpr int PW = R * B, PS = PW | 1;
  constexpr int OW = (R + 1) * B, OS = OW | 1;
  constexpr int VS = B | 1;
  static_assert(PS <= OS, "the lifted poses reuse the staged span's LDS");
  __shared__ double sm[64 * OS];
  __shared__ double sv[64 * VS];
  const int t = static_cast<int>(threadIdx.x);
  const long first = static_cast<long>(blockIdx.x) * 64;
  if (first >= n) return;
  const int count = n - first < 64 ? static_cast<int>(n - first) : 64;
  const double* src = X + first * PW;
  double* dst = out + first * OW;
  const bool full = count == 64;
  if (PW % 2 == 0 && full && (reinterpret_cast<unsigned long>(src) & 15) == 0) {
    constexpr int NV = PW / 2;  // 16-byte chunks per lane (PW even: a chunk never straddles two poses)
    const double2* S2 = reinterpret_cast<const double2*>(src);
    double2 w[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) w[i] = S2[t + 64 * i];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int x = 2 * (t + 64 * i);
      double* q = sm + (x / PW) * PS + x % PW;
      q[0] = w[i].x;
      q[1] = w[i].y;
    }
  } else {
    const int total = count * PW;
    for (int x = t; x < total; x += 64) sm[(x / PW) * PS + x % PW] = src[x];
  }
  if (v != nullptr) {
    const double* vsrc = v + first * B;
    if (B % 2 == 0 && full && (reinterpret_cast<unsigned long>(vsrc) & 15) == 0) {
      constexpr int NB = B / 2;
      const double2* V2 = reinterpret_cast<const double2*>(vsrc);
      double2 w[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) w[i] = V2[t + 64 * i];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int x = 2 * (t + 64 * i);
        double* q = sv + (x / B) * VS + x % B;
        q[0] = w[i].x;
        q[1] = w[i].y;
      }
    } else {
      const int total_v = count * B;
      for (int x = t; x < total_v; x += 64) sv[(x / B) * VS + x % B] = vsrc[x];
    }
  }
  __syncthreads();
  const bool own = t < count;
  double M[R + 1][B];
  if (own) {
    const double* ps = sm + t * PS;
#pragma unroll
    for (int c = 0; c < B; ++c) {
#pragma unroll
      for (int a = 0; a < R; ++a) M[a][c] = ps[c * R + a];
      M[R][c] = 0.0;
    }
    if (v != nullptr) {  // block-uniform
#pragma unroll
      for (int c = 0; c < B; ++c) M[R][c] = alpha * sv[t * VS + c];
      qf_inplace<R + 1, D>(M);
    }
  }
  __syncthreads();  // every pose of the span is in registers: its LDS now takes the lifted poses
  if (own) {
    double* po = sm + t * OS;
#pragma unroll
    for (int c = 0; c < B; ++c)
#pragma unroll
      for (int a = 0; a < R + 1; ++a) po[c * (R + 1) + a] = M[a][c];
  }
  __syncthreads();
  if (OW % 2 == 0 && full && (reinterpret_cast<unsigned long>(dst) & 15) == 0) {
    constexpr int NO = OW / 2;
    double2* O2 = reinterpret_cast<double2*>(dst);
#pragma unroll
    for (int i = 0; i < NO; ++i) {
      const int x = 2 * (t + 64 * i);
      const double* q = sm + (x / OW) * OS + x % OW;
      O2[t + 64 * i] = make_double2(q[0], q[1]);
    }
  } else {
    const int total_out = count * OW;
    for (int x = t; x < total_out; x += 64) dst[x] = sm[(x / OW) * OS + x % OW];
  }
}

// The inverse of k_round_se: lift SE(d) poses to rank R, each composed with a frame first (the engine's read-in of a
// per-agent initialisation or a warm start; PGOAgent::initializeInGlobalFrame's T_world2_world1 T then X = YLift T,
// src/PGOAgent.cpp:402-415).  Per pose j with T_j = [R_j | t_j] (D x B column-major) and F = frames[frame_of[j]]
// ([F_R | F_t], D x B column-major):
//   W = [F_R R_j | F_R t_j + F_t],   out_j = YLift W   (R x B column-major);
// frames == nullptr (block-uniform): W = T_j, T's entries only pass through the YLift product.  k_round_se's shape:
// block k takes poses [64 k, 64 k + 64); the D B-wide span streams through LDS coalesced (16-byte chunks where the
// span width is even, the block full and the span aligned, 8-byte otherwise), thread t works on pose t, and the R B-wide
// result streams out of the same LDS.  Row strides are the span widths made odd (conflict-free b64 reads).  The frame
// table is a few entries read at (mostly wave-uniform) addresses: agent-contiguous spans hit one entry.
template <int R, int B>
__global__ __launch_bounds__(64) void k_frame_lift(long n, const double* __restrict__ T, FrameLiftY yl,
                                                   const double* __restrict__ frames,
                                                   const int* __restrict__ frame_of, double* __restrict__ out) {
  constexpr int D = B - 1;
  constexpr int PW = D * B, PS = PW | 1;  // D (D + 1) is even
  constexpr int OW = R * B, OS = OW | 1;
  static_assert(PS <= OS, "the lifted poses reuse the staged span's LDS");
  __shared__ double sm[64 * OS];
  const int t = static_cast<int>(threadIdx.x);
  const long first = static_cast<long>(blockIdx.x) * 64;
  if (first >= n) return;
  const int count = n - first < 64 ? static_cast<int>(n - first) : 64;
  const double* src = T + first * PW;
  double* dst = out + first * OW;
  const bool full = count == 64;
  if (full && (reinterpret_cast<unsigned long>(src) & 15) == 0) {
    constexpr int NV = PW / 2;  // 16-byte chunks per lane (PW even: a chunk never straddles two poses)
    const double2* S2 = reinterpret_cast<const double2*>(src);
    double2 w[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) w[i] = S2[t + 64 * i];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int x = 2 * (t + 64 * i);
      double* q = sm + (x / PW) * PS + x % PW;
      q[0] = w[i].x;
      q[1] = w[i].y;
    }
  } else {
    const int total = count * PW;
    for (int x = t; x < total; x += 64) sm[(x / PW) * PS + x % PW] = src[x];
  }
  __syncthreads();
  const bool own = t < count;
  double W[D][B];
  if (own) {
    const double* ps = sm + t * PS;
    if (frames != nullptr) {  // block-uniform
      const double* F = frames + static_cast<long>(frame_of[first + t]) * PW;
#pragma unroll
      for (int c = 0; c < B; ++c)
#pragma unroll
        for (int u = 0; u < D; ++u) {
          double s = c == D ? F[D * D + u] : 0.0;
#pragma unroll
          for (int k = 0; k < D; ++k) s = fma(F[k * D + u], ps[c * D + k], s);
          W[u][c] = s;
        }
    } else {
#pragma unroll
      for (int c = 0; c < B; ++c)
#pragma unroll
        for (int u = 0; u < D; ++u) W[u][c] = ps[c * D + u];
    }
  }
  __syncthreads();  // every pose of the span is in registers: its LDS now takes the lifted poses
  if (own) {
    double* po = sm + t * OS;
#pragma unroll
    for (int c = 0; c < B; ++c)
#pragma unroll
      for (int a = 0; a < R; ++a) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < D; ++u) s = fma(yl.v[u * R + a], W[u][c], s);
        po[c * R + a] = s;
      }
  }
  __syncthreads();
  if (OW % 2 == 0 && full && (reinterpret_cast<unsigned long>(dst) & 15) == 0) {
    constexpr int NO = OW / 2;
    double2* O2 = reinterpret_cast<double2*>(dst);
#pragma unroll
    for (int i = 0; i < NO; ++i) {
      const int x = 2 * (t + 64 * i);
      const double* q = sm + (x / OW) * OS + x % OW;
      O2[t + 64 * i] = make_double2(q[0], q[1]);
    }
  } else {
    const int total_out = count * OW;
    for (int x = t; x < total_out; x += 64) dst[x] = sm[(x / OW) * OS + x % OW];
  }
}

// Rank reduction, first half (build-defined): the Gram matrix of the rotation columns,
//   C = sum_j Y_j Y_j^T   (R x R; the translation column takes no part),
// as R (R + 1) / 2 packed sums (a <= c at index c (c + 1) / 2 + a).  Block k takes the kGramSpans consecutive 64-pose
// spans from pose 64 kGramSpans k on; each span streams through LDS exactly as k_round_se stages it (16-byte chunks on
// a full, aligned span, 8-byte otherwise: the staging moves bits only, so the sums do not depend on the alignment),
// thread t adds its pose's products -- each one a product and D - 1 FMAs, then one addition into the thread's sum --
// and after the last span one xor butterfly over the 64 lanes (five DPP / permute steps and one across the halves per
// packed entry, the same order in every lane) leaves the block's partial, which lane 0 writes.  The grid is a
// function of n alone; k_gram_finish sums the partials.  No atomics anywhere.
template <int R, int B>
__global__ __launch_bounds__(64) void k_gram(long n, const double* __restrict__ X, double* __restrict__ partial) {
  constexpr int D = B - 1;
  constexpr int PW = R * B, PS = PW | 1;
  constexpr int P = R * (R + 1) / 2;
  __shared__ double sm[64 * PS];
  const int t = static_cast<int>(threadIdx.x);
  double acc[P];
#pragma unroll
  for (int i = 0; i < P; ++i) acc[i] = 0.0;
#pragma unroll 1
  for (int s = 0; s < kGramSpans; ++s) {
    const long first = (static_cast<long>(blockIdx.x) * kGramSpans + s) * 64;
    if (first >= n) break;  // block-uniform
    const int count = n - first < 64 ? static_cast<int>(n - first) : 64;
    const double* src = X + first * PW;
    if (s > 0) __syncthreads();  // the previous span has been read
    if (PW % 2 == 0 && count == 64 && (reinterpret_cast<unsigned long>(src) & 15) == 0) {
      constexpr int NV = PW / 2;  // 16-byte chunks per lane (PW even: a chunk never straddles two poses)
      const double2* S2 = reinterpret_cast<const double2*>(src);
      double2 v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = S2[t + 64 * i];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int x = 2 * (t + 64 * i);
        double* q = sm + (x / PW) * PS + x % PW;
        q[0] = v[i].x;
        q[1] = v[i].y;
      }
    } else {
      const int total = count * PW;
      for (int x = t; x < total; x += 64) sm[(x / PW) * PS + x % PW] = src[x];
    }
    __syncthreads();
    if (t < count) {
      const double* ps = sm + t * PS;
      double Y[R][D];
#pragma unroll
      for (int c = 0; c < D; ++c)
#pragma unroll
        for (int a = 0; a < R; ++a) Y[a][c] = ps[c * R + a];
#pragma unroll
      for (int c = 0; c < R; ++c)
#pragma unroll
        for (int a = 0; a <= c; ++a) {
          double p = Y[a][0] * Y[c][0];
#pragma unroll
          for (int q = 1; q < D; ++q) p = fma(Y[a][q], Y[c][q], p);
          acc[c * (c + 1) / 2 + a] += p;
        }
    }
  }
#pragma unroll
  for (int i = 0; i < P; ++i) {
    double v = acc[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    acc[i] = v;
  }
  if (t == 0) {  // entry-major: k_gram_finish reads each entry's partials contiguously
    double* dst = partial + blockIdx.x;
#pragma unroll
    for (int i = 0; i < P; ++i) dst[static_cast<long>(i) * gridDim.x] = acc[i];
  }
}

// Second half of the Gram: block i sums packed entry i of the `blocks` partials (entry-major: partial[i blocks + g]
// is block g's) -- thread t adds partials t, t + 1024, ... in that order, k_gram's butterfly sums each wave, and
// thread 0 adds the 16 wave sums in wave order -- and writes it at both (a, c) and (c, a) of the full column-major C.
// The order is a function of `blocks` alone: bitwise repeatable.
constexpr int kGramFinishThreads = 1024;
__global__ __launch_bounds__(kGramFinishThreads) void k_gram_finish(long blocks, int R,
                                                                    const double* __restrict__ partial,
                                                                    double* __restrict__ C) {
  __shared__ double ws[kGramFinishThreads / 64];
  const int i = static_cast<int>(blockIdx.x);
  const int t = static_cast<int>(threadIdx.x);
  const double* src = partial + static_cast<long>(i) * blocks;
  double v = 0.0;
  for (long g = t; g < blocks; g += kGramFinishThreads) v += src[g];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((t & 63) == 0) ws[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    double s = ws[0];
#pragma unroll
    for (int k = 1; k < kGramFinishThreads / 64; ++k) s += ws[k];
    int c = 0;
    while ((c + 1) * (c + 2) / 2 <= i) ++c;
    const int a = i - c * (c + 1) / 2;
    C[c * R + a] = s;
    C[a * R + c] = s;
  }
}

// Rank reduction, second half: truncate the n poses X (R x B each) to rank K < R along W (R x K, orthonormal columns:
// the leading eigenvectors of k_gram's C), per pose
//   out_j = [polar(W^T Y_j) | W^T p_j],   K x B column-major,
// polar being LiftedSEManifold::project's factor (polar_fast: Newton-Schulz near the manifold, else polar_inplace's
// one-sided Jacobi).  A pose whose W^T Y_j is exactly rank-deficient takes the Jacobi path, whose zero columns stay
// zero (1 / sigma is replaced by 0): the output is finite and not orthonormal; that pose has no nearest point and
// the pass does not invent one.  k_round_se's shape: block k takes poses [64 k, 64 k + 64); the R B-wide span streams
// in through LDS coalesced (16-byte chunks where the span width is even, the block full and the span aligned, 8-byte
// otherwise), thread t works on pose t, and the K B-wide result streams out of the same LDS.  Row strides are the
// span widths made odd (conflict-free b64 reads).  W travels in the kernel arguments.
template <int R, int K, int B>
__global__ __launch_bounds__(64) void k_rank_project(long n, const double* __restrict__ X, RankW w,
                                                     double* __restrict__ out) {
  constexpr int D = B - 1;
  constexpr int PW = R * B, PS = PW | 1;
  constexpr int OW = K * B, OS = OW | 1;
  static_assert(D <= K && K < R && OS <= PS, "the reduced poses reuse the staged span's LDS");
  __shared__ double sm[64 * PS];
  const int t = static_cast<int>(threadIdx.x);
  const long first = static_cast<long>(blockIdx.x) * 64;
  if (first >= n) return;
  const int count = n - first < 64 ? static_cast<int>(n - first) : 64;
  const double* src = X + first * PW;
  double* dst = out + first * OW;
  const bool full = count == 64;
  if (PW % 2 == 0 && full && (reinterpret_cast<unsigned long>(src) & 15) == 0) {
    constexpr int NV = PW / 2;  // 16-byte chunks per lane (PW even: a chunk never straddles two poses)
    const double2* S2 = reinterpret_cast<const double2*>(src);
    double2 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = S2[t + 64 * i];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int x = 2 * (t + 64 * i);
      double* q = sm + (x / PW) * PS + x % PW;
      q[0] = v[i].x;
      q[1] = v[i].y;
    }
  } else {
    const int total = count * PW;
    for (int x = t; x < total; x += 64) sm[(x / PW) * PS + x % PW] = src[x];
  }
  __syncthreads();
  const bool own = t < count;
  double M[K][B];
  if (own) {
    const double* ps = sm + t * PS;
#pragma unroll
    for (int c = 0; c < B; ++c)
#pragma unroll
      for (int i = 0; i < K; ++i) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < R; ++a) s = fma(w.v[i * R + a], ps[c * R + a], s);
        M[i][c] = s;
      }
  }
  __syncthreads();  // every pose of the span is in registers: its LDS now takes the reduced poses
  if (own) {
    polar_fast<K, D>(M);  // the translation column passes through unchanged
    double* po = sm + t * OS;
#pragma unroll
    for (int c = 0; c < B; ++c)
#pragma unroll
      for (int i = 0; i < K; ++i) po[c * K + i] = M[i][c];
  }
  __syncthreads();
  if (OW % 2 == 0 && full && (reinterpret_cast<unsigned long>(dst) & 15) == 0) {
    constexpr int NO = OW / 2;
    double2* O2 = reinterpret_cast<double2*>(dst);
#pragma unroll
    for (int i = 0; i < NO; ++i) {
      const int x = 2 * (t + 64 * i);
      const double* q = sm + (x / OW) * OS + x % OW;
      O2[t + 64 * i] = make_double2(q[0], q[1]);
    }
  } else {
    const int total_out = count * OW;
    for (int x = t; x < total_out; x += 64) dst[x] = sm[(x / OW) * OS + x % OW];
  }
}

// Edge errors (build-defined batch form of computeMeasurementError, src/DPGO_utils.cpp:509-515; DESIGN 3.13 and 7
// item 13).  One thread per measurement e = (p1, p2, R, t, kappa, tau):
//   rot = |Y1 R - Y2|_F^2,  tra = |p2 - p1 - Y1 t|^2,  err = kappa rot + tau tra,
// the poses R x B column-major; an index s >= 0 is pose s of X, s < 0 pose -1 - s of X2 (GncEntries' encoding).
// One operation order per (R, D), the same for every edge, block, pointer alignment and pose source:
//   per row a: per column c, v = Y1[a,0] R[0,c], then D - 1 FMAs, df = v - Y2[a,c], rot = fma(df, df, rot);
//              yt = Y1[a,0] t[0], then D - 1 FMAs, dt = (p2[a] - p1[a]) - yt, tra = fma(dt, dt, tra);
//   err = (kappa rot) + (tau tra), each product rounded (no contraction).
// rot is a chain of R D squares, tra of R.  With `partial` the block also leaves sum_e (0.5 w_e) err_e over its
// kEdgeErrThreads edges (w NULL = ones; lanes past m add 0): k_gram's xor butterfly per wave, then thread 0 adds the wave
// sums in wave order.  k_edge_cost_finish sums the partials.  No atomics, no LDS beyond the wave sums, no scratch.
template <int R, int D>
__global__ __launch_bounds__(kEdgeErrThreads) void k_edge_errors(long m, const int* __restrict__ p1, const int* __restrict__ p2,
                                                          const double* __restrict__ Rm, const double* __restrict__ tv,
                                                          const double* __restrict__ kappa,
                                                          const double* __restrict__ tau, const double* __restrict__ w,
                                                          const double* __restrict__ X, const double* __restrict__ X2,
                                                          double* __restrict__ err, double* __restrict__ rot_sq,
                                                          double* __restrict__ tra_sq, double* __restrict__ partial) {
#pragma clang fp contract(off)
  constexpr int B = D + 1;
  __shared__ double ws[kEdgeErrThreads / 64];
  const long e = static_cast<long>(blockIdx.x) * kEdgeErrThreads + threadIdx.x;
  double term = 0.0;
  if (e < m) {
    const int s1 = p1[e], s2 = p2[e];
    const double* P1 = s1 >= 0 ? X + static_cast<long>(s1) * (R * B) : X2 + static_cast<long>(-1 - s1) * (R * B);
    const double* P2 = s2 >= 0 ? X + static_cast<long>(s2) * (R * B) : X2 + static_cast<long>(-1 - s2) * (R * B);
    double Rr[D][D], tr[D];
#pragma unroll
    for (int u = 0; u < D; ++u) {
#pragma unroll
      for (int c = 0; c < D; ++c) Rr[u][c] = Rm[e * (D * D) + u * D + c];
      tr[u] = tv[e * D + u];
    }
    double rot = 0.0, tra = 0.0;
#pragma unroll
    for (int a = 0; a < R; ++a) {
      double y1[B];
#pragma unroll
      for (int u = 0; u < B; ++u) y1[u] = P1[u * R + a];
#pragma unroll
      for (int c = 0; c < D; ++c) {
        double v = y1[0] * Rr[0][c];
#pragma unroll
        for (int u = 1; u < D; ++u) v = fma(y1[u], Rr[u][c], v);
        const double df = v - P2[c * R + a];
        rot = fma(df, df, rot);
      }
      double yt = y1[0] * tr[0];
#pragma unroll
      for (int u = 1; u < D; ++u) yt = fma(y1[u], tr[u], yt);
      const double dt = (P2[D * R + a] - y1[D]) - yt;
      tra = fma(dt, dt, tra);
    }
    const double kr = kappa[e] * rot, tt = tau[e] * tra;
    const double er = kr + tt;
    if (err) err[e] = er;
    if (rot_sq) rot_sq[e] = rot;
    if (tra_sq) tra_sq[e] = tra;
    if (partial) term = (w ? 0.5 * w[e] : 0.5) * er;
  }
  if (partial == nullptr) return;  // uniform over the grid
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) term += __shfl_xor(term, off, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = term;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = ws[0];
#pragma unroll
    for (int k = 1; k < kEdgeErrThreads / 64; ++k) s += ws[k];
    partial[blockIdx.x] = s;
  }
}

// The cost from k_edge_errors' block partials, one block: thread t adds partials t, t + 1024, ... in that order,
// the xor butterfly sums each wave, thread 0 adds the 16 wave sums in wave order.  A function of `blocks` alone.
constexpr int kEdgeFinishThreads = 1024;
__global__ __launch_bounds__(kEdgeFinishThreads) void k_edge_cost_finish(long blocks,
                                                                         const double* __restrict__ partial,
                                                                         double* __restrict__ cost) {
  __shared__ double ws[kEdgeFinishThreads / 64];
  const int t = static_cast<int>(threadIdx.x);
  double v = 0.0;
  for (long g = t; g < blocks; g += kEdgeFinishThreads) v += partial[g];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((t & 63) == 0) ws[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    double s = ws[0];
#pragma unroll
    for (int k = 1; k < kEdgeFinishThreads / 64; ++k) s += ws[k];
    *cost = s;
  }
}

// ---- trajectory evaluation against a ground truth (build-defined) ----
// A 64-pose span of SE(D) poses (PW = D (D + 1) doubles each, PW even) into LDS at row stride PW + 1, as k_round_se
// stages it: 16-byte chunks on a full, 16-byte-aligned span, 8-byte loads otherwise.  The staging moves bits only.
template <int PW>
__device__ __forceinline__ void traj_stage_span(double* sm, const double* __restrict__ src, int count, int t) {
  constexpr int PS = PW + 1;
  static_assert(PW % 2 == 0, "a 16-byte chunk never straddles two poses");
  if (count == 64 && (reinterpret_cast<unsigned long>(src) & 15) == 0) {
    constexpr int NV = PW / 2;
    const double2* S2 = reinterpret_cast<const double2*>(src);
    double2 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = S2[t + 64 * i];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int x = 2 * (t + 64 * i);
      double* q = sm + (x / PW) * PS + x % PW;
      q[0] = v[i].x;
      q[1] = v[i].y;
    }
  } else {
    const int total = count * PW;
    for (int x = t; x < total; x += 64) sm[(x / PW) * PS + x % PW] = src[x];
  }
}

// Moments of two trajectories' translations about a shift (sh = the estimate's, st = the truth's): with
// a = fl(that_j - sh), b = fl(t_j - st) per used pose (use null = every pose, else use[j] != 0),
//   [count, sum |a|^2, sum |b|^2, sum a (D), sum b (D), M = sum b a^T (D x D column-major)]   (3 + 2 D + D^2 sums).
// k_gram's shape: block k takes the kTrajSpans consecutive 64-pose spans from pose 64 kTrajSpans k on, both
// trajectories stream through LDS, thread t adds its pose's terms (a squared norm is one product and D - 1 FMAs, a
// product b_i a_j one multiplication) to its sums, and one xor butterfly over the 64 lanes leaves the block's partial
// (entry-major, for k_traj_finish).  The grid is a function of n alone.  No atomics.
struct TrajShift {
  double sh[3], st[3];
};
template <int D>
__global__ __launch_bounds__(64) void k_traj_moments(long n, const double* __restrict__ That,
                                                     const double* __restrict__ T, const int* __restrict__ use,
                                                     TrajShift S, double* __restrict__ partial) {
#pragma clang fp contract(off)
  constexpr int PW = D * (D + 1), PS = PW + 1;
  constexpr int P = 3 + 2 * D + D * D;
  __shared__ double sa[64 * PS], sb[64 * PS];
  const int t = static_cast<int>(threadIdx.x);
  double acc[P];
#pragma unroll
  for (int i = 0; i < P; ++i) acc[i] = 0.0;
#pragma unroll 1
  for (int s = 0; s < kTrajSpans; ++s) {
    const long first = (static_cast<long>(blockIdx.x) * kTrajSpans + s) * 64;
    if (first >= n) break;  // block-uniform
    const int count = n - first < 64 ? static_cast<int>(n - first) : 64;
    if (s > 0) __syncthreads();  // the previous span has been read
    traj_stage_span<PW>(sa, That + first * PW, count, t);
    traj_stage_span<PW>(sb, T + first * PW, count, t);
    __syncthreads();
    if (t < count && (use == nullptr || use[first + t] != 0)) {
      const double* pa = sa + t * PS + D * D;
      const double* pb = sb + t * PS + D * D;
      double a[D], b[D];
#pragma unroll
      for (int i = 0; i < D; ++i) {
        a[i] = pa[i] - S.sh[i];
        b[i] = pb[i] - S.st[i];
      }
      double na = a[0] * a[0], nb = b[0] * b[0];
#pragma unroll
      for (int i = 1; i < D; ++i) {
        na = fma(a[i], a[i], na);
        nb = fma(b[i], b[i], nb);
      }
      acc[0] += 1.0;
      acc[1] += na;
      acc[2] += nb;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        acc[3 + i] += a[i];
        acc[3 + D + i] += b[i];
      }
#pragma unroll
      for (int c = 0; c < D; ++c)
#pragma unroll
        for (int i = 0; i < D; ++i) acc[3 + 2 * D + c * D + i] += b[i] * a[c];
    }
  }
#pragma unroll
  for (int i = 0; i < P; ++i) {
    double v = acc[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    acc[i] = v;
  }
  if (t == 0) {
    double* dst = partial + blockIdx.x;
#pragma unroll
    for (int i = 0; i < P; ++i) dst[static_cast<long>(i) * gridDim.x] = acc[i];
  }
}

// Entry i (= the block) of the `blocks` entry-major partials into out[i], in k_gram_finish's order: thread t takes
// partials t, t + 1024, ..., the xor butterfly joins each wave, thread 0 joins the 16 wave results in wave order.
// Entries below nsum are sums, the others maxima (exact in any order).  A function of `blocks` alone.
constexpr int kTrajFinishThreads = 1024;
__global__ __launch_bounds__(kTrajFinishThreads) void k_traj_finish(long blocks, int nsum,
                                                                    const double* __restrict__ partial,
                                                                    double* __restrict__ out) {
  __shared__ double ws[kTrajFinishThreads / 64];
  const int i = static_cast<int>(blockIdx.x);
  const int t = static_cast<int>(threadIdx.x);
  const bool sum = i < nsum;  // block-uniform
  const double* src = partial + static_cast<long>(i) * blocks;
  double v = 0.0;  // the maxima are of squares: 0 is their identity too
  if (sum) {
    for (long g = t; g < blocks; g += kTrajFinishThreads) v += src[g];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  } else {
    for (long g = t; g < blocks; g += kTrajFinishThreads) v = fmax(v, src[g]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  }
  if ((t & 63) == 0) ws[t >> 6] = v;
  __syncthreads();
  if (t == 0) {
    double s = ws[0];
#pragma unroll
    for (int k = 1; k < kTrajFinishThreads / 64; ++k) s = sum ? s + ws[k] : fmax(s, ws[k]);
    out[i] = s;
  }
}

// Per-pose errors of the estimate That against the truth T under the rigid map [A | a] (D x (D + 1) column-major in
// the kernel arguments):
//   tra_sq[j] = |A that_j + a - t_j|^2,   rot_sq[j] = |A Rhat_j - R_j|_F^2   (chordal).
// One operation order per D, the same for every pose, block and pointer alignment:
//   per row i: v = A[i,0] that[0], then D - 1 FMAs, v = v + a[i], rho = v - t[i], tra = fma(rho, rho, tra);
//   per column c, per row i: v = A[i,0] Rhat[0,c], then D - 1 FMAs, df = v - R[i,c], rot = fma(df, df, rot).
// An unused pose (use[j] == 0) gets a quiet NaN in both outputs and takes no part in the block's partial
// [count, sum tra, sum rot, max tra, max rot] (entry-major; k_traj_moments' shape, spans, butterfly and finish).
struct TrajAa {
  double v[12];
};
template <int D>
__global__ __launch_bounds__(64) void k_traj_errors(long n, const double* __restrict__ That,
                                                    const double* __restrict__ T, const int* __restrict__ use,
                                                    TrajAa Aa, double* __restrict__ tra_sq,
                                                    double* __restrict__ rot_sq, double* __restrict__ partial) {
#pragma clang fp contract(off)
  constexpr int PW = D * (D + 1), PS = PW + 1;
  __shared__ double sa[64 * PS], sb[64 * PS];
  const int t = static_cast<int>(threadIdx.x);
  double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int s = 0; s < kTrajSpans; ++s) {
    const long first = (static_cast<long>(blockIdx.x) * kTrajSpans + s) * 64;
    if (first >= n) break;  // block-uniform
    const int count = n - first < 64 ? static_cast<int>(n - first) : 64;
    if (s > 0) __syncthreads();
    traj_stage_span<PW>(sa, That + first * PW, count, t);
    traj_stage_span<PW>(sb, T + first * PW, count, t);
    __syncthreads();
    if (t < count) {
      const long j = first + t;
      if (use == nullptr || use[j] != 0) {
        const double* pa = sa + t * PS;
        const double* pb = sb + t * PS;
        double tra = 0.0, rot = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) {
          double v = Aa.v[i] * pa[D * D];
#pragma unroll
          for (int k = 1; k < D; ++k) v = fma(Aa.v[k * D + i], pa[D * D + k], v);
          v = v + Aa.v[D * D + i];
          const double rho = v - pb[D * D + i];
          tra = fma(rho, rho, tra);
        }
#pragma unroll
        for (int c = 0; c < D; ++c)
#pragma unroll
          for (int i = 0; i < D; ++i) {
            double v = Aa.v[i] * pa[c * D];
#pragma unroll
            for (int k = 1; k < D; ++k) v = fma(Aa.v[k * D + i], pa[c * D + k], v);
            const double df = v - pb[c * D + i];
            rot = fma(df, df, rot);
          }
        if (tra_sq) tra_sq[j] = tra;
        if (rot_sq) rot_sq[j] = rot;
        acc[0] += 1.0;
        acc[1] += tra;
        acc[2] += rot;
        acc[3] = fmax(acc[3], tra);
        acc[4] = fmax(acc[4], rot);
      } else {
        const double qnan = __longlong_as_double(0x7ff8000000000000LL);
        if (tra_sq) tra_sq[j] = qnan;
        if (rot_sq) rot_sq[j] = qnan;
      }
    }
  }
  if (partial == nullptr) return;  // uniform over the grid
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    double v = acc[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double o = __shfl_xor(v, off, 64);
      v = i < 3 ? v + o : fmax(v, o);
    }
    acc[i] = v;
  }
  if (t == 0) {
    double* dst = partial + blockIdx.x;
#pragma unroll
    for (int i = 0; i < 5; ++i) dst[static_cast<long>(i) * gridDim.x] = acc[i];
  }
}

// Relative poses of a trajectory T over an edge list, one thread per edge (two gathered poses in, D^2 + D doubles
// out, as dpgo_edges takes them):
//   R_out[e] (row-major) = R_p1^T R_p2,   t_out[e] = R_p1^T (t_p2 - t_p1).
// Entry (u, c): R1[0,u] R2[0,c], then D - 1 FMAs; t_out[u]: dt = t2 - t1 per component, R1[0,u] dt[0], then D - 1
// FMAs.  The same order for every edge: an edge's outputs depend on its two poses alone.
template <int D>
__global__ __launch_bounds__(kEdgeErrThreads) void k_relative_poses(long m, const int* __restrict__ p1,
                                                                    const int* __restrict__ p2,
                                                                    const double* __restrict__ T,
                                                                    double* __restrict__ R_out,
                                                                    double* __restrict__ t_out) {
#pragma clang fp contract(off)
  constexpr int PW = D * (D + 1);
  const long e = static_cast<long>(blockIdx.x) * kEdgeErrThreads + threadIdx.x;
  if (e >= m) return;
  const double* P1 = T + static_cast<long>(p1[e]) * PW;
  const double* P2 = T + static_cast<long>(p2[e]) * PW;
  double a[PW], b[PW];
#pragma unroll
  for (int x = 0; x < PW; ++x) {
    a[x] = P1[x];
    b[x] = P2[x];
  }
  double dt[D];
#pragma unroll
  for (int k = 0; k < D; ++k) dt[k] = b[D * D + k] - a[D * D + k];
#pragma unroll
  for (int u = 0; u < D; ++u) {
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double v = a[u * D] * b[c * D];
#pragma unroll
      for (int k = 1; k < D; ++k) v = fma(a[u * D + k], b[c * D + k], v);
      R_out[e * (D * D) + u * D + c] = v;
    }
    double w = a[u * D] * dt[0];
#pragma unroll
    for (int k = 1; k < D; ++k) w = fma(a[u * D + k], dt[k], w);
    t_out[e * D + u] = w;
  }
}

// Pairwise consistency of frame candidates (pcm_pair.h: definitions, operation order, contraction off).  One wave
// per 64 x 64 tile of one group: the tile's row candidates are staged in LDS (coalesced copy, record stride
// pcm_record<D>()), lane l keeps column candidate c0 + l in registers (15 doubles at D = 3, 8 at D = 2) and the wave
// walks the rows, every lane reading the row's record at one LDS address (a broadcast: no bank conflict).  The
// ballot of the 64 decisions is word col_tile of row k; lane r keeps row r's word and stores it after the walk, one
// plain 8-byte vector store per row.  A lane past the group's end votes 0, which leaves the padding bits zero; rows
// past the end are not walked.  degree gathers __popcll of the stored words by integer atomics (exact in any order).
template <int D>
__global__ __launch_bounds__(64) void k_pair_consistency(const PcmTile* __restrict__ tiles,
                                                         const double* __restrict__ F, const double* __restrict__ x,
                                                         const int* __restrict__ group_off,
                                                         const long long* __restrict__ word_off,
                                                         const long long* __restrict__ dense_off, double cR2,
                                                         double ct2, unsigned long long* __restrict__ adj,
                                                         int* __restrict__ degree, double* __restrict__ e_rot,
                                                         double* __restrict__ e_tra) {
  constexpr int PW = D * (D + 1), REC = pcm_record<D>();
  __shared__ double sm[64 * REC];
  const int lane = static_cast<int>(threadIdx.x);
  const PcmTile T = tiles[blockIdx.x];
  const int g0 = group_off[T.group], mg = group_off[T.group + 1] - g0;
  const int r0 = T.row_tile * 64, c0 = T.col_tile * 64;
  const int rows = mg - r0 < 64 ? mg - r0 : 64;  // >= 1: the table lists tiles inside the group only
  const double* Fr = F + static_cast<long>(g0 + r0) * PW;
  const double* xr = x + static_cast<long>(g0 + r0) * D;
  for (int i = lane; i < rows * PW; i += 64) sm[(i / PW) * REC + i % PW] = Fr[i];
  for (int i = lane; i < rows * D; i += 64) sm[(i / D) * REC + PW + i % D] = xr[i];
  const int l = c0 + lane;
  const bool valid = l < mg;
  double col[REC];
#pragma unroll
  for (int i = 0; i < REC; ++i) col[i] = 0.0;
  if (valid) {
    const double* Fc = F + static_cast<long>(g0 + l) * PW;
    const double* xc = x + static_cast<long>(g0 + l) * D;
#pragma unroll
    for (int i = 0; i < PW; ++i) col[i] = Fc[i];
#pragma unroll
    for (int i = 0; i < D; ++i) col[PW + i] = xc[i];
  }
  __syncthreads();
  const long long dbase = dense_off[T.group];
  unsigned long long mine = 0;
  for (int r = 0; r < rows; ++r) {
    double er, et;
    pcm_pair_errors<D>(sm + r * REC, col, er, et);
    const int k = r0 + r;
    const bool ok = valid && k != l && pcm_consistent(er, et, cR2, ct2);
    const unsigned long long word = __ballot(ok);
    if (lane == r) mine = word;
    if (valid) {
      const long long at = dbase + static_cast<long long>(k) * mg + l;
      if (e_rot) e_rot[at] = er;
      if (e_tra) e_tra[at] = et;
    }
  }
  if (lane < rows) {
    const int words = (mg + 63) / 64;
    adj[word_off[T.group] + static_cast<long long>(r0 + lane) * words + T.col_tile] = mine;
    if (mine != 0) atomicAdd(&degree[g0 + r0 + lane], __popcll(mine));
  }
}

// Nesterov updateV deferred into the colour's next combination pass (one pass instead of two):
//   V' = project(V + gv (X - Yv))   (updateV, src/PGOAgent.cpp:1086-1091, of the agent's last update)
//   out = project(sa X + sb V')     (updateY / the iterate(false) step, :1077-1084, of the next iteration)
// V' is written back to V.  The combinations are the expressions k_polar_comb evaluates, so the
// results are those of the two separate passes.
// NEXT (TUNE_NEXT_Y, the engine's non-selected pass over the colour selected next): two more outputs from the
// registers, the colour's next updateY and status reference,
//   ynext = project(sa2 out + sb2 V')   and   xprev = out,
// k_polar_comb's expressions on the values it would load back.  ynext may be the buffer Yv was read from.
template <int R, int B, bool NEXT>
__global__ __launch_bounds__(64) void k_polar_vnext(LaunchCtx c, const double* __restrict__ X,
                                                    double* __restrict__ V, const double* __restrict__ Yv,
                                                    double gv, double sa, double sb, double* __restrict__ out,
                                                    double* __restrict__ xcopy, double sa2, double sb2, double* ynext,
                                                    double* __restrict__ xprev) {
  constexpr int D = B - 1;
  constexpr int PW = R * B;
  constexpr int PS = PW + 1;
  __shared__ double sm[64 * PS];
  const int tile = launch_tile(c);
  const int agent = c.tile_agent[tile];
  if (tile_skipped(c, agent)) return;
  const int count = c.tile_count[tile];
  const long base = static_cast<long>(c.tile_start[tile]) * PW;
  const int total = count * PW;
  const int t = static_cast<int>(threadIdx.x);
  auto project_span = [&]() {
    if (t < count) {
      double M[R][B];
      double* ps = sm + t * PS;
#pragma unroll
      for (int cc = 0; cc < D; ++cc)
#pragma unroll
        for (int a = 0; a < R; ++a) M[a][cc] = ps[cc * R + a];
#pragma unroll
      for (int a = 0; a < R; ++a) M[a][D] = 0.0;
      polar_fast<R, D>(M);
#pragma unroll
      for (int cc = 0; cc < D; ++cc)
#pragma unroll
        for (int a = 0; a < R; ++a) ps[cc * R + a] = M[a][cc];
    }
  };
  constexpr bool kVec = PW % 2 == 0;
  if (kVec && count == 64) {
    constexpr int NV = PW / 2;
    const double2* X2 = reinterpret_cast<const double2*>(X + base);
    const double2* V2 = reinterpret_cast<const double2*>(V + base);
    const double2* Y2 = reinterpret_cast<const double2*>(Yv + base);
    double2 vx[NV], vv[NV], vy[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) vx[i] = X2[t + 64 * i];
    if (xcopy != nullptr) {
      double2* XC = reinterpret_cast<double2*>(xcopy + base);
#pragma unroll
      for (int i = 0; i < NV; ++i) XC[t + 64 * i] = vx[i];
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) vv[i] = V2[t + 64 * i];
#pragma unroll
    for (int i = 0; i < NV; ++i) vy[i] = Y2[t + 64 * i];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int x = 2 * (t + 64 * i);
      double* dst = sm + (x / PW) * PS + x % PW;
      dst[0] = vv[i].x + gv * (vx[i].x - vy[i].x);
      dst[1] = vv[i].y + gv * (vx[i].y - vy[i].y);
    }
    __syncthreads();
    project_span();
    __syncthreads();
    double2* Vo = reinterpret_cast<double2*>(V + base);
#pragma unroll
    for (int i = 0; i < NV; ++i) {  // each lane re-reads exactly the LDS words it wrote above
      const int x = 2 * (t + 64 * i);
      double* src = sm + (x / PW) * PS + x % PW;
      const double2 v = make_double2(src[0], src[1]);
      Vo[t + 64 * i] = v;
      src[0] = sa * vx[i].x + sb * v.x;
      src[1] = sa * vx[i].y + sb * v.y;
      if constexpr (NEXT) vv[i] = v;  // V' stays in registers for ynext
    }
    __syncthreads();
    project_span();
    __syncthreads();
    double2* O2 = reinterpret_cast<double2*>(out + base);
    if constexpr (NEXT) {
      double2* XP = reinterpret_cast<double2*>(xprev + base);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int x = 2 * (t + 64 * i);
        double* src = sm + (x / PW) * PS + x % PW;
        const double2 xn = make_double2(src[0], src[1]);
        O2[t + 64 * i] = xn;
        if (xprev != nullptr) XP[t + 64 * i] = xn;
        src[0] = comb_xv(sa2, xn.x, sb2, vv[i].x);
        src[1] = comb_xv(sa2, xn.y, sb2, vv[i].y);
      }
      __syncthreads();
      project_span();
      __syncthreads();
      double2* Y2n = reinterpret_cast<double2*>(ynext + base);
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int x = 2 * (t + 64 * i);
        const double* src = sm + (x / PW) * PS + x % PW;
        Y2n[t + 64 * i] = make_double2(src[0], src[1]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int x = 2 * (t + 64 * i);
        const double* src = sm + (x / PW) * PS + x % PW;
        O2[t + 64 * i] = make_double2(src[0], src[1]);
      }
    }
  } else {
    for (int x = t; x < total; x += 64) {
      if (xcopy != nullptr) xcopy[base + x] = X[base + x];
      sm[(x / PW) * PS + x % PW] = V[base + x] + gv * (X[base + x] - Yv[base + x]);
    }
    __syncthreads();
    project_span();
    __syncthreads();
    for (int x = t; x < total; x += 64) {
      double* src = sm + (x / PW) * PS + x % PW;
      const double v = *src;
      V[base + x] = v;
      *src = sa * X[base + x] + sb * v;
    }
    __syncthreads();
    project_span();
    __syncthreads();
    if constexpr (NEXT) {
      for (int x = t; x < total; x += 64) {  // V[base + x] is this thread's own store above
        double* src = sm + (x / PW) * PS + x % PW;
        const double xn = *src;
        out[base + x] = xn;
        if (xprev != nullptr) xprev[base + x] = xn;
        *src = comb_xv(sa2, xn, sb2, V[base + x]);
      }
      __syncthreads();
      project_span();
      __syncthreads();
      for (int x = t; x < total; x += 64) ynext[base + x] = sm[(x / PW) * PS + x % PW];
    } else {
      for (int x = t; x < total; x += 64) out[base + x] = sm[(x / PW) * PS + x % PW];
    }
  }
}

// out = sel ? A : B per agent; partial |out - ref|^2
template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_select(LaunchCtx c, const double* __restrict__ A,
                                                     const double* __restrict__ Bv,
                                                     const int* __restrict__ use_a,
                                                     const double* __restrict__ ref,
                                                     double* __restrict__ out) {
  const PoseLane p = pose_lane<B>(c);
  if (tile_skipped(c, p.agent)) return;
  const bool own = p.ok && p.k < B;
  const long off = p.j * (R * B) + p.k * R;
  bool ua;
  if (use_a != nullptr) {
    ua = use_a[p.agent] != 0;
  } else {  // QuadraticOptimizer::trustRegion result: accepted step, else the input (:92-110)
    const AgentState& st = c.state[p.agent];
    ua = st.runs > 0 && st.accepted && !st.gave_up;
  }
  double dd = 0.0;
  if (own) {
#pragma unroll
    for (int a = 0; a < R; ++a) {
      const double v = ua ? A[off + a] : Bv[off + a];
      const double df = v - ref[off + a];
      dd = fma(df, df, dd);
      out[off + a] = v;
    }
  }
  double parts[1] = {dd};
  block_partials<1>(parts, c.partials, p.tile);
}

// partial |A - B|^2 per tile (PGOAgent status relativeChange against XPrev, src/PGOAgent.cpp:707)
template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_sqdiff(LaunchCtx c, const double* __restrict__ A,
                                                     const double* __restrict__ Bv) {
  const PoseLane p = pose_lane<B>(c);
  if (tile_skipped(c, p.agent)) return;
  const bool own = p.ok && p.k < B;
  const long off = p.j * (R * B) + p.k * R;
  double dd = 0.0;
  if (own) {
#pragma unroll
    for (int a = 0; a < R; ++a) {
      const double df = A[off + a] - Bv[off + a];
      dd = fma(df, df, dd);
    }
  }
  double parts[1] = {dd};
  block_partials<1>(parts, c.partials, p.tile);
}

// accepted RTR step in a multi-iteration Run: x1 <- x2, g <- g2, S <- S2
template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_accept(LaunchCtx c, const double* __restrict__ x2,
                                                     const double* __restrict__ g2,
                                                     const double* __restrict__ S2,
                                                     double* __restrict__ x1, double* __restrict__ g,
                                                     double* __restrict__ S) {
  constexpr int D = B - 1;
  const PoseLane p = pose_lane<B>(c);
  if (c.state[p.agent].copy_pending == 0) return;
  if (!(p.ok && p.k < B)) return;
  const long off = p.j * (R * B) + p.k * R;
#pragma unroll
  for (int a = 0; a < R; ++a) {
    x1[off + a] = x2[off + a];
    g[off + a] = g2[off + a];
  }
  if (p.k == 0) {
#pragma unroll
    for (int v = 0; v < s_width(D); ++v) S[p.j * s_width(D) + v] = S2[p.j * s_width(D) + v];
  }
}

// Separate launch (grid = #agents, block = 256): every thread loads its tiles' partials, the two
// cross-wave levels go through LDS once for all quantities and the in-wave levels are shuffles; the
// agent's state is staged in LDS while the partials load and written back after the scalar logic.
static_assert(sizeof(AgentState) % sizeof(double) == 0, "AgentState is staged as doubles");
// OPC >= 0: specialised for one op (the per-tCG-iteration ones): a few hundred instructions instead of every
// op's logic -- a launch on a few CUs starts with a cold instruction cache, so the code it walks costs time.
// the finalize's stand-in operand for an absent partial quantity
__device__ const double g_zero_partial = 0.0;

#ifdef DPGO_FIN_PROBE
// tools/fin_probe.py (a variant build only): wall-clock marks inside the merged tCG finalize, agent 0's block
__device__ long long g_fin_probe[256][6];
__device__ int g_fin_probe_n;
#define DPGO_FIN_MARK(i) \
  if (probe) tp[i] = wall_clock64();
#else
#define DPGO_FIN_MARK(i)
#endif

template <int NQ, int OPC = -1>
__global__ __launch_bounds__(kThreads) void k_finalize(FinalizeArgs f) {
  static_assert(NQ <= kMaxTot, "finalize slots");
#ifdef DPGO_FIN_PROBE
  long long tp[6] = {};
  const bool probe = OPC == OP_TCG_STEP_CHECK && blockIdx.x == 0 && threadIdx.x == 0;
#endif
  DPGO_FIN_MARK(0)
  constexpr bool kDd = OPC < 0 || OPC == OP_TCG_STEP_CHECK || OPC == OP_TCG_CHECK_M;  // ops with dd partials
  const int agent = blockIdx.x;
  const int t0 = f.agent_tile_off[agent], t1 = f.agent_tile_off[agent + 1];
  constexpr int kStateWords = static_cast<int>(sizeof(AgentState) / sizeof(double));
  __shared__ double red[NQ][kThreads];
  __shared__ double red_lo[kDd ? NQ : 1][kThreads];  // low parts of double-double quantities (f.dd_mask)
  __shared__ AgentState sh_state;
  if (threadIdx.x < kStateWords)
    reinterpret_cast<double*>(&sh_state)[threadIdx.x] = reinterpret_cast<const double*>(&f.state[agent])[threadIdx.x];
  double acc[NQ], accl[NQ];
  const double* srcs[NQ];
  int qqs[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    acc[q] = 0.0;
    accl[q] = 0.0;
    srcs[q] = part_src(f, q, qqs[q]);
  }
  for (int t = t0 + threadIdx.x; t < t1; t += kThreads) {
    // every quantity's loads issued back to back (absent ones read a zero), then the sums: a load inside each
    // quantity's branch waited for its own round trip before the next load was issued
    double v[NQ], vl[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const bool have = srcs[q] != nullptr;
      const double* ph = have ? srcs[q] + t * kPartialStride + qqs[q] : &g_zero_partial;
      const double* pl = have && kDd && ((f.dd_mask >> q) & 1) ? ph + kDdLo : &g_zero_partial;
      v[q] = *ph;
      vl[q] = *pl;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (srcs[q] == nullptr) continue;
      if (kDd && ((f.dd_mask >> q) & 1)) {
        const dd a = dd_add({acc[q], accl[q]}, {v[q], vl[q]});
        acc[q] = a.hi;
        accl[q] = a.lo;
      } else {
        acc[q] += v[q];
      }
    }
  }
  DPGO_FIN_MARK(1)
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if (srcs[q] != nullptr) {
      red[q][threadIdx.x] = acc[q];
      if constexpr (kDd) red_lo[q][threadIdx.x] = accl[q];
    }
  __syncthreads();
  DPGO_FIN_MARK(2)
  // wave w reduces quantities w and w + 4 (lane 0's halving tree over the same lane pairs as the fused path)
  __shared__ double s_tot[2 * kMaxTot];
  const int l = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int q0 = 0; q0 < kMaxTot; q0 += 4) {
    const int q = q0 + wv;  // wave-uniform
    int qq = 0;
    double th = 0.0, tl = 0.0;
    if (q < NQ && part_src(f, q, qq) != nullptr) {
      if (kDd && ((f.dd_mask >> q) & 1)) {
        auto at = [&](int i) { return dd{red[q][i], red_lo[kDd ? q : 0][i]}; };
        const dd x = wave_sum_dd(dd_add(dd_add(at(l), at(l + 128)), dd_add(at(l + 64), at(l + 192))));
        th = x.hi;
        tl = x.lo;
      } else {
        th = wave_sum((red[q][l] + red[q][l + 128]) + (red[q][l + 64] + red[q][l + 192]));
      }
    }
    if (l == 0) {
      s_tot[q] = th;
      s_tot[kMaxTot + q] = tl;
    }
  }
  __syncthreads();
  DPGO_FIN_MARK(3)
  if (threadIdx.x != 0) return;
  double tot[kMaxTot], lo[kMaxTot];
#pragma unroll
  for (int q = 0; q < kMaxTot; ++q) {
    tot[q] = s_tot[q];
    lo[q] = s_tot[kMaxTot + q];
  }
  // the scalar logic runs on a register copy: a chain of dependent LDS accesses costs microseconds
  AgentState st = sh_state;
  finalize_scalar<OPC>(f, agent, tot, lo, st);
  DPGO_FIN_MARK(4)
  double* dst = reinterpret_cast<double*>(&f.state[agent]);
  const double* srcw = reinterpret_cast<const double*>(&st);
#pragma unroll
  for (int w = 0; w < kStateWords; ++w) dst[w] = srcw[w];
#ifdef DPGO_FIN_PROBE
  if (probe) {
    __builtin_amdgcn_s_waitcnt(0);
    tp[5] = wall_clock64();
    const int slot = atomicAdd(&g_fin_probe_n, 1) & 255;
    for (int m = 0; m < 6; ++m) g_fin_probe[slot][m] = tp[m];
  }
#endif
}


// Consumer-side finalize: the scalar logic of a k_finalize launch run in the prologue of the kernel
// that consumes its decision (k_tcg_update: OP_TCG_STEP, k_tcg_dir: OP_TCG_CHECK), so a tCG iteration
// is three launches instead of five.  Every block of the agent restates k_finalize's reduction of the
// agent's tile partials (same per-thread serial sums, same tree: bitwise the same totals) and its
// scalar logic on a private LDS copy of the agent's state, so every block takes the same decision.
// The block that arrives last on the agent's counter writes the copy back and publishes the status
// word.  A block reads the global state and partials only before its first barrier (their values are
// in LDS by then) and arrives after it, so the write-back races with no reader of this launch.
template <int NQ>
__device__ void prologue_finalize(const FinalizeArgs& f, int agent, int* arrive, AgentState& sh) {
  (void)arrive;
  constexpr int kStateWords = static_cast<int>(sizeof(AgentState) / sizeof(double));
  __shared__ double red[NQ][kThreads];
  const int t0 = f.agent_tile_off[agent], t1 = f.agent_tile_off[agent + 1];
  if (threadIdx.x < kStateWords)
    reinterpret_cast<double*>(&sh)[threadIdx.x] = reinterpret_cast<const double*>(&f.state[agent])[threadIdx.x];
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  for (int t = t0 + threadIdx.x; t < t1; t += kThreads) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      int qq = 0;
      const double* src = part_src(f, q, qq);
      if (src != nullptr) acc[q] += src[t * kPartialStride + qq];
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) red[q][threadIdx.x] = acc[q];
  __syncthreads();
  if (threadIdx.x < 64) {
    const int l = threadIdx.x;
    double tot[kMaxTot];
#pragma unroll
    for (int q = 0; q < kMaxTot; ++q) tot[q] = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      double v = (red[q][l] + red[q][l + 128]) + (red[q][l + 64] + red[q][l + 192]);
      tot[q] = wave_sum(v);  // lane 0's halving tree
    }
    if (l == 0) {
      FinalizeArgs g = f;
      g.pub = nullptr;  // published once, by the last block (finalize_arrive)
      AgentState st = sh;  // register copy (see k_finalize)
      const double nolo[kMaxTot] = {};  // the classic ops' quantities are plain sums
      finalize_scalar(g, agent, tot, nolo, st);
      sh = st;
    }
  }
  __syncthreads();
}

// Second half of the consumer-side finalize, at the end of the block (every block of the agent calls
// it exactly once, skipped or not): the last block to arrive writes the state copy back and
// publishes.  Arriving last means every other block of the agent has finished, so all of this
// launch's reads of the agent's global state are done.
__device__ void finalize_arrive(const FinalizeArgs& f, int agent, int* arrive, const AgentState& sh) {
  constexpr int kStateWords = static_cast<int>(sizeof(AgentState) / sizeof(double));
  __shared__ int s_last;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = f.agent_tile_off[agent + 1] - f.agent_tile_off[agent];
    const int old = atomicAdd(&arrive[agent], 1);
    s_last = old == n - 1 ? 1 : 0;
    if (s_last) atomicExch(&arrive[agent], 0);
  }
  __syncthreads();
  if (!s_last) return;
  if (threadIdx.x < kStateWords)
    reinterpret_cast<double*>(&f.state[agent])[threadIdx.x] = reinterpret_cast<const double*>(&sh)[threadIdx.x];
  if (threadIdx.x == 0 && f.pub != nullptr) {
    const int flag = f.pub_kind == 1 ? sh.tcg_active : sh.run_active;
    const int cg = f.pub_kind == 2 && sh.tcg_iters > 1 ? 2 : 0;
    const int never = f.pub_kind == 2 && sh.runs == 0 && !sh.run_active ? 4 : 0;
    __hip_atomic_store(&f.pub[agent], (f.pub_tag << 3) | never | cg | (flag ? 1 : 0), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// --- block-Jacobi inverse of (Q_jj + shift I), computed on device from Q's diagonal blocks ---
// In place on A = [M | I] (B x 2B): Gauss-Jordan with partial pivoting (SPD, so pivoting is a
// safety net); on return the right half holds M^-1.
template <int B>
__device__ __forceinline__ void gauss_jordan(double (&A)[B][2 * B]) {
#pragma unroll
  for (int col = 0; col < B; ++col) {
    int piv = col;
    double best = fabs(A[col][col]);
#pragma unroll
    for (int u = col + 1; u < B; ++u)
      if (fabs(A[u][col]) > best) {
        best = fabs(A[u][col]);
        piv = u;
      }
#pragma unroll
    for (int u = col + 1; u < B; ++u) {
      if (u == piv) {
#pragma unroll
        for (int w = 0; w < 2 * B; ++w) {
          const double t = A[col][w];
          A[col][w] = A[u][w];
          A[u][w] = t;
        }
      }
    }
    const double inv = 1.0 / A[col][col];
#pragma unroll
    for (int w = 0; w < 2 * B; ++w) A[col][w] *= inv;
#pragma unroll
    for (int u = 0; u < B; ++u) {
      if (u != col) {
        const double fct = A[u][col];
#pragma unroll
        for (int w = 0; w < 2 * B; ++w) A[u][w] = fma(-fct, A[col][w], A[u][w]);
      }
    }
  }
}

template <int B>
__global__ __launch_bounds__(kThreads) void k_bj_inverse(int n, QView q, double shift,
                                                         double* __restrict__ Minv) {
  const long j = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double A[B][2 * B];
#pragma unroll
  for (int u = 0; u < B; ++u)
#pragma unroll
    for (int w = 0; w < 2 * B; ++w) A[u][w] = (w - B == u) ? 1.0 : 0.0;
  const int beg = q.rowptr[j], end = q.rowptr[j + 1];
  for (int nz = beg; nz < end; ++nz) {
    if (q.col[nz] == j) {
      // block (j,j) column-major: element (u,w) at w*B + u
#pragma unroll
      for (int u = 0; u < B; ++u)
#pragma unroll
        for (int w = 0; w < B; ++w) A[u][w] += q.blocks[static_cast<long>(nz) * B * B + w * B + u];
    }
  }
#pragma unroll
  for (int u = 0; u < B; ++u) A[u][u] += shift;
  gauss_jordan<B>(A);
#pragma unroll
  for (int u = 0; u < B; ++u)
#pragma unroll
    for (int w = u; w < B; ++w) Minv[j * diag_width(B - 1) + minv_index<B>(u, w)] = A[u][B + w];
}

// Same from the packed diagonal blocks of an edge-stream Q (one thread per pose).
template <int B>
__global__ __launch_bounds__(kThreads) void k_bj_inverse_diag(int n, QView q, double shift,
                                                              double* __restrict__ Minv) {
  constexpr int DW = diag_width(B - 1);
  const long j = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double A[B][2 * B];
#pragma unroll
  for (int u = 0; u < B; ++u)
#pragma unroll
    for (int w = 0; w < B; ++w) {
      A[u][w] = q.diag[j * DW + sym_index<B>(u, w)] + (u == w ? shift : 0.0);
      A[u][B + w] = (u == w) ? 1.0 : 0.0;
    }
  gauss_jordan<B>(A);
#pragma unroll
  for (int u = 0; u < B; ++u)
#pragma unroll
    for (int w = u; w < B; ++w) Minv[j * diag_width(B - 1) + minv_index<B>(u, w)] = A[u][B + w];
}

// The certificate matrix's diagonal blocks (one thread per pose): S(X) = Q - Lambda(X), Lambda block-diagonal with
// pose j's packed sym(Y_j^T (XQ+G)_Y) (the S an EVAL pass leaves) in the rotation part and zero in the translation
// row / column.  out may not alias diag.
template <int B>
__global__ __launch_bounds__(kThreads) void k_cert_diag(int n, const double* __restrict__ diag,
                                                        const double* __restrict__ S, double* __restrict__ out) {
  constexpr int D = B - 1, DW = diag_width(D), SW = s_width(D);
  const long j = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= n) return;
#pragma unroll
  for (int u = 0; u < B; ++u)
#pragma unroll
    for (int v = u; v < B; ++v) {
      const double lam = (u < D && v < D) ? S[j * SW + sym_index<D>(u < D ? u : 0, v < D ? v : 0)] : 0.0;
      out[j * DW + sym_index<B>(u, v)] = diag[j * DW + sym_index<B>(u, v)] - lam;
    }
}

// ------------------------------------------------------------------------------------------
// On-device Q assembly from edge weights (PGOAgent::constructQMatrix after a GNC weight update,
// src/PGOAgent.cpp:720-781, 1181-1244).  raw per slot = [R (row-major) | t | kappa | tau]; the
// arithmetic mirrors edge_blocks() (graph.cpp) so the result is bitwise the host build.
// ------------------------------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void edge_T_Om(const double* __restrict__ q, double w, double (&T)[D + 1][D + 1],
                                          double (&Om)[D + 1]) {
#pragma unroll
  for (int u = 0; u < D; ++u) {
#pragma unroll
    for (int v = 0; v < D; ++v) T[u][v] = q[u * D + v];
    T[u][D] = q[D * D + u];
    Om[u] = w * q[D * D + D];
    T[D][u] = 0.0;
  }
  T[D][D] = 1.0;
  Om[D] = w * q[D * D + D + 1];
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_edge_records(int m, const double* __restrict__ raw,
                                                           const int* __restrict__ slot_of_edge,
                                                           const double* __restrict__ w, double* __restrict__ rec) {
  constexpr int B = D + 1, RAW = D * D + D + 2, RW = edge_rec_width(D);
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int s = slot_of_edge[e];
  double T[B][B], Om[B];
  edge_T_Om<D>(raw + static_cast<long>(s) * RAW, w[e], T, Om);
  double* M = rec + static_cast<long>(s) * RW;
#pragma unroll
  for (int u = 0; u < B; ++u)
#pragma unroll
    for (int v = 0; v < B; ++v) M[4 * u + v] = -(-T[u][v] * Om[v]);  // -Wij, as the host build
}

template <int D>
__global__ __launch_bounds__(kThreads) void k_edge_diag(int n, const double* __restrict__ raw,
                                                        const int* __restrict__ edge_of_slot_w,
                                                        const double* __restrict__ wslot,
                                                        const int* __restrict__ dinc_ptr, const int* __restrict__ dinc,
                                                        double* __restrict__ diag) {
  // no FMA contraction: the host build (x86-64, separate multiply and add) is reproduced bitwise
#pragma clang fp contract(off)
  constexpr int B = D + 1, RAW = D * D + D + 2, DW = diag_width(D);
  const long j = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double F[B][B];
#pragma unroll
  for (int u = 0; u < B; ++u)
#pragma unroll
    for (int v = 0; v < B; ++v) F[u][v] = 0.0;
  for (int z = dinc_ptr[j]; z < dinc_ptr[j + 1]; ++z) {
    const int code = dinc[z], s = code >> 1;
    double T[B][B], Om[B];
    edge_T_Om<D>(raw + static_cast<long>(s) * RAW, wslot[s], T, Om);
    if (code & 1) {  // p1 side: T Omega T^T
#pragma unroll
      for (int u = 0; u < B; ++u)
#pragma unroll
        for (int v = 0; v < B; ++v) {
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < B; ++q) acc += T[u][q] * Om[q] * T[v][q];
          F[v][u] += acc;  // column-major (v * b + u), summed as the host
        }
    } else {  // p2 side: Omega
#pragma unroll
      for (int u = 0; u < B; ++u) F[u][u] += Om[u];
    }
  }
  int o = 0;
#pragma unroll
  for (int u = 0; u < B; ++u)
#pragma unroll
    for (int v = u; v < B; ++v) diag[j * DW + o++] = F[v][u];
}

// RobustCost::weight (src/DPGO_robust.cpp:23-67), r = sqrt(computeMeasurementError)
__device__ __forceinline__ double robust_weight(const RobustParams& p, double r) {
  switch (p.type) {
    case 1: return 1.0 / r;                                    // L1
    case 2: return r < p.tls ? 1.0 : 0.0;                      // TLS
    case 3: return r < p.huber ? 1.0 : p.huber / r;            // Huber
    case 4: { const double a = 1.0 + r * r; return 1.0 / (a * a); }  // GM
    case 5: {                                                  // GNC_TLS, eq. (14) of the GNC paper
      const double rSq = r * r, bc = p.barc * p.barc;
      const double upper = (p.mu + 1) / p.mu * bc, lower = p.mu / (p.mu + 1) * bc;
      if (rSq >= upper) return 0.0;
      if (rSq <= lower) return 1.0;
      return sqrt(bc * p.mu * (p.mu + 1) / rSq) - p.mu;
    }
    default: return 1.0;                                       // L2
  }
}

// One thread per loop closure: computeMeasurementError (src/DPGO_utils.cpp:509-515)
//   kappa |Y1 R - Y2|^2 + tau |p2 - p1 - Y1 t|^2, residual = sqrt, weight.
// FIXED: fixed[e] != 0 marks a known inlier (isKnownInlier, :1186 / :1203): its weight stays what was set.  The
// FIXED = false instantiation never reads the argument and is the kernel as it was before the flags existed.
template <int R, int D, bool FIXED>
__global__ __launch_bounds__(kThreads) void k_gnc_weights(GncEntries g, const double* __restrict__ X,
                                                          const double* __restrict__ RX, RobustParams rp,
                                                          double* __restrict__ w_prob, double* __restrict__ w_g,
                                                          const unsigned char* __restrict__ fixed) {
  constexpr int B = D + 1;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= g.n) return;
  if constexpr (FIXED) {
    if (fixed[e] != 0) return;
  }
  const int s1 = g.src1[e], s2 = g.src2[e], ne = g.nbr_end[e];
  if (ne >= 0 && g.dict_ok[e] == 0) return;  // no neighbour pose received yet: weight unchanged (:1208-1212)
  const double* D_ = ne >= 0 ? g.dict + static_cast<long>(e) * (R * B) : nullptr;
  const double* P1 = ne == 0 ? D_ : s1 >= 0 ? X + static_cast<long>(s1) * (R * B) : RX + static_cast<long>(-1 - s1) * (R * B);
  const double* P2 = ne == 1 ? D_ : s2 >= 0 ? X + static_cast<long>(s2) * (R * B) : RX + static_cast<long>(-1 - s2) * (R * B);
  const double* Rm = g.R + static_cast<long>(e) * D * D;
  const double* tv = g.t + static_cast<long>(e) * D;
  double rot = 0.0, tra = 0.0;
#pragma unroll
  for (int a = 0; a < R; ++a) {
#pragma unroll
    for (int c = 0; c < D; ++c) {
      double v = 0.0;
#pragma unroll
      for (int u = 0; u < D; ++u) v += P1[u * R + a] * Rm[u * D + c];
      const double df = v - P2[c * R + a];
      rot += df * df;
    }
    double yt = 0.0;
#pragma unroll
    for (int u = 0; u < D; ++u) yt += P1[u * R + a] * tv[u];
    const double dt = P2[D * R + a] - P1[D * R + a] - yt;
    tra += dt * dt;
  }
  const double err = g.kappa[e] * rot + g.tau[e] * tra;
  const double w = robust_weight(rp, sqrt(err));
  w_prob[g.prob_edge[e]] = w;
  if (g.g_entry[e] >= 0) w_g[g.g_entry[e]] = w;
}

// The selected agents receive their neighbours' poses (updateNeighborPoses): every shared entry of a selected agent
// (mask[agent] != 0, or every agent without a mask) copies the neighbour's current pose into its dictionary slot.
// One thread per (entry, double).
template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_gnc_snapshot(GncEntries g, const double* __restrict__ X,
                                                           const double* __restrict__ RX, const int* __restrict__ mask) {
  const long x = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int e = static_cast<int>(x / (R * B)), q = static_cast<int>(x % (R * B));
  if (e >= g.n) return;
  const int ne = g.nbr_end[e];
  if (ne < 0 || (mask != nullptr && mask[g.agent[e]] == 0)) return;
  const int s = ne ? g.src2[e] : g.src1[e];
  const double* P = s >= 0 ? X + static_cast<long>(s) * (R * B) : RX + static_cast<long>(-1 - s) * (R * B);
  g.dict[static_cast<long>(e) * (R * B) + q] = P[q];
  if (q == 0) g.dict_ok[e] = 1;
}

// One block per agent: converged (w == 1 or w == 0) over all loop closures of the agent.  FIXED: a copy with
// fixed[idx[i]] != 0 (a known inlier, :1257 / :1266) is left out of the converged count and of the total, which is
// then counted; the FIXED = false instantiation is the kernel as it was before the flags existed.
template <bool FIXED>
__global__ __launch_bounds__(kThreads) void k_conv_ratio(const int* __restrict__ off, const int* __restrict__ idx,
                                                         const double* __restrict__ w, double* __restrict__ ratio,
                                                         const unsigned char* __restrict__ fixed) {
  __shared__ int cnt[2];
  const int a = blockIdx.x;
  if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
  __syncthreads();
  int conv = 0, counted = 0;
  for (int i = off[a] + threadIdx.x; i < off[a + 1]; i += kThreads) {
    if constexpr (FIXED) {
      if (fixed[idx[i]] != 0) continue;
      counted += 1;
    }
    const double v = w[idx[i]];
    conv += (v == 1.0 || v == 0.0) ? 1 : 0;
  }
  atomicAdd(&cnt[0], conv);  // integer sums: order-independent
  if constexpr (FIXED) atomicAdd(&cnt[1], counted);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double total = static_cast<double>(FIXED ? cnt[1] : off[a + 1] - off[a]);
    ratio[a] = static_cast<double>(cnt[0]) / total;
  }
}

hipError_t launch_conv_ratio(int num_agents, const int* off, const int* idx, const double* w, double* ratio,
                             const unsigned char* fixed, hipStream_t stream) {
  if (num_agents == 0) return hipSuccess;
  if (fixed)
    k_conv_ratio<true><<<num_agents, kThreads, 0, stream>>>(off, idx, w, ratio, fixed);
  else
    k_conv_ratio<false><<<num_agents, kThreads, 0, stream>>>(off, idx, w, ratio, nullptr);
  return hipGetLastError();
}

// dpgo_rbcd_set_weights: one thread per destination of one colour.  The destinations are, in this order, the colour
// problem's n_prob edge weights (w_prob), the n_g G entries' weights (w_g), then -- only when flags are given --
// one flag per GNC entry (fix_gnc, n_gnc) and one per problem edge (fix_prob, n_prob: what k_conv_ratio reads).
// src holds the graph edge of every destination of the first three ranges, destination-ordered; the fourth reuses
// the first range's.  Reads gather from the graph-order arrays w / fixed, stores are contiguous.
__global__ __launch_bounds__(kThreads) void k_set_weights(SetWeights s, const double* __restrict__ w,
                                                          const unsigned char* __restrict__ fixed) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int n_w = s.n_prob + s.n_g;
  if (t < s.n_prob) {
    s.w_prob[t] = w[s.src[t]];
  } else if (t < n_w) {
    s.w_g[t - s.n_prob] = w[s.src[t]];
  } else if (fixed == nullptr) {
    return;
  } else if (t < n_w + s.n_gnc) {
    s.fix_gnc[t - n_w] = fixed[s.src[t]];
  } else if (t < n_w + s.n_gnc + s.n_prob) {
    const int u = t - n_w - s.n_gnc;
    s.fix_prob[u] = fixed[s.src[u]];
  }
}

hipError_t launch_set_weights(const SetWeights& s, const double* w, const unsigned char* fixed, hipStream_t stream) {
  const long total = static_cast<long>(s.n_prob) + s.n_g + (fixed ? static_cast<long>(s.n_gnc) + s.n_prob : 0);
  if (total == 0) return hipSuccess;
  const int grid = static_cast<int>((total + kThreads - 1) / kThreads);
  k_set_weights<<<grid, kThreads, 0, stream>>>(s, w, fixed);
  return hipGetLastError();
}

// w per slot (scatter of the edge-order weights) for the diagonal pass
__global__ __launch_bounds__(kThreads) void k_weights_to_slots(int m, const int* __restrict__ slot_of_edge,
                                                               const double* __restrict__ w,
                                                               double* __restrict__ wslot) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < m) wslot[slot_of_edge[e]] = w[e];
}

// ------------------------------------------------------------------------------------------
// Exact preconditioner (QuadraticProblem::PreConditioner with the Cholesky factor of Q + 0.1 I,
// src/QuadraticProblem.cpp:37-41, 75-87): supernodal triangular solves as dense panel products
// (chol_internal.h: Panel = [L_SS^-1 ; L_RS L_SS^-1] per supernode).  In row form the r right-hand
// sides of scalar row c = pose j column k are the r doubles of column k of pose block j (the engine's
// layout), so every "vector" element is r doubles.  One launch per tree level and sweep:
//   k_sn_assemble  frontal vector f of every supernode of the level: [rhs_S ; 0_R] + its children's
//                  update vectors (extend-add as a gather, children in order: deterministic)
//   k_sn_fwd       per (supernode, row tile): y_S = L_SS^-1 f_S into y; u = f_R - (L_RS L_SS^-1) f_S
//   k_sn_bwd       per (supernode, column tile): x_S = L_SS^-T y_S - (L_RS L_SS^-1)^T x_R into x
// A workgroup streams its panel tiles (row-major 64 x 64 scalars) once; thread (rq, cq) = (t >> 4,
// t & 15) owns rows 4 rq .. 4 rq + 3 and columns 4 cq .. 4 cq + 3 of every tile, with the tile's 64
// vector elements staged in LDS; the next tile's 16 panel values are loaded before the current ones
// are consumed.  Memory-bound: 8 bytes of panel per 2 r flops.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int sn_pad_dev(int scalars) { return (scalars + kSnTileDev - 1) / kSnTileDev * kSnTileDev; }
__device__ __forceinline__ long sn_tile_dev(int ns, int I, int J) {
  return I < ns ? static_cast<long>(I) * (I + 1) / 2 + J
                : static_cast<long>(ns) * (ns + 1) / 2 + static_cast<long>(I - ns) * ns + J;
}

// Rows 4 rq .. 4 rq + 3, columns 4 cq .. 4 cq + 3 of a tile (plain loads: k_sn_bwd's two-deep pipeline, which
// measured faster than the three-deep buffer-load one there: 226 vs 253 us per level launch at C5)
__device__ __forceinline__ void sn_load_tile(const double* __restrict__ tile, int rq, int cq, double (&p)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f64x2* src = reinterpret_cast<const f64x2*>(tile + (rq * 4 + i) * kSnTileDev + cq * 4);
    const f64x2 a = src[0], c = src[1];
    p[i][0] = a.x;
    p[i][1] = a.y;
    p[i][2] = c.x;
    p[i][3] = c.y;
  }
}

// Rows 4 rq .. 4 rq + 3, columns 4 cq .. 4 cq + 3 of a panel tile, by raw buffer loads (byte offset of the
// tile < 4 GiB: a node's panel is checked
// on the host): intrinsic loads stay where the software pipeline issues them (plain loads of a loop-carried
// register set are folded into one load of a phi of the addresses at the point of use)
__device__ __forceinline__ void sn_load_tile_buf(__amdgpu_buffer_rsrc_t r, unsigned tile_byte, int rq, int cq,
                                                 double (&p)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned o = tile_byte + 8u * static_cast<unsigned>((rq * 4 + i) * kSnTileDev + cq * 4);
    const f64x2 a = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(r, o, 0, 0));
    const f64x2 c = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(r, o + 16u, 0, 0));
    p[i][0] = a.x;
    p[i][1] = a.y;
    p[i][2] = c.x;
    p[i][3] = c.y;
  }
}

// A narrow supernode's compact panel (SnView::cpanel): buffer resource bounded by the node's bytes, so an offset of
// 0x80000000 (a padding row or column) loads exact zeros -- the tile path's stored padding -- with no branch
struct SnCompact {
  __amdgpu_buffer_rsrc_t r;
  int sb, tb, ld;
};
// The item's record (SnView::desc): one load
__device__ __forceinline__ SnItem sn_item(const SnView& v, const int2* items) {
  return v.desc[(items - v.items_base) + static_cast<long>(blockIdx.x)];
}
__device__ __forceinline__ bool sn_item_skipped(const SnView& v, const SnItem& d) {
  return v.node_agent && (agent_skipped(v.state, v.flag_kind, 0, d.agent) || (v.ident && v.ident[d.agent]));
}

__device__ __forceinline__ SnCompact sn_compact_view(const SnView& v, long coff, int sb, int tb) {
  const int ld = sn_compact_ld(sb);
  return SnCompact{__builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(v.cpanel + coff), static_cast<short>(0),
                                                     8 * (sb + tb) * ld, 0x00020000),
                   sb, tb, ld};
}
// Rows 4 rq .. 4 rq + 3, columns 4 cq .. 4 cq + 3 of logical tile (I, J) (the tile path's numbering: row tiles I < ns
// of the S part, then the R part's) from the compact matrix
__device__ __forceinline__ void sn_load_tile_cmp(const SnCompact& cm, int ns, int I, int J, int rq, int cq,
                                                 double (&p)[4][4]) {
  const int col = J * kSnTileDev + cq * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int prow = (I < ns ? I : I - ns) * kSnTileDev + rq * 4 + i;  // row inside the S or the R part
    const bool ok = (I < ns ? prow < cm.sb : prow < cm.tb) && col < cm.ld;
    const int cr = I < ns ? prow : cm.sb + prow;
    const unsigned o = ok ? 8u * static_cast<unsigned>(cr * cm.ld + col) : 0x80000000u;
    const f64x2 a = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(cm.r, o, 0, 0));
    const f64x2 c = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(cm.r, o + 16u, 0, 0));
    p[i][0] = a.x;
    p[i][1] = a.y;
    p[i][2] = c.x;
    p[i][3] = c.y;
  }
}

// The sweeps' cross-lane sums by DPP / permlane swaps (row16_sum, lane_xor16 / 32: bitwise __shfl_xor's) instead of
// ds_bpermute; -DDPGO_SN_DPP_SUMS=0 restores the shuffles (A/B)
#ifndef DPGO_SN_DPP_SUMS
#define DPGO_SN_DPP_SUMS 1
#endif
constexpr bool kSnDppSums = DPGO_SN_DPP_SUMS != 0;

// A/B probe only (-DDPGO_SN_ACQUIRE_TEST): an agent-scope acquire (L2 invalidate) at the start of every supernodal
// kernel, to test whether a wrong exact-preconditioner result with contiguous panel memory is a stale L2 line
#ifdef DPGO_SN_ACQUIRE_TEST
#define DPGO_SN_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent")
#else
#define DPGO_SN_ACQUIRE() \
  do {                    \
  } while (0)
#endif

// The compact copy of narrow supernodes' panels: item (node, block of 64 compact rows); compact row cr < sb is S row
// cr, row sb + q is R row q; column c < sb (columns sb .. ld - 1 are zero)
__global__ __launch_bounds__(kThreads) void k_sn_compact(int b, const double* __restrict__ panel,
                                                         const long* __restrict__ panel_off, const int* __restrict__ sv,
                                                         const int* __restrict__ tv, const long* __restrict__ cpanel_off,
                                                         double* __restrict__ cpanel, const int2* __restrict__ items) {
  DPGO_SN_ACQUIRE();
  const int2 it = items[blockIdx.x];
  const int node = it.x;
  const int sb = sv[node] * b, tb = tv[node] * b, ld = sn_compact_ld(sb), Sp = sn_pad_dev(sb), ns = Sp / kSnTileDev;
  const double* __restrict__ src = panel + panel_off[node];
  double* __restrict__ dst = cpanel + cpanel_off[node];
  const int r0 = it.y * kSnTileDev, r1 = min(sb + tb, r0 + kSnTileDev);
  for (int x = threadIdx.x; x < (r1 - r0) * ld; x += kThreads) {
    const int cr = r0 + x / ld, c = x - (x / ld) * ld;
    double val = 0.0;
    if (c < sb) {
      const int pr = cr < sb ? cr : Sp + (cr - sb);  // padded row
      const int I = pr / kSnTileDev, J = c / kSnTileDev;
      val = src[sn_tile_dev(ns, I, J) * (kSnTileDev * kSnTileDev) + (pr - I * kSnTileDev) * kSnTileDev +
                (c - J * kSnTileDev)];
    }
    dst[static_cast<long>(cr) * ld + c] = val;
  }
}

template <int R>
__global__ __launch_bounds__(kThreads) void k_sn_assemble(SnView v, const int2* __restrict__ items, int b,
                                                          const double* __restrict__ rhs) {
  DPGO_SN_ACQUIRE();
  const int2 it = items[blockIdx.x];
  if (v.node_agent && (agent_skipped(v.state, v.flag_kind, 0, v.node_agent[it.x]) ||
                       (v.ident && v.ident[v.node_agent[it.x]]))) return;
  const int node = it.x, row = it.y * kThreads + static_cast<int>(threadIdx.x);
  const int s = v.s[node], t = v.t[node], sb = s * b, tb = t * b, Sp = sn_pad_dev(sb), Rp = sn_pad_dev(tb);
  if (row >= Sp + Rp) return;
  double val[R];
#pragma unroll
  for (int a = 0; a < R; ++a) val[a] = 0.0;
  int pos = -1, k = 0;
  if (row < Sp) {
    if (row < sb) {
      pos = row / b;
      k = row - pos * b;
      const double* src = rhs + (static_cast<long>(v.poses[v.poses_off[node] + pos]) * b + k) * R;
#pragma unroll
      for (int a = 0; a < R; ++a) val[a] = src[a];
    }
  } else if (row - Sp < tb) {
    const int rr = row - Sp;
    pos = s + rr / b;
    k = rr - (rr / b) * b;
  }
  if (pos >= 0) {
    const int* cp = v.cpos + v.cpos_off[node] + pos;
    for (int e = cp[0]; e < cp[1]; ++e) {
      const int2 ce = v.contrib[e];
      const double* src = v.U + v.u_off[ce.x] + (static_cast<long>(ce.y) * b + k) * R;
#pragma unroll
      for (int a = 0; a < R; ++a) val[a] += src[a];
    }
  }
  double* dst = v.F + v.f_off[node] + static_cast<long>(row) * R;
#pragma unroll
  for (int a = 0; a < R; ++a) dst[a] = val[a];
}

// a tile's 64 vector elements (64 R doubles) through registers: element e = tid + 256 i, i < kSnVecRegs
constexpr int kSnVecRegs = (kSnTileDev * 8 + kThreads - 1) / kThreads;  // enough for R <= 8

template <int R>
__global__ __launch_bounds__(kThreads) void k_sn_fwd(SnView v, const int2* __restrict__ items, int b,
                                                     double* __restrict__ y) {
  DPGO_SN_ACQUIRE();
  __shared__ double sfl[4 * kSnTileDev * R];  // triple-buffered frontal chunks, then the row tile's f rows (f_R)
  __shared__ int spz[kSnTileDev];                // the row tile's pose ids (S rows)
  const SnItem d = sn_item(v, items);
  if (sn_item_skipped(v, d)) return;
  constexpr int kTileD = kSnTileDev * kSnTileDev, kChunk = kSnTileDev * R;
  double (*sf)[kChunk] = reinterpret_cast<double (*)[kChunk]>(sfl);
  double* __restrict__ sfr = sfl + 3 * kChunk;
  const int I = d.tile;
  const int s = d.s, t = d.t, sb = s * b, tb = t * b, Sp = sn_pad_dev(sb), ns = Sp / kSnTileDev;
  const double* __restrict__ f = v.F + d.f_off;
  const double* __restrict__ panel = v.panel + d.panel_off;
  const int* __restrict__ pz = v.poses + d.poses_off;
  const int tid = static_cast<int>(threadIdx.x), rq = tid >> 4, cq = tid & 15;
  // the epilogue's operands (the S rows' pose ids, or the R rows' f values) staged into LDS with chunk 0: the
  // workgroup's outputs then wait on no load after the sweep
  if (I < ns) {
    const int row = I * kSnTileDev + tid;
    if (tid < kSnTileDev && row < sb) spz[tid] = pz[row / b];
  } else {
    for (int e = tid; e < kChunk; e += kThreads) sfr[e] = f[static_cast<long>(I) * kChunk + e];
  }
  double acc[4][R];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int a = 0; a < R; ++a) acc[i][a] = 0.0;
  const int nJ = I < ns ? I + 1 : ns;
  // software pipeline: tiles J + 1 and J + 2's panel values are loaded into registers and their frontal chunks
  // staged in LDS while tile J is consumed (one barrier per tile)
  double p[4][4], pn[4][4], pm[4][4], fv[kSnVecRegs];
  auto load_chunk = [&](int J) {
#pragma unroll
    for (int i = 0; i < kSnVecRegs; ++i) {
      const int e = tid + i * kThreads;
      if (e < kChunk) fv[i] = f[static_cast<long>(J) * kChunk + e];
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kSnVecRegs; ++i) {
      const int e = tid + i * kThreads;
      if (e < kChunk) sf[buf][e] = fv[i];
    }
  };
  auto consume = [&](const double (&pt)[4][4], int buf) {
    const double* cf = sf[buf];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double fc[R];
#pragma unroll
      for (int a = 0; a < R; ++a) fc[a] = cf[(cq * 4 + c) * R + a];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int a = 0; a < R; ++a) acc[i][a] = fma(pt[i][c], fc[a], acc[i][a]);
    }
  };
  const __amdgpu_buffer_rsrc_t rp = buf_rsrc(panel);
  auto tile = [&](int J) { return 8u * static_cast<unsigned>(sn_tile_dev(ns, I, J) * kTileD); };
  // (the tiles even for a narrow node of a mixed level: the compact path's offsets cost this three-deep pipeline its
  // third wave -- 172 VGPRs; k_sn_fwd_small and k_sn_bwd read narrow nodes compact)
  auto load_tile = [&](int J, double (&pt)[4][4]) { sn_load_tile_buf(rp, tile(J), rq, cq, pt); };
  // Sub-step J: store chunk J + 1 (loaded one sub-step earlier; its wait is for loads issued before tile J + 1's),
  // issue chunk J + 2 and tile J + 2, consume tile J: tiles J + 1 and J + 2 stay in flight while tile J is
  // consumed.  Three register sets (tile J in set J % 3), chunk J in LDS buffer J % 3, one barrier per tile.
  if (nJ > 0) {
    load_chunk(0);
    load_tile(0, p);
    store_chunk(0);
  }
  if (nJ > 1) {
    load_chunk(1);
    load_tile(1, pn);
  }
  __syncthreads();
  auto sub_step = [&](int J, const double (&pc)[4][4], double (&pnext)[4][4], int bc, int b1) {
    if (J + 1 < nJ) store_chunk(b1);
    if (J + 2 < nJ) {
      load_chunk(J + 2);
      load_tile(J + 2, pnext);
    }
    consume(pc, bc);
    __syncthreads();  // chunk J + 1 visible; every read of buffer bc done before chunk J + 3 lands there
  };
  for (int J = 0; J < nJ; J += 3) {
    sub_step(J, p, pm, 0, 1);
    if (J + 1 >= nJ) break;
    sub_step(J + 1, pn, p, 1, 2);
    if (J + 2 >= nJ) break;
    sub_step(J + 2, pm, pn, 2, 0);
  }
  // sum over the 16 column groups (lanes cq = 0..15 of a 16-lane group, fixed order)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int a = 0; a < R; ++a) {
      double x = acc[i][a];
      if constexpr (kSnDppSums) {
        x = row16_sum(x);
      } else {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) x += __shfl_xor(x, off, 64);
      }
      acc[i][a] = x;
    }
  if (cq != 0) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = I * kSnTileDev + rq * 4 + i;
    if (row < sb) {  // y_S
      const int pos = row / b, k = row - pos * b;
      double* dst = y + (static_cast<long>(spz[rq * 4 + i]) * b + k) * R;
#pragma unroll
      for (int a = 0; a < R; ++a) dst[a] = acc[i][a];
    } else if (row >= Sp && row - Sp < tb) {  // update u = f_R - M f_S
      const double* fr = sfr + (rq * 4 + i) * R;
      double* dst = v.U + d.u_off + static_cast<long>(row - Sp) * R;
#pragma unroll
      for (int a = 0; a < R; ++a) dst[a] = fr[a] - acc[i][a];
    }
  }
}

// Forward sweep, narrow supernodes (ns <= kSnSmallNs S column tiles: the deep levels' many small separators, whose
// row tiles are one or two panel tiles long): the same item (node, row tile I), products and order as k_sn_fwd, but
// with no pipeline to fill -- every load of the workgroup (epilogue operands, the <= 2 frontal chunks, the <= 2
// tiles) is issued at once and waited for once -- in about half k_sn_fwd's registers, so more workgroups (and bytes)
// are in flight per CU on the levels where each streams only 32-64 KB.
#ifndef DPGO_SNF_SMALL_WAVES
#define DPGO_SNF_SMALL_WAVES 1  // k_sn_fwd_small's occupancy hint (waves per SIMD; 1 = none)
#endif
template <int R>
__global__ __launch_bounds__(kThreads, DPGO_SNF_SMALL_WAVES) void k_sn_fwd_small(SnView v, const int2* __restrict__ items, int b,
                                                           double* __restrict__ y) {
  DPGO_SN_ACQUIRE();
  constexpr int kTileD = kSnTileDev * kSnTileDev, kChunk = kSnTileDev * R;
  constexpr int KV = (kSnSmallNs * kChunk + kThreads - 1) / kThreads;
  __shared__ double sf[kSnSmallNs * kChunk];  // frontal chunks 0 .. nJ - 1
  __shared__ double sfr[kChunk];               // the row tile's f rows (f_R)
  __shared__ int spz[kSnTileDev];              // the row tile's pose ids (S rows)
  const SnItem d = sn_item(v, items);
  if (sn_item_skipped(v, d)) return;
  const int I = d.tile;
  const int s = d.s, t = d.t, sb = s * b, tb = t * b, Sp = sn_pad_dev(sb), ns = Sp / kSnTileDev;
  const double* __restrict__ f = v.F + d.f_off;
  const double* __restrict__ panel = v.panel + d.panel_off;
  const int* __restrict__ pz = v.poses + d.poses_off;
  const int tid = static_cast<int>(threadIdx.x), rq = tid >> 4, cq = tid & 15;
  const int nJ = I < ns ? I + 1 : ns;  // <= kSnSmallNs (host: ns <= kSnSmallNs)
  if (I < ns) {
    const int row = I * kSnTileDev + tid;
    if (tid < kSnTileDev && row < sb) spz[tid] = pz[row / b];
  } else {
    for (int e = tid; e < kChunk; e += kThreads) sfr[e] = f[static_cast<long>(I) * kChunk + e];
  }
  double fv[KV];
#pragma unroll
  for (int i = 0; i < KV; ++i) {
    const int e = tid + i * kThreads;
    if (e < nJ * kChunk) fv[i] = f[e];
  }
  const __amdgpu_buffer_rsrc_t rp = buf_rsrc(panel);
  double p[kSnSmallNs][4][4];
  const long coff = d.cpanel_off;  // a narrow node's compact panel (workgroup-uniform)
  if (coff >= 0) {
    const SnCompact cm = sn_compact_view(v, coff, sb, tb);
#pragma unroll
    for (int J = 0; J < kSnSmallNs; ++J)
      if (J < nJ) sn_load_tile_cmp(cm, ns, I, J, rq, cq, p[J]);
  } else {
#pragma unroll
    for (int J = 0; J < kSnSmallNs; ++J)
      if (J < nJ) sn_load_tile_buf(rp, 8u * static_cast<unsigned>(sn_tile_dev(ns, I, J) * kTileD), rq, cq, p[J]);
  }
#pragma unroll
  for (int i = 0; i < KV; ++i) {
    const int e = tid + i * kThreads;
    if (e < nJ * kChunk) sf[e] = fv[i];
  }
  __syncthreads();
  double acc[4][R];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int a = 0; a < R; ++a) acc[i][a] = 0.0;
#pragma unroll
  for (int J = 0; J < kSnSmallNs; ++J) {
    if (J >= nJ) break;
    const double* cf = sf + J * kChunk;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double fc[R];
#pragma unroll
      for (int a = 0; a < R; ++a) fc[a] = cf[(cq * 4 + c) * R + a];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int a = 0; a < R; ++a) acc[i][a] = fma(p[J][i][c], fc[a], acc[i][a]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int a = 0; a < R; ++a) {
      double x = acc[i][a];
      if constexpr (kSnDppSums) {
        x = row16_sum(x);
      } else {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) x += __shfl_xor(x, off, 64);
      }
      acc[i][a] = x;
    }
  if (cq != 0) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = I * kSnTileDev + rq * 4 + i;
    if (row < sb) {
      const int pos = row / b, k = row - pos * b;
      double* dst = y + (static_cast<long>(spz[rq * 4 + i]) * b + k) * R;
#pragma unroll
      for (int a = 0; a < R; ++a) dst[a] = acc[i][a];
    } else if (row >= Sp && row - Sp < tb) {
      const double* fr = sfr + (rq * 4 + i) * R;
      double* dst = v.U + d.u_off + static_cast<long>(row - Sp) * R;
#pragma unroll
      for (int a = 0; a < R; ++a) dst[a] = fr[a] - acc[i][a];
    }
  }
}

#ifndef DPGO_SNB_WAVES
#define DPGO_SNB_WAVES 1  // k_sn_bwd's occupancy hint (waves per SIMD; 1 = none)
#endif
template <int R>
__global__ __launch_bounds__(kThreads, DPGO_SNB_WAVES) void k_sn_bwd(SnView v, const int2* __restrict__ items, int b,
                                                     const double* __restrict__ y, double* __restrict__ x) {
  DPGO_SN_ACQUIRE();
  __shared__ double sg[2][kSnTileDev * R];  // double-buffered [y_S ; -x_R] chunks
  __shared__ double red[kThreads / 64][16][4 * R];
  const SnItem d = sn_item(v, items);
  if (sn_item_skipped(v, d)) return;
  const int J = d.tile;
  const int s = d.s, t = d.t, sb = s * b, tb = t * b, Sp = sn_pad_dev(sb), Rp = sn_pad_dev(tb);
  const int ns = Sp / kSnTileDev, nI = (Sp + Rp) / kSnTileDev;
  const double* __restrict__ panel = v.panel + d.panel_off;
  const int* __restrict__ poses = v.poses + d.poses_off;
  const int tid = static_cast<int>(threadIdx.x), rq = tid >> 4, cq = tid & 15;
  double acc[4][R];  // columns 4 cq + c
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int a = 0; a < R; ++a) acc[c][a] = 0.0;
  constexpr int kTileD = kSnTileDev * kSnTileDev, kChunk = kSnTileDev * R;
  double p[4][4], pn[4][4], gv[kSnVecRegs];
  // rows of tile I: y_S on the S part, -x_R on the R part (ancestors' solution), 0 on padding
  auto load_chunk = [&](int I) {
#pragma unroll
    for (int i = 0; i < kSnVecRegs; ++i) {
      const int e = tid + i * kThreads;
      if (e >= kChunk) continue;
      const int rl = e / R, a = e - rl * R, row = I * kSnTileDev + rl;
      double g = 0.0;
      if (row < sb) {
        const int pos = row / b, k = row - pos * b;
        g = y[(static_cast<long>(poses[pos]) * b + k) * R + a];
      } else if (row >= Sp && row - Sp < tb) {
        const int rr = row - Sp, q = rr / b, k = rr - q * b;
        g = -x[(static_cast<long>(poses[s + q]) * b + k) * R + a];
      }
      gv[i] = g;
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kSnVecRegs; ++i) {
      const int e = tid + i * kThreads;
      if (e < kChunk) sg[buf][e] = gv[i];
    }
  };
  const long coff = d.cpanel_off;  // a narrow node's compact panel (workgroup-uniform)
  const SnCompact cm = coff >= 0 ? sn_compact_view(v, coff, sb, tb) : SnCompact{buf_rsrc(panel), 0, 0, 0};
  auto load_tile = [&](int I, double (&pt)[4][4]) {
    if (coff >= 0)
      sn_load_tile_cmp(cm, ns, I, J, rq, cq, pt);
    else
      sn_load_tile(panel + sn_tile_dev(ns, I, J) * kTileD, rq, cq, pt);
  };
  if (J < nI) {
    load_tile(J, p);
    load_chunk(J);
    store_chunk(0);
  }
  __syncthreads();
  for (int I = J; I < nI; ++I) {
    const bool more = I + 1 < nI;
    if (more) {
      load_tile(I + 1, pn);
      load_chunk(I + 1);
    }
    const double* cg = sg[(I - J) & 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double gi[R];
#pragma unroll
      for (int a = 0; a < R; ++a) gi[a] = cg[(rq * 4 + i) * R + a];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int a = 0; a < R; ++a) acc[c][a] = fma(p[i][c], gi[a], acc[c][a]);
    }
    if (more) store_chunk((I + 1 - J) & 1);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 4; ++c) p[i][c] = pn[i][c];
  }
  // sum over the 16 row groups: the 4 of a wave (lane bits 4, 5), then the 4 waves in order
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int a = 0; a < R; ++a) {
      double z = acc[c][a];
      z += kSnDppSums ? lane_xor16(z) : __shfl_xor(z, 16, 64);
      z += kSnDppSums ? lane_xor32(z) : __shfl_xor(z, 32, 64);
      acc[c][a] = z;
    }
  if (lane < 16) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int a = 0; a < R; ++a) red[wave][lane][c * R + a] = acc[c][a];
  }
  __syncthreads();
  if (tid >= 16) return;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int col = J * kSnTileDev + tid * 4 + c;
    if (col >= sb) continue;
    const int pos = col / b, k = col - pos * b;
    double* dst = x + (static_cast<long>(poses[pos]) * b + k) * R;
#pragma unroll
    for (int a = 0; a < R; ++a)
      dst[a] = ((red[0][tid][c * R + a] + red[1][tid][c * R + a]) + red[2][tid][c * R + a]) + red[3][tid][c * R + a];
  }
}

// ------------------------------------------------------------------------------------------
// Numeric supernodal factorisation on the device (SnFactorView): one workgroup per supernode of one tree level.
// Dense frontal work in 64 x 64 tiles staged in LDS; the tile products run on the fp64 matrix cores
// (v_mfma_f64_16x16x4f64: A lane l = A[l & 15][k = l >> 4], B lane l = B[k = l >> 4][l & 15], C/D lane l,
// register q = C[(l >> 4) + 4 q][l & 15]), one 16-row strip of the output tile per wave.
// ------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int kFT = kSnTileDev;  // 64
constexpr int kFLD = kFT + 1;    // LDS tile stride (doubles)

// acc (rows r0 .. r0 + 15 of a 64 x 64 tile, four 16-column blocks) += sign * A(strip) . op(B): op(B)[k][c] =
// B[c][k] (BT) or B[k][c]; A and B are LDS tiles
template <bool BT>
__device__ __forceinline__ void mfma_strip(f64x4 (&acc)[4], const double* As, const double* Bs, int r0, double sign) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
#pragma unroll 4
  for (int k0 = 0; k0 < kFT; k0 += 4) {
    const double a = sign * As[(r0 + lr) * kFLD + k0 + lk];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int c = cb * 16 + lr;
      const double bv = BT ? Bs[c * kFLD + k0 + lk] : Bs[(k0 + lk) * kFLD + c];
      acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[cb], 0, 0, 0);
    }
  }
}

// The A operand of mfma_strip read straight from a global tile into registers (the wave's strip: row r0 + (l & 15),
// columns 4 i + (l >> 4)), so a kernel needs only B's LDS tile: half the LDS, twice the resident workgroups
__device__ __forceinline__ void sn_strip_a(double (&a)[kFT / 4], const double* __restrict__ Ag, long ld, int r0) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < kFT / 4; ++i) a[i] = Ag[(r0 + (l & 15)) * ld + 4 * i + (l >> 4)];
}
// acc += sign * A(strip, registers) . op(B) (B an LDS tile): the same MFMA sequence as mfma_strip<BT>
template <bool BT = true>
__device__ __forceinline__ void mfma_strip_ra(f64x4 (&acc)[4], const double (&a)[kFT / 4], const double* Bs,
                                              double sign) {
  const int l = threadIdx.x & 63, lr = l & 15, lk = l >> 4;
#pragma unroll
  for (int k0 = 0; k0 < kFT; k0 += 4) {
    const double av = sign * a[k0 / 4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int c = cb * 16 + lr;
      const double bv = BT ? Bs[c * kFLD + k0 + lk] : Bs[(k0 + lk) * kFLD + c];
      acc[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[cb], 0, 0, 0);
    }
  }
}

// global 64 x 64 tile (row-major, leading dimension ld) <-> LDS tile, all threads
__device__ __forceinline__ void sn_tile_to_lds(double* Ls, const double* __restrict__ g, long ld) {
  for (int x = threadIdx.x; x < kFT * kFT; x += kThreads) {
    const int i = x / kFT, j = x % kFT;
    Ls[i * kFLD + j] = g[i * ld + j];
  }
}
// the wave's strip of a global tile into / out of the MFMA accumulator layout
__device__ __forceinline__ void sn_strip_load(f64x4 (&acc)[4], const double* __restrict__ g, long ld, int r0) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[cb][q] = g[(r0 + (l >> 4) + 4 * q) * ld + cb * 16 + (l & 15)];
}
__device__ __forceinline__ void sn_strip_store(const f64x4 (&acc)[4], double* __restrict__ g, long ld, int r0) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) g[(r0 + (l >> 4) + 4 * q) * ld + cb * 16 + (l & 15)] = acc[cb][q];
}

// In-place lower Cholesky of the LDS tile (right-looking, one column per step); a non-positive pivot sets *bad
__device__ void sn_potrf_lds(double* A, int* bad) {
  const int tid = threadIdx.x;
  for (int j = 0; j < kFT; ++j) {
    if (tid == 0) {
      const double d = A[j * kFLD + j];
      if (!(d > 0.0)) *bad = 1;
      A[j * kFLD + j] = sqrt(d > 0.0 ? d : 1.0);
    }
    __syncthreads();
    const double inv = 1.0 / A[j * kFLD + j];
    if (tid > j && tid < kFT) A[tid * kFLD + j] *= inv;
    __syncthreads();
    const int i = tid & 63;
    if (i > j) {
      const double lij = A[i * kFLD + j];
      for (int k = j + 1 + (tid >> 6); k <= i; k += 4) A[i * kFLD + k] -= lij * A[k * kFLD + j];
    }
    __syncthreads();
  }
}
// Linv = L^-1 (lower) of the lower LDS tile L, column c by thread c (forward substitution); upper part zeroed
__device__ void sn_trtri_lds(const double* L, double* Linv) {
  const int c = threadIdx.x;
  if (c < kFT) {
    for (int i = 0; i < c; ++i) Linv[i * kFLD + c] = 0.0;
    Linv[c * kFLD + c] = 1.0 / L[c * kFLD + c];
    for (int i = c + 1; i < kFT; ++i) {
      double acc = 0.0;
      for (int k = c; k < i; ++k) acc = fma(L[i * kFLD + k], Linv[k * kFLD + c], acc);
      Linv[i * kFLD + c] = -acc / L[i * kFLD + i];
    }
  }
  __syncthreads();
}

// frontal row of (pose position pos, component k): S poses first, then R poses after the S padding
__device__ __forceinline__ int sn_frow(int pos, int k, int s, int b, int Sp) {
  return pos < s ? pos * b + k : Sp + (pos - s) * b + k;
}

template <int B>
__global__ __launch_bounds__(kThreads) void k_sn_factor(SnFactorView v) {
  DPGO_SN_ACQUIRE();
  constexpr int D = B - 1, RW = edge_rec_width(D), DW = diag_width(D);
  __shared__ double As[kFT * kFLD], Bs[kFT * kFLD];
  __shared__ int s_bad;
  const int g = v.nodes[blockIdx.x];
  const int s = v.s[g], t = v.t[g], sb = s * B, tb = t * B, Sp = sn_pad_dev(sb), Rp = sn_pad_dev(tb);
  const int M = Sp + Rp, NT = M / kFT, ns = Sp / kFT;
  const long ld = M;
  double* __restrict__ F = v.F + v.f_off[g];
  double* __restrict__ panel = v.panel + v.panel_off[g];
  const int tid = threadIdx.x, wave = tid >> 6;
  if (tid == 0) s_bad = 0;
  // ---- assembly: zero the lower triangle (identity on the padding rows), original entries, children
  const int lane = tid & 63;
  for (int i = wave; i < M; i += 4) {  // a row per wave, its columns over the lanes
    const bool pad = (i >= sb && i < Sp) || i >= Sp + tb;
    for (int j = lane; j <= i; j += 64) F[static_cast<long>(i) * ld + j] = (i == j && pad) ? 1.0 : 0.0;
  }
  __syncthreads();
  const int* poses = v.poses + v.poses_off[g];
  for (int e = v.ent_off[g] + tid; e < v.ent_off[g + 1]; e += kThreads) {
    const SnEntry en = v.ent[e];
    double blk[B][B];  // Q block (pose q, pose p)
    if (en.q == en.p) {
      const double* dg = v.diag + static_cast<long>(poses[en.p]) * DW;
#pragma unroll
      for (int i = 0; i < B; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j) blk[i][j] = dg[sym_index<B>(i, j)] + (i == j ? v.shift : 0.0);
    } else {
#pragma unroll
      for (int i = 0; i < B; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j) blk[i][j] = 0.0;
      for (int k = en.s0; k < en.s1; ++k) {  // in source order (duplicate measurements of one pair)
        const int code = v.src[k];
        const double* m = v.rec + static_cast<long>(code >> 1) * RW;
#pragma unroll
        for (int i = 0; i < B; ++i)
#pragma unroll
          for (int j = 0; j < B; ++j) blk[i][j] -= (code & 1) ? m[4 * j + i] : m[4 * i + j];
      }
    }
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const long row = sn_frow(en.q, i, s, B, Sp);
#pragma unroll
      for (int j = 0; j < B; ++j) {
        const int col = en.p * B + j;
        if (row >= col) F[row * ld + col] += blk[i][j];
      }
    }
  }
  __syncthreads();
  for (int ci = v.ch_off[g]; ci < v.ch_off[g + 1]; ++ci) {  // children in order, one at a time
    const int c = v.ch[ci];
    const int tcb = v.t[c] * B, Spc = sn_pad_dev(v.s[c] * B);
    const long ldc = Spc + sn_pad_dev(tcb);
    const double* __restrict__ U = v.Fchild + v.f_off[c] + Spc * ldc + Spc;
    const int* tp = v.tp + v.tp_off[c];
    for (int ri = wave; ri < tcb; ri += 4) {
      const long pr = sn_frow(tp[ri / B], ri % B, s, B, Sp);
      for (int rj = lane; rj <= ri; rj += 64) {
        const long pc = sn_frow(tp[rj / B], rj % B, s, B, Sp);
        F[pr * ld + pc] += U[static_cast<long>(ri) * ldc + rj];
      }
    }
    __syncthreads();
  }
  // ---- blocked right-looking Cholesky over the S tile columns
  for (int K = 0; K < ns; ++K) {
    sn_tile_to_lds(As, F + static_cast<long>(K) * kFT * ld + K * kFT, ld);
    __syncthreads();
    sn_potrf_lds(As, &s_bad);
    sn_trtri_lds(As, Bs);
    for (int x = tid; x < kFT * kFT; x += kThreads) {
      const int i = x / kFT, j = x % kFT;
      F[(static_cast<long>(K) * kFT + i) * ld + K * kFT + j] = As[i * kFLD + j];
      // the panel's diagonal tile: L_KK^-1 with the padding zeroed
      const bool real = K * kFT + i < sb && K * kFT + j < sb;
      panel[sn_tile_dev(ns, K, K) * kFT * kFT + x] = real ? Bs[i * kFLD + j] : 0.0;
    }
    __syncthreads();
    // L_IK = F_IK L_KK^-T for every tile row below
    for (int I = K + 1; I < NT; ++I) {
      double* gt = F + static_cast<long>(I) * kFT * ld + K * kFT;
      sn_tile_to_lds(As, gt, ld);
      __syncthreads();
      f64x4 acc[4] = {};
      mfma_strip<true>(acc, As, Bs, wave * 16, 1.0);
      sn_strip_store(acc, gt, ld, wave * 16);
      __syncthreads();
    }
    // trailing update F_IJ -= L_IK L_JK^T, K < J <= I (the R block becomes the update matrix)
    for (int I = K + 1; I < NT; ++I) {
      sn_tile_to_lds(As, F + static_cast<long>(I) * kFT * ld + K * kFT, ld);
      for (int J = K + 1; J <= I; ++J) {
        sn_tile_to_lds(Bs, F + static_cast<long>(J) * kFT * ld + K * kFT, ld);
        __syncthreads();
        double* gt = F + static_cast<long>(I) * kFT * ld + J * kFT;
        f64x4 acc[4];
        sn_strip_load(acc, gt, ld, wave * 16);
        mfma_strip<true>(acc, As, Bs, wave * 16, -1.0);
        sn_strip_store(acc, gt, ld, wave * 16);
        __syncthreads();
      }
    }
  }
  if (tid == 0 && s_bad) v.not_pd[v.node_agent[g]] = 1;
  // ---- panel: Z = [I ; L_RS] L_SS^-1, tile column J from the last: Z_IJ = (B_IJ - sum_{K > J} Z_IK L_KJ) L_JJ^-1,
  // B_IJ = 0 (S rows, I != J) or L_RS (R rows); Z_IK = 0 for S rows with K > I
  for (int J = ns - 1; J >= 0; --J) {
    for (int I = J + 1; I < NT; ++I) {
      f64x4 acc[4] = {};
      if (I >= ns) sn_strip_load(acc, F + static_cast<long>(I) * kFT * ld + J * kFT, ld, wave * 16);
      const int Kmax = I < ns ? I : ns - 1;
      for (int K = J + 1; K <= Kmax; ++K) {
        const double* z = panel + sn_tile_dev(ns, I, K) * kFT * kFT;
        for (int x = tid; x < kFT * kFT; x += kThreads) As[(x / kFT) * kFLD + x % kFT] = z[x];
        sn_tile_to_lds(Bs, F + static_cast<long>(K) * kFT * ld + J * kFT, ld);
        __syncthreads();
        mfma_strip<false>(acc, As, Bs, wave * 16, -1.0);
        __syncthreads();
      }
      // acc L_JJ^-1: acc through LDS into the A-operand layout, L_JJ^-1 from the panel's diagonal tile
      {
        const int l = tid & 63;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int q = 0; q < 4; ++q) As[(wave * 16 + (l >> 4) + 4 * q) * kFLD + cb * 16 + (l & 15)] = acc[cb][q];
      }
      const double* dj = panel + sn_tile_dev(ns, J, J) * kFT * kFT;
      for (int x = tid; x < kFT * kFT; x += kThreads) Bs[(x / kFT) * kFLD + x % kFT] = dj[x];
      __syncthreads();
      f64x4 z[4] = {};
      mfma_strip<false>(z, As, Bs, wave * 16, 1.0);
      {
        const int l = tid & 63;
        double* out = panel + sn_tile_dev(ns, I, J) * kFT * kFT;
        const int rbase = I < ns ? I * kFT : (I - ns) * kFT, rlim = I < ns ? sb : tb;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int rr = wave * 16 + (l >> 4) + 4 * q, cc = cb * 16 + (l & 15);
            const bool real = rbase + rr < rlim && J * kFT + cc < sb;
            out[rr * kFT + cc] = real ? z[cb][q] : 0.0;
          }
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------
// The same factorisation tile-parallel over a level's nodes (levels with few, large supernodes: one workgroup per
// node leaves most CUs idle there): per launch one row block / entry chunk / tile of every node of the level, the
// right-looking K loop and the panel's J loop as launch sequences on the stream (FacLaunchKind).  Each tile sees
// the same operations in the same order as in k_sn_factor, so the factors agree bitwise.
// ------------------------------------------------------------------------------------------
// k_snf_asm's extend-add in batches of four positions per lane (-DDPGO_SNF_ASM_BATCH=0: one at a time)
#ifndef DPGO_SNF_ASM_BATCH
#define DPGO_SNF_ASM_BATCH 1
#endif
constexpr bool kSnfAsmBatch = DPGO_SNF_ASM_BATCH != 0;

template <int B>
__global__ __launch_bounds__(kThreads) void k_snf_asm(SnFactorView v, const int2* __restrict__ items, int phase) {
  DPGO_SN_ACQUIRE();
  constexpr int D = B - 1, RW = edge_rec_width(D), DW = diag_width(D);
  const int2 it = items[blockIdx.x];
  const int g = it.x;
  const int s = v.s[g], t = v.t[g], sb = s * B, tb = t * B, Sp = sn_pad_dev(sb), M = Sp + sn_pad_dev(tb);
  const long ld = M;
  double* __restrict__ F = v.F + v.f_off[g];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (phase == 0) {  // zero rows 64 it.y .. (identity on the padding rows)
    const int i1 = min(M, it.y * kFT + kFT);
    for (int i = it.y * kFT + wave; i < i1; i += 4) {
      const bool pad = (i >= sb && i < Sp) || i >= Sp + tb;
      for (int j = lane; j <= i; j += 64) F[static_cast<long>(i) * ld + j] = (i == j && pad) ? 1.0 : 0.0;
    }
    return;
  }
  const int* poses = v.poses + v.poses_off[g];
  if (phase == 1) {  // original entries, chunk it.y of 256
    const int e = v.ent_off[g] + it.y * kThreads + tid;
    if (e >= v.ent_off[g + 1]) return;
    const SnEntry en = v.ent[e];
    double blk[B][B];
    if (en.q == en.p) {
      const double* dg = v.diag + static_cast<long>(poses[en.p]) * DW;
#pragma unroll
      for (int i = 0; i < B; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j) blk[i][j] = dg[sym_index<B>(i, j)] + (i == j ? v.shift : 0.0);
    } else {
#pragma unroll
      for (int i = 0; i < B; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j) blk[i][j] = 0.0;
      for (int k = en.s0; k < en.s1; ++k) {
        const int code = v.src[k];
        const double* m = v.rec + static_cast<long>(code >> 1) * RW;
#pragma unroll
        for (int i = 0; i < B; ++i)
#pragma unroll
          for (int j = 0; j < B; ++j) blk[i][j] -= (code & 1) ? m[4 * j + i] : m[4 * i + j];
      }
    }
#pragma unroll
    for (int i = 0; i < B; ++i) {
      const long row = sn_frow(en.q, i, s, B, Sp);
#pragma unroll
      for (int j = 0; j < B; ++j) {
        const int col = en.p * B + j;
        if (row >= col) F[row * ld + col] += blk[i][j];
      }
    }
    return;
  }
  // phase 2 + c: child c's update matrix extend-added, its rows 64 it.y ..
  const int c = v.ch[v.ch_off[g] + phase - 2];
  const int tcb = v.t[c] * B, Spc = sn_pad_dev(v.s[c] * B);
  const long ldc = Spc + sn_pad_dev(tcb);
  const double* __restrict__ U = v.Fchild + v.f_off[c] + Spc * ldc + Spc;
  const int* tp = v.tp + v.tp_off[c];
  const int r1 = min(tcb, it.y * kFT + kFT);
  for (int ri = it.y * kFT + wave; ri < r1; ri += 4) {
    const long pr = sn_frow(tp[ri / B], ri % B, s, B, Sp);
    if constexpr (kSnfAsmBatch) {
      // four of the lane's positions per pass: every position and load issued before any add and store (the
      // positions of one row are distinct, so the batch reorders no dependent access; each entry gets the same add)
      constexpr int NB = 4;
      for (int rj0 = lane; rj0 <= ri; rj0 += NB * 64) {
        long pc[NB];
        double fu[NB], uu[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const int rj = rj0 + u * 64;
          pc[u] = rj <= ri ? sn_frow(tp[rj / B], rj % B, s, B, Sp) : 0;
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const int rj = rj0 + u * 64;
          if (rj <= ri) {
            uu[u] = U[static_cast<long>(ri) * ldc + rj];
            fu[u] = F[pr * ld + pc[u]];
          }
        }
#pragma unroll
        for (int u = 0; u < NB; ++u)
          if (rj0 + u * 64 <= ri) F[pr * ld + pc[u]] = fu[u] + uu[u];
      }
    } else {
      for (int rj = lane; rj <= ri; rj += 64) {
        const long pc = sn_frow(tp[rj / B], rj % B, s, B, Sp);
        F[pr * ld + pc] += U[static_cast<long>(ri) * ldc + rj];
      }
    }
  }
}

// kind 5 (the blocked trailing update): the tiles right of the current block of kSnfBlockK columns
constexpr int kSnfBlockK = kBK;
// kind 5 with the next K's operands loaded during the current K's MFMAs (-DDPGO_SNF5_PIPE=0: load, then multiply)
#ifndef DPGO_SNF5_PIPE
#define DPGO_SNF5_PIPE 1
#endif
constexpr bool kSnf5Pipe = DPGO_SNF5_PIPE != 0;
// kind 1's triangular inverse right-looking over all threads (-DDPGO_SNF1_RIGHT=0: one thread per column)
#ifndef DPGO_SNF1_RIGHT
#define DPGO_SNF1_RIGHT 1
#endif
constexpr bool kSnf1Right = DPGO_SNF1_RIGHT != 0;
// kind 4 (the panel tiles) pipelined the same way (-DDPGO_SNF4_PIPE=0: load, then multiply)
#ifndef DPGO_SNF4_PIPE
#define DPGO_SNF4_PIPE 1
#endif
constexpr bool kSnf4Pipe = DPGO_SNF4_PIPE != 0;
#ifndef DPGO_SNF5_WAVES
#define DPGO_SNF5_WAVES 1  // the pipelined kind 5's occupancy hint (waves per SIMD; 1 = none)
#endif

// kind 1: the diagonal tile K of every node (POTRF, its inverse into the panel); 2: L_IK = F_IK L_KK^-T, item
// (node, I); 3: F_IJ -= L_IK L_JK^T, item (node, I << 16 | J); 4: the panel's tile (I, J = param), item (node, I)
template <int B, int KIND>
__global__ __launch_bounds__(kThreads, KIND == 5 && kSnf5Pipe ? DPGO_SNF5_WAVES : 1) void k_snf_tile(SnFactorView v,
                                                                                    const int2* __restrict__ items, int P) {
  DPGO_SN_ACQUIRE();
  constexpr int kind = KIND;
  __shared__ double As[kFT * kFLD], Bs[kFT * kFLD];
  __shared__ int s_bad;
  const int2 it = items[blockIdx.x];
  const int g = it.x;
  const int s = v.s[g], t = v.t[g], sb = s * B, tb = t * B, Sp = sn_pad_dev(sb), M = Sp + sn_pad_dev(tb);
  const int NT = M / kFT, ns = Sp / kFT;
  const long ld = M;
  double* __restrict__ F = v.F + v.f_off[g];
  double* __restrict__ panel = v.panel + v.panel_off[g];
  const int tid = threadIdx.x, wave = tid >> 6;
  if constexpr (kind == 1) {
    const int K = P;
    if (tid == 0) s_bad = 0;
    sn_tile_to_lds(As, F + static_cast<long>(K) * kFT * ld + K * kFT, ld);
    __syncthreads();
    sn_potrf_lds(As, &s_bad);
    // L^-1 by sn_trtri_lds's recurrence, kept in the same tile: its strict lower part transposed into the (unused)
    // strict upper triangle, its diagonal in s_dinv -- one LDS tile instead of two
    __shared__ double s_dinv[kFT];
    if constexpr (kSnf1Right) {
      // Right-looking: the partial sum of X[i][c] (i > c, held in Bs) takes L[i][k] X[k][c] as soon as X[k][c] is
      // final, for k = c, c + 1, ... -- the column recurrence's fma chain in its order, from 0.0, so X is bitwise the
      // same; every thread works on every step instead of thread c walking column c alone
      if (tid < kFT) s_dinv[tid] = 1.0 / As[tid * kFLD + tid];
      __syncthreads();
      for (int k = 0; k < kFT; ++k) {
        if (tid < k) As[tid * kFLD + k] = -Bs[k * kFLD + tid] / As[k * kFLD + k];  // X[k][c], c = tid
        __syncthreads();
        const int w = k + 1, n = (kFT - 1 - k) * w;  // rows k + 1 .. 63, columns 0 .. k
        for (int x = tid; x < n; x += kThreads) {
          const int i = k + 1 + x / w, c = x - (x / w) * w;
          const double xk = c == k ? s_dinv[k] : As[c * kFLD + k];
          Bs[i * kFLD + c] = fma(As[i * kFLD + k], xk, c == k ? 0.0 : Bs[i * kFLD + c]);
        }
        __syncthreads();
      }
    } else {
      if (tid < kFT) {
        const int c = tid;
        const double dc = 1.0 / As[c * kFLD + c];
        s_dinv[c] = dc;
        for (int i = c + 1; i < kFT; ++i) {
          double acc = 0.0;
          for (int k = c; k < i; ++k) acc = fma(As[i * kFLD + k], k == c ? dc : As[c * kFLD + k], acc);
          As[c * kFLD + i] = -acc / As[i * kFLD + i];
        }
      }
      __syncthreads();
    }
    for (int x = tid; x < kFT * kFT; x += kThreads) {
      const int i = x / kFT, j = x % kFT;
      if (j <= i) F[(static_cast<long>(K) * kFT + i) * ld + K * kFT + j] = As[i * kFLD + j];  // L (upper unchanged)
      const bool real = K * kFT + i < sb && K * kFT + j < sb;
      const double li = j < i ? As[j * kFLD + i] : j == i ? s_dinv[i] : 0.0;
      panel[sn_tile_dev(ns, K, K) * kFT * kFT + x] = real ? li : 0.0;
    }
    if (tid == 0 && s_bad) v.not_pd[v.node_agent[g]] = 1;
    return;
  }
  if constexpr (kind == 2) {
    const int K = P, I = it.y;
    double* gt = F + static_cast<long>(I) * kFT * ld + K * kFT;
    double a[kFT / 4];
    sn_strip_a(a, gt, ld, wave * 16);
    // L_KK^-1 with its padding block (identity there; the panel stores zeros)
    const double* dk = panel + sn_tile_dev(ns, K, K) * kFT * kFT;
    for (int x = tid; x < kFT * kFT; x += kThreads) {
      const int i = x / kFT, j = x % kFT;
      const bool padi = K * kFT + i >= sb;
      Bs[i * kFLD + j] = padi ? (i == j ? 1.0 : 0.0) : dk[x];
    }
    __syncthreads();
    f64x4 acc[4] = {};
    mfma_strip_ra(acc, a, Bs, 1.0);
    sn_strip_store(acc, gt, ld, wave * 16);
    return;
  }
  if constexpr (kind == 5) {  // F_IJ -= sum_{K = P .. P + kSnfBlockK - 1, K < ns} L_IK L_JK^T, K in order
    const int I = it.y >> 16, J = it.y & 0xFFFF, K1 = min(P + kSnfBlockK, ns);
    double* gt = F + static_cast<long>(I) * kFT * ld + J * kFT;
    f64x4 acc[4];
    sn_strip_load(acc, gt, ld, wave * 16);
    if constexpr (kSnf5Pipe) {
      // K + 1's B tile loaded into registers while K's MFMAs run (its A strip right after them, in flight across the
      // barrier and the tile's LDS store): the same MFMA sequence, one LDS tile
      constexpr int kTV = kFT * kFT / kThreads;
      double a[kFT / 4], bn[kTV];
      auto load_b = [&](int K) {
        const double* g = F + static_cast<long>(J) * kFT * ld + K * kFT;
#pragma unroll
        for (int u = 0; u < kTV; ++u) {
          const int x = tid + u * kThreads, i = x / kFT, j = x % kFT;
          bn[u] = g[i * ld + j];
        }
      };
      auto store_b = [&]() {
#pragma unroll
        for (int u = 0; u < kTV; ++u) {
          const int x = tid + u * kThreads, i = x / kFT, j = x % kFT;
          Bs[i * kFLD + j] = bn[u];
        }
      };
      sn_strip_a(a, F + static_cast<long>(I) * kFT * ld + P * kFT, ld, wave * 16);
      load_b(P);
      store_b();
      __syncthreads();
      for (int K = P; K < K1; ++K) {
        const bool more = K + 1 < K1;
        if (more) load_b(K + 1);
        mfma_strip_ra(acc, a, Bs, -1.0);
        if (more) {
          sn_strip_a(a, F + static_cast<long>(I) * kFT * ld + (K + 1) * kFT, ld, wave * 16);
          __syncthreads();
          store_b();
          __syncthreads();
        }
      }
      sn_strip_store(acc, gt, ld, wave * 16);
      return;
    }
    for (int K = P; K < K1; ++K) {
      double a[kFT / 4];
      sn_strip_a(a, F + static_cast<long>(I) * kFT * ld + K * kFT, ld, wave * 16);
      sn_tile_to_lds(Bs, F + static_cast<long>(J) * kFT * ld + K * kFT, ld);
      __syncthreads();
      mfma_strip_ra(acc, a, Bs, -1.0);
      __syncthreads();
    }
    sn_strip_store(acc, gt, ld, wave * 16);
    return;
  }
  if constexpr (kind == 3) {
    const int K = P, I = it.y >> 16, J = it.y & 0xFFFF;
    double a[kFT / 4];
    sn_strip_a(a, F + static_cast<long>(I) * kFT * ld + K * kFT, ld, wave * 16);
    sn_tile_to_lds(Bs, F + static_cast<long>(J) * kFT * ld + K * kFT, ld);
    __syncthreads();
    double* gt = F + static_cast<long>(I) * kFT * ld + J * kFT;
    f64x4 acc[4];
    sn_strip_load(acc, gt, ld, wave * 16);
    mfma_strip_ra(acc, a, Bs, -1.0);
    sn_strip_store(acc, gt, ld, wave * 16);
    return;
  }
  // kind 4: Z_IJ = (B_IJ - sum_{K > J} Z_IK L_KJ) L_JJ^-1 (A strips in registers: one LDS tile)
  const int J = P, I = it.y;
  f64x4 acc[4] = {};
  if (I >= ns) sn_strip_load(acc, F + static_cast<long>(I) * kFT * ld + J * kFT, ld, wave * 16);
  const int Kmax = I < ns ? I : ns - 1;
  if (kSnf4Pipe && J + 1 <= Kmax) {
    // as kind 5: K + 1's B tile in registers while K's MFMAs run, its A strip right after them (same MFMA sequence)
    constexpr int kTV = kFT * kFT / kThreads;
    double a[kFT / 4], bn[kTV];
    auto load_b = [&](int K) {
      const double* g = F + static_cast<long>(K) * kFT * ld + J * kFT;
#pragma unroll
      for (int u = 0; u < kTV; ++u) {
        const int x = tid + u * kThreads, i = x / kFT, j = x % kFT;
        bn[u] = g[i * ld + j];
      }
    };
    auto store_b = [&]() {
#pragma unroll
      for (int u = 0; u < kTV; ++u) {
        const int x = tid + u * kThreads, i = x / kFT, j = x % kFT;
        Bs[i * kFLD + j] = bn[u];
      }
    };
    sn_strip_a(a, panel + sn_tile_dev(ns, I, J + 1) * kFT * kFT, kFT, wave * 16);
    load_b(J + 1);
    store_b();
    __syncthreads();
    for (int K = J + 1; K <= Kmax; ++K) {
      const bool more = K + 1 <= Kmax;
      if (more) load_b(K + 1);
      mfma_strip_ra<false>(acc, a, Bs, -1.0);
      if (more) sn_strip_a(a, panel + sn_tile_dev(ns, I, K + 1) * kFT * kFT, kFT, wave * 16);
      __syncthreads();
      if (more) {
        store_b();
        __syncthreads();
      }
    }
  } else {
    for (int K = J + 1; K <= Kmax; ++K) {
      double a[kFT / 4];
      sn_strip_a(a, panel + sn_tile_dev(ns, I, K) * kFT * kFT, kFT, wave * 16);
      sn_tile_to_lds(Bs, F + static_cast<long>(K) * kFT * ld + J * kFT, ld);
      __syncthreads();
      mfma_strip_ra<false>(acc, a, Bs, -1.0);
      __syncthreads();
    }
  }
  const int l = tid & 63;
  double a[kFT / 4];
  {  // acc into the A-operand layout through the LDS tile (the wave's own 16 rows)
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int q = 0; q < 4; ++q) Bs[(wave * 16 + (l >> 4) + 4 * q) * kFLD + cb * 16 + (l & 15)] = acc[cb][q];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kFT / 4; ++i) a[i] = Bs[(wave * 16 + (l & 15)) * kFLD + 4 * i + (l >> 4)];
    __syncthreads();
  }
  const double* dj = panel + sn_tile_dev(ns, J, J) * kFT * kFT;
  for (int x = tid; x < kFT * kFT; x += kThreads) Bs[(x / kFT) * kFLD + x % kFT] = dj[x];
  __syncthreads();
  f64x4 z[4] = {};
  mfma_strip_ra<false>(z, a, Bs, 1.0);
  double* out = panel + sn_tile_dev(ns, I, J) * kFT * kFT;
  const int rbase = I < ns ? I * kFT : (I - ns) * kFT, rlim = I < ns ? sb : tb;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int rr = wave * 16 + (l >> 4) + 4 * q, cc = cb * 16 + (l & 15);
      const bool real = rbase + rr < rlim && J * kFT + cc < sb;
      out[rr * kFT + cc] = real ? z[cb][q] : 0.0;
    }
}

template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_precond_finish(LaunchCtx c, const double* __restrict__ X,
                                                             const double* __restrict__ zraw,
                                                             const double* __restrict__ in,
                                                             const int* __restrict__ ident,
                                                             const double* __restrict__ rref, int project,
                                                             double* __restrict__ z_out,
                                                             double* __restrict__ delta_out) {
  constexpr int D = B - 1;
  const PoseLane p = pose_lane<B>(c);
  if (tile_skipped(c, p.agent)) return;
  const bool own = p.ok && p.k < B;
  const long off = p.j * (R * B) + p.k * R;
  // an agent whose factorisation failed: out = in, unprojected (src/QuadraticProblem.cpp:81-86), per agent
  const bool fallback = ident != nullptr && ident[p.agent] != 0;
  if (fallback) project = 0;
  double zc[R], xc[R], rc[R];
  load_col<R, B>(fallback ? in : zraw, p.j, p.k, p.ok, zc);
  load_col<R, B>(X, p.j, p.k, p.ok, xc);
  load_col<R, B>(rref, p.j, p.k, p.ok, rc);
  double z[R];
  if (project) {
    double Yf[R][D];
    quad_gather_y<R, D>(xc, Yf);
    double S[D][D];
    sym_ytm_cols<R, D>(Yf, zc, S);
    sub_y_times_col<R, D>(Yf, S, p.k, zc, z);
  } else {
#pragma unroll
    for (int a = 0; a < R; ++a) z[a] = zc[a];
  }
  double zr = 0.0, rr = 0.0, dc[R];
#pragma unroll
  for (int a = 0; a < R; ++a) {
    zr = fma(z[a], rc[a], zr);
    rr = fma(rc[a], rc[a], rr);
    dc[a] = -z[a];
  }
  if (z_out != nullptr) store_vec<R>(z_out, off, own, z);
  if (delta_out != nullptr) store_vec<R>(delta_out, off, own, dc);
  double parts[2] = {own ? zr : 0.0, own ? rr : 0.0};
  if (c.partials != nullptr) block_partials<2>(parts, c.partials, p.tile);
}

// ------------------------------------------------------------------------------------------
// Public-pose exchange helpers (PGOAgent::getSharedPoseDict / updateNeighborPoses,
// src/PGOAgent.cpp:95-118, 434-479): dst[s] = pose idx[s] of A (idx >= 0) or of B (-1 - idx).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_gather_poses(int count, int rb, const int* __restrict__ idx,
                                                           const double* __restrict__ A,
                                                           const double* __restrict__ Bsrc,
                                                           double* __restrict__ dst) {
  const long t = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<long>(count) * rb) return;
  const int s = static_cast<int>(t / rb), e = static_cast<int>(t % rb);
  const int i = idx[s];
  dst[t] = i >= 0 ? A[static_cast<long>(i) * rb + e] : Bsrc[static_cast<long>(-1 - i) * rb + e];
}

// dst[idx[s]] = src[s] for count pose blocks of rb doubles (a per-colour halo into its receive slots)
__global__ __launch_bounds__(kThreads) void k_scatter_poses(int count, int rb, const int* __restrict__ idx,
                                                            const double* __restrict__ src, double* __restrict__ dst) {
  const long t = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<long>(count) * rb) return;
  const int s = static_cast<int>(t / rb), e = static_cast<int>(t % rb);
  dst[static_cast<long>(idx[s]) * rb + e] = src[t];
}

// G assembly (PGOAgent::constructGMatrix, src/PGOAgent.cpp:783-859).  For G slot s (a public
// pose of an agent) sum over its shared edges e:
//   outgoing (agent owns p1):  L = -X_nbr Omega T^T = -[k Y R^T + t p t^T | t p]
//   incoming (agent owns p2):  L = -X_nbr T Omega   = -[k Y R | t (Y t + p)]
// with k = w kappa, t = w tau.  One thread per (slot, row a).
template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_assemble_G(GEdges e, int nslots, const double* __restrict__ Xa,
                                                         const double* __restrict__ Xb,
                                                         double* __restrict__ gblk) {
  constexpr int D = B - 1;
  const long t = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<long>(nslots) * R) return;
  const int s = static_cast<int>(t / R), a = static_cast<int>(t % R);
  double L[B];
#pragma unroll
  for (int c = 0; c < B; ++c) L[c] = 0.0;
  for (int q = e.slot_off[s]; q < e.slot_off[s + 1]; ++q) {
    const int src = e.src[q];
    const double* P = src >= 0 ? Xa + static_cast<long>(src) * (R * B) : Xb + static_cast<long>(-1 - src) * (R * B);
    double Y[D], p;
#pragma unroll
    for (int v = 0; v < D; ++v) Y[v] = P[v * R + a];
    p = P[D * R + a];
    const double wq = e.w != nullptr ? e.w[q] : 1.0;  // null: unit weights (the central evaluation)
    const double k = wq * e.kappa[q], ta = wq * e.tau[q];
    const double* Rm = e.R + static_cast<long>(q) * D * D;  // row-major
    const double* tv = e.t + static_cast<long>(q) * D;
    if (e.outgoing[q]) {
#pragma unroll
      for (int c = 0; c < D; ++c) {
        double yr = 0.0;
#pragma unroll
        for (int v = 0; v < D; ++v) yr = fma(Y[v], Rm[c * D + v], yr);
        L[c] -= k * yr + ta * p * tv[c];
      }
      L[D] -= ta * p;
    } else {
#pragma unroll
      for (int c = 0; c < D; ++c) {
        double yr = 0.0;
#pragma unroll
        for (int v = 0; v < D; ++v) yr = fma(Y[v], Rm[v * D + c], yr);
        L[c] -= k * yr;
      }
      double yt = 0.0;
#pragma unroll
      for (int v = 0; v < D; ++v) yt = fma(Y[v], tv[v], yt);
      L[D] -= ta * (yt + p);
    }
  }
#pragma unroll
  for (int c = 0; c < B; ++c) gblk[static_cast<long>(s) * (R * B) + c * R + a] = L[c];
}

#endif  // !DPGO_SPMM_TU

// ------------------------------------------------------------------------------------------
// Host-side launchers with (r, b) dispatch
// ------------------------------------------------------------------------------------------
#ifdef DPGO_ISA_54_ONLY  // tools/isa_dump.sh: the headline shape only, for fast ISA inspection (never built into the library)
#define DPGO_DISPATCH(R_, B_, CALL)                        \
  switch ((R_) * 8 + (B_)) {                               \
    case 5 * 8 + 4: { constexpr int R = 5, B = 4; CALL; break; } \
    default: return hipErrorInvalidValue;                  \
  }
#else
#define DPGO_DISPATCH(R_, B_, CALL)                        \
  switch ((R_) * 8 + (B_)) {                               \
    case 2 * 8 + 3: { constexpr int R = 2, B = 3; CALL; break; } \
    case 3 * 8 + 3: { constexpr int R = 3, B = 3; CALL; break; } \
    case 4 * 8 + 3: { constexpr int R = 4, B = 3; CALL; break; } \
    case 5 * 8 + 3: { constexpr int R = 5, B = 3; CALL; break; } \
    case 6 * 8 + 3: { constexpr int R = 6, B = 3; CALL; break; } \
    case 7 * 8 + 3: { constexpr int R = 7, B = 3; CALL; break; } \
    case 8 * 8 + 3: { constexpr int R = 8, B = 3; CALL; break; } \
    case 3 * 8 + 4: { constexpr int R = 3, B = 4; CALL; break; } \
    case 4 * 8 + 4: { constexpr int R = 4, B = 4; CALL; break; } \
    case 5 * 8 + 4: { constexpr int R = 5, B = 4; CALL; break; } \
    case 6 * 8 + 4: { constexpr int R = 6, B = 4; CALL; break; } \
    case 7 * 8 + 4: { constexpr int R = 7, B = 4; CALL; break; } \
    case 8 * 8 + 4: { constexpr int R = 8, B = 4; CALL; break; } \
    default: return hipErrorInvalidValue;                  \
  }
#endif

// one SpMM mode over every (r, b) and Q format (instantiated in the DPGO_SPMM_TU translation units)
template <int MODE>
hipError_t spmm_mode(int r, int b, dim3 grid, const LaunchCtx& c, const QView& q, const SpmmArgs& a);

#ifndef DPGO_SPMM_TU
int g_tuning[TUNE_COUNT] = {0, -1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 6, 1, 2, 1, 1, 2000, 2};

bool supported_rb(int r, int b) {
  if (b == 3) return r >= 2 && r <= 8;
  if (b == 4) return r >= 3 && r <= 8;
  return false;
}
#else
namespace {

template <int MODE, int VAR, int FMT>
hipError_t spmm_rb(int r, int b, dim3 grid, const LaunchCtx& c, const QView& q, const SpmmArgs& a) {
  DPGO_DISPATCH(r, b, (k_spmm<R, B, MODE, VAR, FMT><<<grid, kThreads, 0, c.stream>>>(c, q, a)));
  return hipSuccess;
}

// r = 5, d = 3 (the headline shape), X.Q only: every compiled neighbour-loop variant, for A/B timing
template <int FMT>
hipError_t spmm_variant54(int var, dim3 grid, const LaunchCtx& c, const QView& q, const SpmmArgs& a) {
#define DPGO_VAR(V) \
  case V: k_spmm<5, 4, MODE_XQ, V, FMT><<<grid, kThreads, 0, c.stream>>>(c, q, a); break;
  switch (var) {
    DPGO_VAR(0) DPGO_VAR(1) DPGO_VAR(2) DPGO_VAR(3) DPGO_VAR(4) DPGO_VAR(5) DPGO_VAR(6) DPGO_VAR(7)
    default: return hipErrorInvalidValue;
  }
#undef DPGO_VAR
  return hipSuccess;
}

}  // namespace

// occupancy hint of the unified-loop HESS_M kernel (evar_waves bits: 0 none, 2 / 4 / 6 = 4 / 5 / 6 waves per SIMD)
#ifndef DPGO_UNI_WAVES
#define DPGO_UNI_WAVES 0
#endif
constexpr int kUniWaves = DPGO_UNI_WAVES & 6;
// occupancy hint of the X.Q kernel (A/B builds: -DDPGO_XQ_WAVES=6 asks for 6 waves per SIMD)
#ifndef DPGO_XQ_WAVES
#define DPGO_XQ_WAVES 0
#endif
constexpr int kXqWaves = DPGO_XQ_WAVES & 6;
template <int MODE>
constexpr int mode_waves() { return MODE == MODE_HESS_M ? kUniWaves : MODE == MODE_XQ ? kXqWaves : 0; }

template <int MODE>
hipError_t spmm_mode(int r, int b, dim3 grid, const LaunchCtx& c, const QView& q, const SpmmArgs& a) {
  if (q.fmt == QFMT_EDGES) {
    constexpr bool kPreMode = mode_hess(MODE) || MODE == MODE_QF || MODE == MODE_EVAL_TCG;
    const int v2 = q.tuning[TUNE_SPMM_V2];
    if (v2 > 0) {
      // round-4 kernels: the merged modes' partials (bit 6) for every shape, since the host's dd_mask follows the
      // tuning key; the rotated accumulator (bit 7, bitwise the plain one) at the headline shape: v2 = 1 every
      // mode, 2 none, 3 the merged modes only
      constexpr int V2 = kEdgeDefaultVariant | (mode_merged(MODE) ? 64 : 0);
      // 6 (default): rotated + one pipeline in every mode that stages its records (X.Q, EVAL_TCG, HESS*; the half
      // passes F / QF keep the plain accumulator: rotated measured +3.6 us on F, profiles/r05c_ab_v2.log)
      constexpr bool kHalfMode = MODE == MODE_F || MODE == MODE_QF;
      const bool rot = v2 == 1 || v2 == 5 || (v2 == 6 && !kHalfMode) || ((v2 == 3 || v2 == 4) && mode_merged(MODE));
      const bool uni = v2 == 5 || (v2 == 6 && !kHalfMode) || (v2 == 4 && mode_merged(MODE));
      if (uni && r == 5 && b == 4) {
        if constexpr (kPreMode) {
          if (q.tuning[TUNE_EPI_PREFETCH] > 0) {
            k_spmm<5, 4, MODE, V2 | mode_waves<MODE>() | 8 | 128 | 256, QFMT_EDGES><<<grid, kThreads, 0, c.stream>>>(c, q, a);
            return hipSuccess;
          }
        }
        k_spmm<5, 4, MODE, V2 | mode_waves<MODE>() | 128 | 256, QFMT_EDGES><<<grid, kThreads, 0, c.stream>>>(c, q, a);
        return hipSuccess;
      }
      if (r == 5 && b == 4 && (q.tuning[TUNE_EDGE_VARIANT] < 0 || mode_merged(MODE))) {
        if constexpr (kPreMode) {
          if (q.tuning[TUNE_EPI_PREFETCH] > 0) {
            if (rot)
              k_spmm<5, 4, MODE, V2 | 8 | 128, QFMT_EDGES><<<grid, kThreads, 0, c.stream>>>(c, q, a);
            else
              k_spmm<5, 4, MODE, V2 | 8, QFMT_EDGES><<<grid, kThreads, 0, c.stream>>>(c, q, a);
            return hipSuccess;
          }
        }
        if (rot)
          k_spmm<5, 4, MODE, V2 | 128, QFMT_EDGES><<<grid, kThreads, 0, c.stream>>>(c, q, a);
        else
          k_spmm<5, 4, MODE, V2, QFMT_EDGES><<<grid, kThreads, 0, c.stream>>>(c, q, a);
        return hipSuccess;
      }
      if constexpr (mode_merged(MODE)) return spmm_rb<MODE, V2, QFMT_EDGES>(r, b, grid, c, q, a);
    }
    if constexpr (mode_hess(MODE)) {
      if (r == 5 && b == 4 && q.tuning[TUNE_SV_STAGE] > 0 && q.tuning[TUNE_EDGE_VARIANT] < 0 && q.sv_ptr != nullptr) {
        k_spmm<5, 4, MODE, kEdgeDefaultVariant | 8 | 32, QFMT_EDGES><<<grid, kThreads, 0, c.stream>>>(c, q, a);
        return hipSuccess;
      }
    }
    if constexpr (mode_merged(MODE)) {
      const int mp = q.tuning[TUNE_MERGED_PREFETCH];
      if (r == 5 && b == 4 && q.tuning[TUNE_EPI_PREFETCH] > 0 && q.tuning[TUNE_EDGE_VARIANT] < 0 && mp > 0) {
        // (measured slower: occupancy 4 -> 3; the 5-wave register budgets measured spill)
        k_spmm<5, 4, MODE, kEdgeDefaultVariant | 8 | 16, QFMT_EDGES><<<grid, kThreads, 0, c.stream>>>(c, q, a);
        return hipSuccess;
      }
    }
    if constexpr (kPreMode) {
      if (r == 5 && b == 4 && q.tuning[TUNE_EPI_PREFETCH] > 0 && q.tuning[TUNE_EDGE_VARIANT] < 0) {
        k_spmm<5, 4, MODE, kEdgeDefaultVariant | 8, QFMT_EDGES><<<grid, kThreads, 0, c.stream>>>(c, q, a);
        return hipSuccess;
      }
    }
    const int var = q.tuning[TUNE_EDGE_VARIANT] < 0 ? kEdgeDefaultVariant : q.tuning[TUNE_EDGE_VARIANT];
    if constexpr (MODE == MODE_XQ) {
      if (r == 5 && b == 4 && var != kEdgeDefaultVariant) return spmm_variant54<QFMT_EDGES>(var, grid, c, q, a);
    }
    return spmm_rb<MODE, kEdgeDefaultVariant, QFMT_EDGES>(r, b, grid, c, q, a);
  }
  const int var = q.tuning[TUNE_SPMM_VARIANT];
  if constexpr (MODE == MODE_XQ) {
    if (r == 5 && b == 4 && var != 0) return spmm_variant54<QFMT_BSR>(var, grid, c, q, a);
  }
  return spmm_rb<MODE, 0, QFMT_BSR>(r, b, grid, c, q, a);
}

#define DPGO_SPMM_INST(M) template hipError_t spmm_mode<M>(int, int, dim3, const LaunchCtx&, const QView&, const SpmmArgs&);
#if DPGO_SPMM_TU == 1
DPGO_SPMM_INST(MODE_XQ)
DPGO_SPMM_INST(MODE_XQ_G)
#elif DPGO_SPMM_TU == 2
DPGO_SPMM_INST(MODE_EVAL)
DPGO_SPMM_INST(MODE_F)
DPGO_SPMM_INST(MODE_CERT)
#elif DPGO_SPMM_TU == 3
DPGO_SPMM_INST(MODE_HESS)
DPGO_SPMM_INST(MODE_QF)
#elif DPGO_SPMM_TU == 4
DPGO_SPMM_INST(MODE_HESS_QF)
DPGO_SPMM_INST(MODE_EVAL_TCG)
#elif DPGO_SPMM_TU == 5
DPGO_SPMM_INST(MODE_HESS_M)
DPGO_SPMM_INST(MODE_HESS_QF_M)
#else
#error "DPGO_SPMM_TU must be 1..5"
#endif
#undef DPGO_SPMM_INST
#endif  // DPGO_SPMM_TU

#ifndef DPGO_SPMM_TU

hipError_t launch_spmm(int r, int b, int mode, const LaunchCtx& c, const QView& q, const SpmmArgs& a) {
  if (c.num_tiles == 0) return hipSuccess;
  const dim3 grid(c.num_tiles);
  hipError_t e = hipErrorInvalidValue;
  switch (mode) {
    case MODE_XQ: e = spmm_mode<MODE_XQ>(r, b, grid, c, q, a); break;
    case MODE_XQ_G: e = spmm_mode<MODE_XQ_G>(r, b, grid, c, q, a); break;
    case MODE_EVAL: e = spmm_mode<MODE_EVAL>(r, b, grid, c, q, a); break;
    case MODE_HESS: e = spmm_mode<MODE_HESS>(r, b, grid, c, q, a); break;
    case MODE_F: e = spmm_mode<MODE_F>(r, b, grid, c, q, a); break;
    case MODE_EVAL_TCG: e = spmm_mode<MODE_EVAL_TCG>(r, b, grid, c, q, a); break;
    case MODE_CERT: e = spmm_mode<MODE_CERT>(r, b, grid, c, q, a); break;
    case MODE_QF: e = spmm_mode<MODE_QF>(r, b, grid, c, q, a); break;
    case MODE_HESS_QF: e = spmm_mode<MODE_HESS_QF>(r, b, grid, c, q, a); break;
    case MODE_HESS_M: e = spmm_mode<MODE_HESS_M>(r, b, grid, c, q, a); break;
    case MODE_HESS_QF_M: e = spmm_mode<MODE_HESS_QF_M>(r, b, grid, c, q, a); break;
    default: break;
  }
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t launch_tcg_init(int r, int b, const LaunchCtx& c, const double* X, const double* Minv, int pmode,
                           const double* g, double* delta) {
  if (c.num_tiles == 0) return hipSuccess;
  DPGO_DISPATCH(r, b, (k_tcg_init<R, B><<<c.num_tiles, kThreads, 0, c.stream>>>(c, X, Minv, pmode, g, delta)));
  return hipGetLastError();
}

hipError_t launch_tcg_update(int r, int b, const LaunchCtx& c, const double* X, const double* Minv, int pmode,
                             const double* delta, const double* Hdelta, double* eta,
                             const double* r_in, double* rv, double* z, int first, const FinalizeArgs* fin,
                             int* arrive) {
  if (c.num_tiles == 0) return hipSuccess;
  if (fin != nullptr) {
    DPGO_DISPATCH(r, b, (k_tcg_update<R, B, true><<<c.num_tiles, kThreads, 0, c.stream>>>(c, X, Minv, pmode, delta, Hdelta, eta, r_in, rv, z, first, *fin, arrive)));
  } else {
    DPGO_DISPATCH(r, b, (k_tcg_update<R, B, false><<<c.num_tiles, kThreads, 0, c.stream>>>(c, X, Minv, pmode, delta, Hdelta, eta, r_in, rv, z, first, FinalizeArgs{}, nullptr)));
  }
  return hipGetLastError();
}

hipError_t launch_tcg_dir(int r, int b, const LaunchCtx& c, const double* z, double* delta, const FinalizeArgs* fin,
                          int* arrive) {
  if (c.num_tiles == 0) return hipSuccess;
  if (fin != nullptr) {
    DPGO_DISPATCH(r, b, (k_tcg_dir<R, B, true><<<c.num_tiles, kThreads, 0, c.stream>>>(c, z, delta, *fin, arrive)));
  } else {
    DPGO_DISPATCH(r, b, (k_tcg_dir<R, B, false><<<c.num_tiles, kThreads, 0, c.stream>>>(c, z, delta, FinalizeArgs{}, nullptr)));
  }
  return hipGetLastError();
}

hipError_t launch_tcg_updir(int r, int b, const LaunchCtx& c, const double* X, const double* Minv, int pmode,
                            double* delta, const double* Hdelta, double* eta, const double* r_in, double* rv,
                            int first, int last) {
  if (c.num_tiles == 0) return hipSuccess;
  DPGO_DISPATCH(r, b, (k_tcg_updir<R, B><<<c.num_tiles, kThreads, 0, c.stream>>>(c, X, Minv, pmode, delta, Hdelta, eta,
                                                                                  r_in, rv, first, last)));
  return hipGetLastError();
}

hipError_t launch_retract(int r, int b, const LaunchCtx& c, const double* X, const double* V, double scale,
                          double* out, const double* g, const double* HV, const double* delta_impl,
                          const double* status_ref, const RetractTail* tail) {
  if (c.num_tiles == 0) return hipSuccess;
  if (tail != nullptr) {
    if (c.state == nullptr || tail->delta == nullptr || tail->Hdelta == nullptr || tail->peh == nullptr)
      return hipErrorInvalidValue;
    DPGO_DISPATCH(r, b, (k_retract<R, B, true><<<c.num_tiles, kThreads, 0, c.stream>>>(c, X, V, scale, out, g, HV,
                                                                                       delta_impl, status_ref, *tail)));
  } else {
    DPGO_DISPATCH(r, b, (k_retract<R, B, false><<<c.num_tiles, kThreads, 0, c.stream>>>(
                            c, X, V, scale, out, g, HV, delta_impl, status_ref, RetractTail{})));
  }
  return hipGetLastError();
}

hipError_t launch_tangent(int r, int b, const LaunchCtx& c, const double* X, const double* V, double* out) {
  if (c.num_tiles == 0) return hipSuccess;
  DPGO_DISPATCH(r, b, (k_tangent<R, B><<<c.num_tiles, kThreads, 0, c.stream>>>(c, X, V, out)));
  return hipGetLastError();
}

hipError_t launch_precond(int r, int b, const LaunchCtx& c, const double* X, const double* Minv, int pmode,
                          const double* V, double* out) {
  if (c.num_tiles == 0) return hipSuccess;
  DPGO_DISPATCH(r, b, (k_precond<R, B><<<c.num_tiles, kThreads, 0, c.stream>>>(c, X, Minv, pmode, V, out)));
  return hipGetLastError();
}

hipError_t launch_polar_comb(int r, int b, const LaunchCtx& c, const double* A, const double* Bv,
                             const double* ca, const double* cb, double* out, const double* Cv, double sa,
                             double sb, double* out2, double* xcopy, const PolarNext* next) {
  if (c.num_tiles == 0) return hipSuccess;
  if (next != nullptr) {  // the a0 A + b0 B form with uniform coefficients only
    if (Bv == nullptr || Cv != nullptr || ca != nullptr || cb != nullptr || next->y == nullptr)
      return hipErrorInvalidValue;
    DPGO_DISPATCH(r, b, (k_polar_comb<R, B, true><<<c.num_tiles, 64, 0, c.stream>>>(
                            c, A, Bv, ca, cb, out, Cv, sa, sb, out2, xcopy, next->sa, next->sb, next->y, next->xprev)));
  } else {
    DPGO_DISPATCH(r, b, (k_polar_comb<R, B, false><<<c.num_tiles, 64, 0, c.stream>>>(
                            c, A, Bv, ca, cb, out, Cv, sa, sb, out2, xcopy, 0.0, 0.0, nullptr, nullptr)));
  }
  return hipGetLastError();
}

hipError_t launch_polar_vnext(int r, int b, const LaunchCtx& c, const double* X, double* V, const double* Yv,
                              double gv, double sa, double sb, double* out, double* xcopy, const PolarNext* next) {
  if (c.num_tiles == 0) return hipSuccess;
  if (next != nullptr) {
    if (next->y == nullptr) return hipErrorInvalidValue;
    DPGO_DISPATCH(r, b, (k_polar_vnext<R, B, true><<<c.num_tiles, 64, 0, c.stream>>>(
                            c, X, V, Yv, gv, sa, sb, out, xcopy, next->sa, next->sb, next->y, next->xprev)));
  } else {
    DPGO_DISPATCH(r, b, (k_polar_vnext<R, B, false><<<c.num_tiles, 64, 0, c.stream>>>(
                            c, X, V, Yv, gv, sa, sb, out, xcopy, 0.0, 0.0, nullptr, nullptr)));
  }
  return hipGetLastError();
}

hipError_t launch_round_se(int r, int b, long n, const double* X, const double* anchor, double* T,
                           hipStream_t stream) {
  if (n <= 0 || X == nullptr || T == nullptr) return hipErrorInvalidValue;
  const long blocks = (n + 63) / 64;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(blocks));
  const double* A = anchor != nullptr ? anchor : X;  // the local frame: pose 0 of X
  DPGO_DISPATCH(r, b, (k_round_se<R, B><<<grid, 64, 0, stream>>>(n, X, A, T)));
  return hipGetLastError();
}

hipError_t launch_lift_escape(int r, int b, long n, const double* X, const double* v, double alpha, double* out,
                              hipStream_t stream) {
  if (n <= 0 || X == nullptr || out == nullptr || !supported_rb(r + 1, b)) return hipErrorInvalidValue;
  const long blocks = (n + 63) / 64;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(blocks));
  DPGO_DISPATCH(r, b, (k_lift_escape<R, B><<<grid, 64, 0, stream>>>(n, X, v, alpha, out)));
  return hipGetLastError();
}

hipError_t launch_frame_lift(int r, int b, long n, const double* T, const FrameLiftY& ylift, const double* frames,
                             const int* frame_of, double* out, hipStream_t stream) {
  if (n <= 0 || T == nullptr || out == nullptr || (frames == nullptr) != (frame_of == nullptr))
    return hipErrorInvalidValue;
  const long blocks = (n + 63) / 64;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(blocks));
  DPGO_DISPATCH(r, b, (k_frame_lift<R, B><<<grid, 64, 0, stream>>>(n, T, ylift, frames, frame_of, out)));
  return hipGetLastError();
}

hipError_t launch_gram(int r, int b, long n, const double* X, double* C, double* work, hipStream_t stream) {
  if (n <= 0 || X == nullptr || C == nullptr || work == nullptr) return hipErrorInvalidValue;
  const long blocks = gram_blocks(n);
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(blocks));
  DPGO_DISPATCH(r, b, (k_gram<R, B><<<grid, 64, 0, stream>>>(n, X, work)));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  k_gram_finish<<<r * (r + 1) / 2, kGramFinishThreads, 0, stream>>>(blocks, r, work, C);
  return hipGetLastError();
}

namespace {
// the input ranks K < R <= 8 of one compiled output shape (K, B)
template <int R, int K, int B>
hipError_t rank_project_rkb(dim3 grid, long n, const double* X, const RankW& W, double* out, hipStream_t stream) {
  if constexpr (R > K) {
    k_rank_project<R, K, B><<<grid, 64, 0, stream>>>(n, X, W, out);
    return hipSuccess;
  } else {
    return hipErrorInvalidValue;
  }
}
template <int K, int B>
hipError_t rank_project_kb(int r, dim3 grid, long n, const double* X, const RankW& W, double* out,
                           hipStream_t stream) {
  switch (r) {
    case 3: return rank_project_rkb<3, K, B>(grid, n, X, W, out, stream);
    case 4: return rank_project_rkb<4, K, B>(grid, n, X, W, out, stream);
    case 5: return rank_project_rkb<5, K, B>(grid, n, X, W, out, stream);
    case 6: return rank_project_rkb<6, K, B>(grid, n, X, W, out, stream);
    case 7: return rank_project_rkb<7, K, B>(grid, n, X, W, out, stream);
    case 8: return rank_project_rkb<8, K, B>(grid, n, X, W, out, stream);
    default: return hipErrorInvalidValue;
  }
}
}  // namespace

hipError_t launch_rank_project(int r, int k, int b, long n, const double* X, const RankW& W, double* out,
                               hipStream_t stream) {
  if (n <= 0 || X == nullptr || out == nullptr || k < b - 1 || k >= r || !supported_rb(r, b))
    return hipErrorInvalidValue;
  const long blocks = (n + 63) / 64;
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(blocks));
  // R is the output rank here: the dispatch runs over the 13 compiled (k, b)
  hipError_t e = hipSuccess;
  DPGO_DISPATCH(k, b, (e = rank_project_kb<R, B>(r, grid, n, X, W, out, stream)));
  return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_edge_errors(int r, int b, const EdgeList& E, const double* X, const double* X2, double* err,
                              double* rot_sq, double* tra_sq, double* cost, double* work, hipStream_t stream) {
  if (E.m <= 0 || !E.p1 || !E.p2 || !E.R || !E.t || !E.kappa || !E.tau || X == nullptr) return hipErrorInvalidValue;
  if (!err && !rot_sq && !tra_sq && !cost) return hipErrorInvalidValue;
  if (cost != nullptr && work == nullptr) return hipErrorInvalidValue;
  const long blocks = edge_errors_blocks(E.m);
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(blocks));
  double* partial = cost ? work : nullptr;
  DPGO_DISPATCH(r, b, (k_edge_errors<R, B - 1><<<grid, kEdgeErrThreads, 0, stream>>>(
                          E.m, E.p1, E.p2, E.R, E.t, E.kappa, E.tau, E.w, X, X2, err, rot_sq, tra_sq, partial)));
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || !cost) return e;
  k_edge_cost_finish<<<1, kEdgeFinishThreads, 0, stream>>>(blocks, work, cost);
  return hipGetLastError();
}

hipError_t launch_traj_moments(int d, long n, const double* That, const double* T, const int* use,
                               const double* shift, double* mom, double* work, hipStream_t stream) {
  if ((d != 2 && d != 3) || n <= 0 || !That || !T || !mom || !work) return hipErrorInvalidValue;
  const long blocks = traj_blocks(n);
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(blocks));
  TrajShift S{};
  if (shift != nullptr)
    for (int i = 0; i < d; ++i) {
      S.sh[i] = shift[i];
      S.st[i] = shift[d + i];
    }
  if (d == 2)
    k_traj_moments<2><<<grid, 64, 0, stream>>>(n, That, T, use, S, work);
  else
    k_traj_moments<3><<<grid, 64, 0, stream>>>(n, That, T, use, S, work);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int P = traj_moments_len(d);
  k_traj_finish<<<P, kTrajFinishThreads, 0, stream>>>(blocks, P, work, mom);
  return hipGetLastError();
}

hipError_t launch_traj_errors(int d, long n, const double* That, const double* T, const int* use, const double* Aa,
                              double* tra_sq, double* rot_sq, double* sums, double* work, hipStream_t stream) {
  if ((d != 2 && d != 3) || n <= 0 || !That || !T) return hipErrorInvalidValue;
  if (!tra_sq && !rot_sq && !sums) return hipErrorInvalidValue;
  if (sums != nullptr && work == nullptr) return hipErrorInvalidValue;
  const long blocks = traj_blocks(n);
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(blocks));
  TrajAa A{};
  for (int c = 0; c <= d; ++c)
    for (int i = 0; i < d; ++i) A.v[c * d + i] = Aa != nullptr ? Aa[c * d + i] : (i == c ? 1.0 : 0.0);
  double* partial = sums ? work : nullptr;
  if (d == 2)
    k_traj_errors<2><<<grid, 64, 0, stream>>>(n, That, T, use, A, tra_sq, rot_sq, partial);
  else
    k_traj_errors<3><<<grid, 64, 0, stream>>>(n, That, T, use, A, tra_sq, rot_sq, partial);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || !sums) return e;
  k_traj_finish<<<kTrajSums, kTrajFinishThreads, 0, stream>>>(blocks, 3, work, sums);
  return hipGetLastError();
}

hipError_t launch_relative_poses(int d, long m, const int* p1, const int* p2, const double* T, double* R_out,
                                 double* t_out, hipStream_t stream) {
  if ((d != 2 && d != 3) || m <= 0 || !p1 || !p2 || !T || !R_out || !t_out) return hipErrorInvalidValue;
  const long blocks = edge_errors_blocks(m);
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(blocks));
  if (d == 2)
    k_relative_poses<2><<<grid, kEdgeErrThreads, 0, stream>>>(m, p1, p2, T, R_out, t_out);
  else
    k_relative_poses<3><<<grid, kEdgeErrThreads, 0, stream>>>(m, p1, p2, T, R_out, t_out);
  return hipGetLastError();
}

hipError_t launch_pair_consistency(int d, long ntiles, const PcmTile* tiles, const double* F, const double* x,
                                   const int* group_off, const long long* word_off, const long long* dense_off,
                                   double cR2, double ct2, unsigned long long* adj, int* degree, int m,
                                   double* e_rot, double* e_tra, hipStream_t stream) {
  if ((d != 2 && d != 3) || ntiles < 0 || m < 0) return hipErrorInvalidValue;
  if (m == 0) return hipSuccess;
  if (!F || !x || !group_off || !word_off || !dense_off || !degree) return hipErrorInvalidValue;
  const hipError_t z = hipMemsetAsync(degree, 0, sizeof(int) * static_cast<size_t>(m), stream);
  if (z != hipSuccess || ntiles == 0) return z;
  if (!tiles || !adj || ntiles > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(ntiles));
  if (d == 2)
    k_pair_consistency<2><<<grid, 64, 0, stream>>>(tiles, F, x, group_off, word_off, dense_off, cR2, ct2, adj,
                                                   degree, e_rot, e_tra);
  else
    k_pair_consistency<3><<<grid, 64, 0, stream>>>(tiles, F, x, group_off, word_off, dense_off, cR2, ct2, adj,
                                                   degree, e_rot, e_tra);
  return hipGetLastError();
}

hipError_t launch_sqdiff(int r, int b, const LaunchCtx& c, const double* A, const double* Bv) {
  if (c.num_tiles == 0) return hipSuccess;
  DPGO_DISPATCH(r, b, (k_sqdiff<R, B><<<c.num_tiles, kThreads, 0, c.stream>>>(c, A, Bv)));
  return hipGetLastError();
}

hipError_t launch_select(int r, int b, const LaunchCtx& c, const double* A, const double* Bv, const int* use_a,
                         const double* ref, double* out) {
  if (c.num_tiles == 0) return hipSuccess;
  DPGO_DISPATCH(r, b, (k_select<R, B><<<c.num_tiles, kThreads, 0, c.stream>>>(c, A, Bv, use_a, ref, out)));
  return hipGetLastError();
}

hipError_t launch_accept(int r, int b, const LaunchCtx& c, const double* x2, const double* g2, const double* S2,
                         double* x1, double* g, double* S) {
  if (c.num_tiles == 0) return hipSuccess;
  DPGO_DISPATCH(r, b, (k_accept<R, B><<<c.num_tiles, kThreads, 0, c.stream>>>(c, x2, g2, S2, x1, g, S)));
  return hipGetLastError();
}

hipError_t launch_gather_poses(int count, int rb, const int* idx, const double* A, const double* Bsrc, double* dst,
                               hipStream_t stream) {
  if (count == 0) return hipSuccess;
  const long total = static_cast<long>(count) * rb;
  k_gather_poses<<<static_cast<int>((total + kThreads - 1) / kThreads), kThreads, 0, stream>>>(count, rb, idx, A, Bsrc, dst);
  return hipGetLastError();
}

hipError_t launch_scatter_poses(int count, int rb, const int* idx, const double* src, double* dst, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  const long total = static_cast<long>(count) * rb;
  k_scatter_poses<<<static_cast<int>((total + kThreads - 1) / kThreads), kThreads, 0, stream>>>(count, rb, idx, src, dst);
  return hipGetLastError();
}

hipError_t launch_assemble_G(int r, int b, const GEdges& e, int nslots, const double* Xa, const double* Xb,
                             double* gblk, hipStream_t stream) {
  if (nslots == 0) return hipSuccess;
  const long total = static_cast<long>(nslots) * r;
  const int grid = static_cast<int>((total + kThreads - 1) / kThreads);
  DPGO_DISPATCH(r, b, (k_assemble_G<R, B><<<grid, kThreads, 0, stream>>>(e, nslots, Xa, Xb, gblk)));
  return hipGetLastError();
}

#define DPGO_DISPATCH_R(R_, CALL)                          \
  switch (R_) {                                            \
    case 2: { constexpr int R = 2; CALL; break; }          \
    case 3: { constexpr int R = 3; CALL; break; }          \
    case 4: { constexpr int R = 4; CALL; break; }          \
    case 5: { constexpr int R = 5; CALL; break; }          \
    case 6: { constexpr int R = 6; CALL; break; }          \
    case 7: { constexpr int R = 7; CALL; break; }          \
    case 8: { constexpr int R = 8; CALL; break; }          \
    default: return hipErrorInvalidValue;                  \
  }

hipError_t launch_sn_assemble(int r, int b, const SnView& v, const int2* items, int count, const double* rhs,
                              hipStream_t stream) {
  if (count == 0) return hipSuccess;
  DPGO_DISPATCH_R(r, (k_sn_assemble<R><<<count, kThreads, 0, stream>>>(v, items, b, rhs)));
  return hipGetLastError();
}

hipError_t launch_sn_fwd(int r, int b, const SnView& v, const int2* items, int count, double* y, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  DPGO_DISPATCH_R(r, (k_sn_fwd<R><<<count, kThreads, 0, stream>>>(v, items, b, y)));
  return hipGetLastError();
}
hipError_t launch_sn_fwd_small(int r, int b, const SnView& v, const int2* items, int count, double* y,
                               hipStream_t stream) {
  if (count == 0) return hipSuccess;
  DPGO_DISPATCH_R(r, (k_sn_fwd_small<R><<<count, kThreads, 0, stream>>>(v, items, b, y)));
  return hipGetLastError();
}

hipError_t launch_sn_bwd(int r, int b, const SnView& v, const int2* items, int count, const double* y, double* x,
                         hipStream_t stream) {
  if (count == 0) return hipSuccess;
  DPGO_DISPATCH_R(r, (k_sn_bwd<R><<<count, kThreads, 0, stream>>>(v, items, b, y, x)));
  return hipGetLastError();
}

hipError_t launch_sn_compact(int b, const double* panel, const long* panel_off, const int* s, const int* t,
                             const long* cpanel_off, double* cpanel, const int2* items, int count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  k_sn_compact<<<count, kThreads, 0, stream>>>(b, panel, panel_off, s, t, cpanel_off, cpanel, items);
  return hipGetLastError();
}

hipError_t launch_sn_factor(int b, const SnFactorView& v, int count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  if (b == 4)
    k_sn_factor<4><<<count, kThreads, 0, stream>>>(v);
  else if (b == 3)
    k_sn_factor<3><<<count, kThreads, 0, stream>>>(v);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_sn_factor_tiled(int b, const SnFactorView& v, int kind, int param, const int2* items, int count,
                                  hipStream_t stream) {
  if (count == 0) return hipSuccess;
  if (kind == 0) {
    if (b == 4)
      k_snf_asm<4><<<count, kThreads, 0, stream>>>(v, items, param);
    else if (b == 3)
      k_snf_asm<3><<<count, kThreads, 0, stream>>>(v, items, param);
    else
      return hipErrorInvalidValue;
  } else {
    if (b != 3 && b != 4) return hipErrorInvalidValue;
#define DPGO_SNF(K)                                                             \
  case K:                                                                       \
    if (b == 4)                                                                 \
      k_snf_tile<4, K><<<count, kThreads, 0, stream>>>(v, items, param);        \
    else                                                                        \
      k_snf_tile<3, K><<<count, kThreads, 0, stream>>>(v, items, param);        \
    break;
    switch (kind) {
      DPGO_SNF(1) DPGO_SNF(2) DPGO_SNF(3) DPGO_SNF(4) DPGO_SNF(5)
      default: return hipErrorInvalidValue;
    }
#undef DPGO_SNF
  }
  return hipGetLastError();
}

hipError_t launch_precond_finish(int r, int b, const LaunchCtx& c, const double* X, const double* zraw,
                                 const double* in, const int* ident, const double* rref, int project, double* z_out,
                                 double* delta_out) {
  if (c.num_tiles == 0) return hipSuccess;
  DPGO_DISPATCH(r, b, (k_precond_finish<R, B><<<c.num_tiles, kThreads, 0, c.stream>>>(c, X, zraw, in, ident, rref,
                                                                                      project, z_out, delta_out)));
  return hipGetLastError();
}

#ifdef DPGO_FIN_PROBE
}  // namespace dpgo
extern "C" int dpgo_hip_debug_fin_probe(long long* out, int* n) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(dpgo::g_fin_probe), sizeof(long long) * 256 * 6) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(n, HIP_SYMBOL(dpgo::g_fin_probe_n), sizeof(int)) != hipSuccess) return -1;
  return 0;
}
namespace dpgo {
#endif

hipError_t launch_finalize(const FinalizeArgs& f, int num_agents, hipStream_t stream) {
  if (num_agents == 0) return hipSuccess;
  // four slots cover every op but the merged tCG's (seven HESS_M partials) and those carrying pc
  const bool wide = f.nq_c > 0 || f.nq_a + f.nq_b > 4;
  if (wide && f.op == OP_TCG_STEP_CHECK)  // every merged tCG iteration
    k_finalize<kMaxTot, OP_TCG_STEP_CHECK><<<num_agents, kThreads, 0, stream>>>(f);
  else if (wide && f.op == OP_RHO)
    k_finalize<kMaxTot, OP_RHO><<<num_agents, kThreads, 0, stream>>>(f);
  else if (wide)
    k_finalize<kMaxTot><<<num_agents, kThreads, 0, stream>>>(f);
  else if (f.op == OP_EVAL_TCG_INIT)
    k_finalize<4, OP_EVAL_TCG_INIT><<<num_agents, kThreads, 0, stream>>>(f);
  else if (f.op == OP_RHO)
    k_finalize<4, OP_RHO><<<num_agents, kThreads, 0, stream>>>(f);
  else
    k_finalize<4><<<num_agents, kThreads, 0, stream>>>(f);
  return hipGetLastError();
}

hipError_t launch_edge_reweight(int d, int m, int n, const double* raw, const int* slot_of_edge, const double* w,
                                const int* dinc_ptr, const int* dinc, double* wslot, double* rec, double* diag,
                                hipStream_t stream) {
  if (m == 0 && n == 0) return hipSuccess;
  const int ge = (m + kThreads - 1) / kThreads, gn = (n + kThreads - 1) / kThreads;
  if (m > 0) {
    k_weights_to_slots<<<ge, kThreads, 0, stream>>>(m, slot_of_edge, w, wslot);
    if (d == 3)
      k_edge_records<3><<<ge, kThreads, 0, stream>>>(m, raw, slot_of_edge, w, rec);
    else
      k_edge_records<2><<<ge, kThreads, 0, stream>>>(m, raw, slot_of_edge, w, rec);
  }
  if (n > 0) {
    if (d == 3)
      k_edge_diag<3><<<gn, kThreads, 0, stream>>>(n, raw, nullptr, wslot, dinc_ptr, dinc, diag);
    else
      k_edge_diag<2><<<gn, kThreads, 0, stream>>>(n, raw, nullptr, wslot, dinc_ptr, dinc, diag);
  }
  return hipGetLastError();
}

hipError_t launch_gnc_snapshot(int r, int b, const GncEntries& g, const double* X, const double* RX, const int* mask,
                               hipStream_t stream) {
  if (g.n == 0) return hipSuccess;
  const long total = static_cast<long>(g.n) * r * b;
  const int grid = static_cast<int>((total + kThreads - 1) / kThreads);
  DPGO_DISPATCH(r, b, (k_gnc_snapshot<R, B><<<grid, kThreads, 0, stream>>>(g, X, RX, mask)));
  return hipGetLastError();
}

hipError_t launch_gnc_weights(int r, int b, const GncEntries& g, const double* X, const double* RX,
                              const RobustParams& rp, double* w_prob, double* w_g, const unsigned char* fixed,
                              hipStream_t stream) {
  if (g.n == 0) return hipSuccess;
  const int grid = (g.n + kThreads - 1) / kThreads;
  if (fixed) {
    DPGO_DISPATCH(r, b, (k_gnc_weights<R, B - 1, true><<<grid, kThreads, 0, stream>>>(g, X, RX, rp, w_prob, w_g, fixed)));
  } else {
    DPGO_DISPATCH(r, b, (k_gnc_weights<R, B - 1, false><<<grid, kThreads, 0, stream>>>(g, X, RX, rp, w_prob, w_g, nullptr)));
  }
  return hipGetLastError();
}

// ---- Lanczos helpers (certificate) ---------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_dot_multi(long len, const double* __restrict__ w,
                                                        const double* __restrict__ basis, int k,
                                                        double* __restrict__ partial) {
  __shared__ double red[kThreads / 64];
  const long chunk = (len + gridDim.x - 1) / gridDim.x;
  const long beg = chunk * blockIdx.x, end = min(len, beg + chunk);
  for (int j = 0; j < k; ++j) {
    const double* v = basis + static_cast<long>(j) * len;
    double s = 0.0;
    for (long x = beg + threadIdx.x; x < end; x += kThreads) s = fma(w[x], v[x], s);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[static_cast<long>(blockIdx.x) * k + j] = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void k_axpy_multi(long len, double* __restrict__ w,
                                                         const double* __restrict__ basis, int k,
                                                         const double* __restrict__ c) {
  for (long x = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; x < len;
       x += static_cast<long>(gridDim.x) * kThreads) {
    double s = w[x];
    for (int j = 0; j < k; ++j) s = fma(-c[j], basis[static_cast<long>(j) * len + x], s);
    w[x] = s;
  }
}

__global__ __launch_bounds__(kThreads) void k_scale(long len, const double* __restrict__ src, double s,
                                                    double* __restrict__ dst) {
  for (long x = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; x < len;
       x += static_cast<long>(gridDim.x) * kThreads)
    dst[x] = src[x] * s;
}

__global__ __launch_bounds__(kThreads) void k_strided_copy(long len, const double* __restrict__ src, int ss,
                                                           double* __restrict__ dst, int ds) {
  for (long x = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; x < len;
       x += static_cast<long>(gridDim.x) * kThreads)
    dst[x * ds] = src[x * ss];
}

hipError_t launch_strided_copy(long len, const double* src, int src_stride, double* dst, int dst_stride,
                               hipStream_t stream) {
  if (len == 0) return hipSuccess;
  const long blocks = std::min<long>((len + kThreads - 1) / kThreads, 4096);
  k_strided_copy<<<static_cast<int>(blocks), kThreads, 0, stream>>>(len, src, src_stride, dst, dst_stride);
  return hipGetLastError();
}

hipError_t launch_scale(long len, const double* src, double s, double* dst, hipStream_t stream) {
  if (len == 0) return hipSuccess;
  const long blocks = std::min<long>((len + kThreads - 1) / kThreads, 4096);
  k_scale<<<static_cast<int>(blocks), kThreads, 0, stream>>>(len, src, s, dst);
  return hipGetLastError();
}

hipError_t launch_dot_multi(long len, const double* w, const double* basis, int k, double* partial,
                            hipStream_t stream) {
  if (k == 0) return hipSuccess;
  k_dot_multi<<<kDotBlocks, kThreads, 0, stream>>>(len, w, basis, k, partial);
  return hipGetLastError();
}

hipError_t launch_axpy_multi(long len, double* w, const double* basis, int k, const double* c, hipStream_t stream) {
  if (k == 0 || len == 0) return hipSuccess;
  const long blocks = std::min<long>((len + kThreads - 1) / kThreads, 4096);
  k_axpy_multi<<<static_cast<int>(blocks), kThreads, 0, stream>>>(len, w, basis, k, c);
  return hipGetLastError();
}

hipError_t launch_bj_inverse_diag(int b, int n, const QView& q, double shift, double* Minv, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const int blocks = (n + kThreads - 1) / kThreads;
  if (b == 3)
    k_bj_inverse_diag<3><<<blocks, kThreads, 0, stream>>>(n, q, shift, Minv);
  else if (b == 4)
    k_bj_inverse_diag<4><<<blocks, kThreads, 0, stream>>>(n, q, shift, Minv);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_cert_diag(int b, int n, const double* diag, const double* S, double* out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const int blocks = (n + kThreads - 1) / kThreads;
  if (b == 3)
    k_cert_diag<3><<<blocks, kThreads, 0, stream>>>(n, diag, S, out);
  else if (b == 4)
    k_cert_diag<4><<<blocks, kThreads, 0, stream>>>(n, diag, S, out);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---- Jacobi-PCG kernels (chordal initialisation on the device) --------------------------------
template <int BS, int NR>
__global__ __launch_bounds__(kThreads) void k_pcg_spmv(int n, const int* __restrict__ rowptr, const int* __restrict__ col,
                                                       const double* __restrict__ blk, const double* __restrict__ x,
                                                       double* __restrict__ y) {
  const long p = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x;
  if (p >= n) return;
  double acc[BS][NR];
#pragma unroll
  for (int u = 0; u < BS; ++u)
#pragma unroll
    for (int a = 0; a < NR; ++a) acc[u][a] = 0.0;
  for (int k = rowptr[p]; k < rowptr[p + 1]; ++k) {
    const double* B = blk + static_cast<long>(k) * (BS * BS);
    const double* xv = x + static_cast<long>(col[k]) * (BS * NR);
    double xl[BS][NR], bl[BS][BS];
#pragma unroll
    for (int v = 0; v < BS; ++v)
#pragma unroll
      for (int a = 0; a < NR; ++a) xl[v][a] = xv[v * NR + a];
#pragma unroll
    for (int u = 0; u < BS; ++u)
#pragma unroll
      for (int v = 0; v < BS; ++v) bl[u][v] = B[u * BS + v];
#pragma unroll
    for (int u = 0; u < BS; ++u)
#pragma unroll
      for (int v = 0; v < BS; ++v)
#pragma unroll
        for (int a = 0; a < NR; ++a) acc[u][a] = fma(bl[u][v], xl[v][a], acc[u][a]);
  }
  double* yv = y + p * (BS * NR);
#pragma unroll
  for (int u = 0; u < BS; ++u)
#pragma unroll
    for (int a = 0; a < NR; ++a) yv[u * NR + a] = acc[u][a];
}

// fixed-order block reduction of Q per-thread values into partial[blockIdx.x * Q + q]
template <int Q>
__device__ __forceinline__ void pcg_block_reduce(double (&v)[Q], double* __restrict__ partial) {
  __shared__ double red[kThreads / 64][Q];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < Q; ++q) v[q] = wave_sum(v[q]);
  if (lane == 0)
#pragma unroll
    for (int q = 0; q < Q; ++q) red[wave][q] = v[q];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int q = 0; q < Q; ++q) partial[blockIdx.x * Q + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
}

template <int BS, int NR>
__global__ __launch_bounds__(kThreads) void k_pcg_dot(int n, const double* __restrict__ u, const double* __restrict__ v,
                                                      double* __restrict__ partial) {
  double s[NR];
#pragma unroll
  for (int a = 0; a < NR; ++a) s[a] = 0.0;
  for (long p = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; p < n; p += static_cast<long>(gridDim.x) * kThreads) {
#pragma unroll
    for (int w = 0; w < BS; ++w)
#pragma unroll
      for (int a = 0; a < NR; ++a) s[a] = fma(u[p * (BS * NR) + w * NR + a], v[p * (BS * NR) + w * NR + a], s[a]);
  }
  pcg_block_reduce<NR>(s, partial);
}

template <int BS, int NR>
__global__ __launch_bounds__(kThreads) void k_pcg_update(int n, PcgCoef alpha, const double* __restrict__ pv,
                                                         const double* __restrict__ qv, double* __restrict__ x,
                                                         double* __restrict__ r, double* __restrict__ z,
                                                         const double* __restrict__ minv, double* __restrict__ partial) {
  double s[2 * NR];
#pragma unroll
  for (int a = 0; a < 2 * NR; ++a) s[a] = 0.0;
  for (long p = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; p < n; p += static_cast<long>(gridDim.x) * kThreads) {
    double rl[BS][NR];
    const long o = p * (BS * NR);
#pragma unroll
    for (int w = 0; w < BS; ++w)
#pragma unroll
      for (int a = 0; a < NR; ++a) {
        x[o + w * NR + a] = fma(alpha.v[a], pv[o + w * NR + a], x[o + w * NR + a]);
        rl[w][a] = fma(-alpha.v[a], qv[o + w * NR + a], r[o + w * NR + a]);
        r[o + w * NR + a] = rl[w][a];
      }
    const double* M = minv + p * (BS * BS);
#pragma unroll
    for (int u = 0; u < BS; ++u)
#pragma unroll
      for (int a = 0; a < NR; ++a) {
        double zz = 0.0;
#pragma unroll
        for (int w = 0; w < BS; ++w) zz = fma(M[u * BS + w], rl[w][a], zz);
        z[o + u * NR + a] = zz;
        s[a] = fma(rl[u][a], zz, s[a]);
        s[NR + a] = fma(rl[u][a], rl[u][a], s[NR + a]);
      }
  }
  pcg_block_reduce<2 * NR>(s, partial);
}

template <int BS, int NR>
__global__ __launch_bounds__(kThreads) void k_pcg_dir(int n, PcgCoef beta, const double* __restrict__ z,
                                                      double* __restrict__ pv) {
  for (long p = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; p < n; p += static_cast<long>(gridDim.x) * kThreads)
#pragma unroll
    for (int w = 0; w < BS; ++w)
#pragma unroll
      for (int a = 0; a < NR; ++a) pv[p * (BS * NR) + w * NR + a] = fma(beta.v[a], pv[p * (BS * NR) + w * NR + a], z[p * (BS * NR) + w * NR + a]);
}

#define DPGO_PCG_DISPATCH(BS_, NR_, CALL)                                   \
  switch ((BS_) * 8 + (NR_)) {                                              \
    case 1 * 8 + 2: { constexpr int BS = 1, NR = 2; CALL; break; }          \
    case 1 * 8 + 3: { constexpr int BS = 1, NR = 3; CALL; break; }          \
    case 2 * 8 + 2: { constexpr int BS = 2, NR = 2; CALL; break; }          \
    case 3 * 8 + 3: { constexpr int BS = 3, NR = 3; CALL; break; }          \
    default: return hipErrorInvalidValue;                                   \
  }

hipError_t launch_pcg_spmv(int bs, int nr, int n, const int* rowptr, const int* col, const double* blk,
                           const double* x, double* y, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const int grid = (n + kThreads - 1) / kThreads;
  DPGO_PCG_DISPATCH(bs, nr, (k_pcg_spmv<BS, NR><<<grid, kThreads, 0, stream>>>(n, rowptr, col, blk, x, y)));
  return hipGetLastError();
}

hipError_t launch_pcg_dot(int bs, int nr, int n, const double* u, const double* v, double* partial,
                          hipStream_t stream) {
  DPGO_PCG_DISPATCH(bs, nr, (k_pcg_dot<BS, NR><<<kPcgBlocks, kThreads, 0, stream>>>(n, u, v, partial)));
  return hipGetLastError();
}

hipError_t launch_pcg_update(int bs, int nr, int n, PcgCoef alpha, const double* p, const double* q, double* x,
                             double* r, double* z, const double* minv, double* partial, hipStream_t stream) {
  DPGO_PCG_DISPATCH(bs, nr, (k_pcg_update<BS, NR><<<kPcgBlocks, kThreads, 0, stream>>>(n, alpha, p, q, x, r, z, minv,
                                                                                       partial)));
  return hipGetLastError();
}

hipError_t launch_pcg_dir(int bs, int nr, int n, PcgCoef beta, const double* z, double* p, hipStream_t stream) {
  DPGO_PCG_DISPATCH(bs, nr, (k_pcg_dir<BS, NR><<<kPcgBlocks, kThreads, 0, stream>>>(n, beta, z, p)));
  return hipGetLastError();
}

hipError_t launch_bj_inverse(int b, int n, const QView& q, double shift, double* Minv, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const int blocks = (n + kThreads - 1) / kThreads;
  if (b == 3)
    k_bj_inverse<3><<<blocks, kThreads, 0, stream>>>(n, q, shift, Minv);
  else if (b == 4)
    k_bj_inverse<4><<<blocks, kThreads, 0, stream>>>(n, q, shift, Minv);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---- Block certificate (LOBPCG on the r rows of the lifted layout) ------------------------------
// A block is an R-row slice of the lifted layout: entry (row i, column x) at p[x * ld + i], ld = R (the locked block
// U: R + 1).  Every reduction leaves one partial per workgroup of a grid that depends on the column count alone and
// is finished by k_blk_sum in a fixed order: no atomics, the same bits on every call.
constexpr int kBlkChunk = 64;  // columns per LDS tile of k_blk_gram

// partial[g][i * rows + j] = <row i, row j> over workgroup g's column chunks, i over the first left_rows rows of the
// list's concatenated rows, j over all of them.  The chunk of every block is staged once in LDS (row stride
// kBlkChunk + 1: the rows a wave reads at one column sit on distinct banks) and the products are split over the
// threads, NACC per thread, so one launch reads each block once for all of them.
template <int R>
__global__ __launch_bounds__(kThreads) void k_blk_gram(long nc, BlkList L, int left_rows, int rows,
                                                       double* __restrict__ partial) {
  constexpr int kMaxRows = 6 * R + 1, NACC = (3 * R * kMaxRows + kThreads - 1) / kThreads;
  __shared__ double s[kMaxRows][kBlkChunk + 1];
  const int t = threadIdx.x, nout = left_rows * rows;
  int oi[NACC], oj[NACC];
  double acc[NACC];
#pragma unroll
  for (int q = 0; q < NACC; ++q) {
    const int o = t + q * kThreads;
    oi[q] = o < nout ? o / rows : 0;
    oj[q] = o < nout ? o - oi[q] * rows : 0;
    acc[q] = 0.0;
  }
  const long nchunks = (nc + kBlkChunk - 1) / kBlkChunk;
  for (long ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const long c0 = ch * kBlkChunk;
    const int ncol = static_cast<int>(min(static_cast<long>(kBlkChunk), nc - c0));
    int roff = 0;
    for (int k = 0; k < L.n; ++k) {
      const int ld = L.ld[k];
      const double* __restrict__ p = L.p[k] + c0 * ld;
      for (int e = t; e < kBlkChunk * ld; e += kThreads) {
        const int col = e / ld, row = e - col * ld;
        s[roff + row][col] = col < ncol ? p[e] : 0.0;
      }
      roff += ld;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NACC; ++q) {
      const double* a = s[oi[q]];
      const double* b = s[oj[q]];
      double v = acc[q];
#pragma unroll 8
      for (int c = 0; c < kBlkChunk; ++c) v = fma(a[c], b[c], v);
      acc[q] = v;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < NACC; ++q) {
    const int o = t + q * kThreads;
    if (o < nout) partial[static_cast<long>(blockIdx.x) * nout + o] = acc[q];
  }
}

// out[o] = partial[0][o] + partial[1][o] + ... in that order (one thread per entry, coalesced across entries)
__global__ __launch_bounds__(kThreads) void k_blk_sum(int blocks, int nout, const double* __restrict__ partial,
                                                      double* __restrict__ out) {
  const int o = blockIdx.x * kThreads + threadIdx.x;
  if (o >= nout) return;
  double v = 0.0;
  for (int g = 0; g < blocks; ++g) v += partial[static_cast<long>(g) * nout + o];
  out[o] = v;
}

// the workgroup's per-row sums of nrm into part[block][R]; every thread of the workgroup calls it
template <int R>
__device__ __forceinline__ void blk_row_sums(const double (&nrm)[R], double* __restrict__ part) {
  __shared__ double red[R][kThreads / 64];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const double v = wave_sum(nrm[i]);
    if ((threadIdx.x & 63) == 0) red[i][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < R)
    part[static_cast<long>(blockIdx.x) * R + threadIdx.x] =
        ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

// out = SX - diag(theta) X, and the partials of |out_i|^2 per row
template <int R>
__global__ __launch_bounds__(kThreads) void k_blk_residual(long nc, const double* __restrict__ SX,
                                                           const double* __restrict__ X,
                                                           const double* __restrict__ theta, double* __restrict__ out,
                                                           double* __restrict__ part) {
  double nrm[R];
#pragma unroll
  for (int i = 0; i < R; ++i) nrm[i] = 0.0;
  for (long x = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; x < nc;
       x += static_cast<long>(gridDim.x) * kThreads) {
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const double v = fma(-theta[i], X[x * R + i], SX[x * R + i]);
      out[x * R + i] = v;
      nrm[i] = fma(v, v, nrm[i]);
    }
  }
  blk_row_sums<R>(nrm, part);
}

// V <- V - coef U (coef R x RU at coef[i * ldc + j], left on the device by the cross Gram), and optionally the
// partials of the result's |V_i|^2
template <int R, int RU>
__global__ __launch_bounds__(kThreads) void k_blk_project(long nc, double* __restrict__ V, const double* __restrict__ U,
                                                          const double* __restrict__ coef, int ldc,
                                                          double* __restrict__ part) {
  double nrm[R];
#pragma unroll
  for (int i = 0; i < R; ++i) nrm[i] = 0.0;
  for (long x = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; x < nc;
       x += static_cast<long>(gridDim.x) * kThreads) {
    double u[RU];
#pragma unroll
    for (int j = 0; j < RU; ++j) u[j] = U[x * RU + j];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      double v = V[x * R + i];
#pragma unroll
      for (int j = 0; j < RU; ++j) v = fma(-coef[i * ldc + j], u[j], v);
      V[x * R + i] = v;
      nrm[i] = fma(v, v, nrm[i]);
    }
  }
  if (part != nullptr) blk_row_sums<R>(nrm, part);  // uniform over the workgroup
}

// V <- T V per column (T R x R row-major on the device)
template <int R>
__global__ __launch_bounds__(kThreads) void k_blk_transform(long nc, double* __restrict__ V,
                                                            const double* __restrict__ T) {
  for (long x = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; x < nc;
       x += static_cast<long>(gridDim.x) * kThreads) {
    double v[R], o[R];
#pragma unroll
    for (int j = 0; j < R; ++j) v[j] = V[x * R + j];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      double a = 0.0;
#pragma unroll
      for (int j = 0; j < R; ++j) a = fma(T[i * R + j], v[j], a);
      o[i] = a;
    }
#pragma unroll
    for (int i = 0; i < R; ++i) V[x * R + i] = o[i];
  }
}

// The Rayleigh-Ritz update, in place per column: x' = cx [x; w; p], p' = cp [x; w; p] (R x 3R row-major tiles on the
// device; cp's x part is zero and not read), for the vector blocks (blockIdx.y 0) and their operator images (1) in
// one launch.  has_p == 0: the p block does not exist yet and is not read.
template <int R>
__global__ __launch_bounds__(kThreads) void k_blk_combine(long nc, BlkCombine a) {
  double* __restrict__ X = blockIdx.y == 0 ? a.x : a.sx;
  const double* __restrict__ W = blockIdx.y == 0 ? a.w : a.sw;
  double* __restrict__ P = blockIdx.y == 0 ? a.p : a.sp;
  const double* __restrict__ cx = a.cx;
  const double* __restrict__ cp = a.cp;
  const bool has_p = a.has_p != 0;
  for (long x = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x; x < nc;
       x += static_cast<long>(gridDim.x) * kThreads) {
    double z[3 * R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      z[j] = X[x * R + j];
      z[R + j] = W[x * R + j];
      z[2 * R + j] = has_p ? P[x * R + j] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < R; ++i) {
      double xo = 0.0, po = 0.0;
#pragma unroll
      for (int j = 0; j < 3 * R; ++j) xo = fma(cx[i * 3 * R + j], z[j], xo);
#pragma unroll
      for (int j = R; j < 3 * R; ++j) po = fma(cp[i * 3 * R + j], z[j], po);
      X[x * R + i] = xo;
      P[x * R + i] = po;
    }
  }
}

// V_j <- V_j Minv_j per pose (the block-Jacobi inverses as launch_bj_inverse* leave them), one thread per pose
template <int R, int B>
__global__ __launch_bounds__(kThreads) void k_blk_precond(long n, double* __restrict__ V,
                                                          const double* __restrict__ Minv) {
  const long j = static_cast<long>(blockIdx.x) * kThreads + threadIdx.x;
  if (j >= n) return;
  double M[B][B], v[R][B];
#pragma unroll
  for (int u = 0; u < B; ++u)
#pragma unroll
    for (int w = 0; w < B; ++w) M[u][w] = Minv[j * diag_width(B - 1) + minv_index<B>(u, w)];
#pragma unroll
  for (int k = 0; k < B; ++k)
#pragma unroll
    for (int a = 0; a < R; ++a) v[a][k] = V[(j * B + k) * R + a];
#pragma unroll
  for (int k = 0; k < B; ++k)
#pragma unroll
    for (int a = 0; a < R; ++a) {
      double z = 0.0;
#pragma unroll
      for (int u = 0; u < B; ++u) z = fma(v[a][u], M[u][k], z);
      V[(j * B + k) * R + a] = z;
    }
}

// T (R x R row-major) with T G T^T = I on the kept directions of the R x R Gram matrix G (G[i * ldg + j],
// symmetrised here): cyclic Jacobi by one thread, rows of T by descending eigenvalue, T_i = z_i / sqrt(e_i); an
// eigenvalue at or below drop * the largest gives a zero row (and so does anything that is not a number).
template <int R>
__global__ __launch_bounds__(64) void k_blk_orthcoef(const double* __restrict__ G, int ldg, double drop,
                                                     double* __restrict__ T) {
  __shared__ double a[R][R], v[R][R], e[R];
  __shared__ int ord[R];
  if (threadIdx.x != 0) return;
  for (int i = 0; i < R; ++i)
    for (int j = 0; j < R; ++j) {
      a[i][j] = 0.5 * (G[i * ldg + j] + G[j * ldg + i]);
      v[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, dia = 0.0;
    for (int i = 0; i < R; ++i)
      for (int j = 0; j < R; ++j) (i == j ? dia : off) += a[i][j] * a[i][j];
    if (!(off > 1e-34 * dia)) break;
    for (int p = 0; p + 1 < R; ++p)
      for (int q = p + 1; q < R; ++q) {
        const double apq = a[p][q];
        if (apq == 0.0) continue;
        const double tau = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double c = 1.0 / sqrt(1.0 + tt * tt), sn = tt * c;
        for (int k = 0; k < R; ++k) {
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - sn * akq;
          a[k][q] = sn * akp + c * akq;
        }
        for (int k = 0; k < R; ++k) {
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - sn * aqk;
          a[q][k] = sn * apk + c * aqk;
        }
        for (int k = 0; k < R; ++k) {
          const double vkp = v[k][p], vkq = v[k][q];
          v[k][p] = c * vkp - sn * vkq;
          v[k][q] = sn * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < R; ++i) {
    e[i] = a[i][i];
    ord[i] = i;
  }
  for (int i = 0; i + 1 < R; ++i)  // descending, ties by index
    for (int j = i + 1; j < R; ++j)
      if (e[ord[j]] > e[ord[i]]) {
        const int tmp = ord[i];
        ord[i] = ord[j];
        ord[j] = tmp;
      }
  const double emax = e[ord[0]];
  for (int i = 0; i < R; ++i) {
    const int c = ord[i];
    const bool keep = emax > 0.0 && e[c] > drop * emax;
    const double sc = keep ? 1.0 / sqrt(e[c]) : 0.0;
    for (int j = 0; j < R; ++j) T[i * R + j] = keep ? v[j][c] * sc : 0.0;
  }
}

#define DPGO_DISPATCH_R(R_, CALL)                     \
  switch (R_) {                                       \
    case 2: { constexpr int R = 2; CALL; break; }     \
    case 3: { constexpr int R = 3; CALL; break; }     \
    case 4: { constexpr int R = 4; CALL; break; }     \
    case 5: { constexpr int R = 5; CALL; break; }     \
    case 6: { constexpr int R = 6; CALL; break; }     \
    case 7: { constexpr int R = 7; CALL; break; }     \
    case 8: { constexpr int R = 8; CALL; break; }     \
    default: return hipErrorInvalidValue;             \
  }

static int blk_vec_grid(long nc) {
  return static_cast<int>(std::min<long>((nc + kThreads - 1) / kThreads, kBlkVecBlocks));
}

hipError_t launch_blk_gram(int r, long nc, const BlkList& L, int nleft, double* partial, double* out,
                           hipStream_t stream) {
  if (nc <= 0 || L.n < 1 || L.n > 6 || nleft < 1 || nleft > L.n || nleft > 3) return hipErrorInvalidValue;
  int rows = 0, left_rows = 0;
  for (int k = 0; k < L.n; ++k) {
    if (L.p[k] == nullptr || (L.ld[k] != r && L.ld[k] != r + 1)) return hipErrorInvalidValue;
    rows += L.ld[k];
    if (k < nleft) left_rows += L.ld[k];
  }
  if (rows > 6 * r + 1 || left_rows > 3 * r) return hipErrorInvalidValue;
  const int grid = blk_gram_grid(nc), nout = left_rows * rows;
  DPGO_DISPATCH_R(r, (k_blk_gram<R><<<grid, kThreads, 0, stream>>>(nc, L, left_rows, rows, partial)));
  k_blk_sum<<<(nout + kThreads - 1) / kThreads, kThreads, 0, stream>>>(grid, nout, partial, out);
  return hipGetLastError();
}

hipError_t launch_blk_residual(int r, long nc, const double* SX, const double* X, const double* theta, double* out,
                               double* partial, double* norms, hipStream_t stream) {
  if (nc <= 0) return hipErrorInvalidValue;
  const int grid = blk_vec_grid(nc);
  DPGO_DISPATCH_R(r, (k_blk_residual<R><<<grid, kThreads, 0, stream>>>(nc, SX, X, theta, out, partial)));
  k_blk_sum<<<1, kThreads, 0, stream>>>(grid, r, partial, norms);
  return hipGetLastError();
}

hipError_t launch_blk_project(int r, int ru, long nc, double* V, const double* U, const double* coef, int ldc,
                              double* partial, double* norms, hipStream_t stream) {
  if (nc <= 0 || (ru != r && ru != r + 1) || (partial == nullptr) != (norms == nullptr)) return hipErrorInvalidValue;
  const int grid = blk_vec_grid(nc);
  if (ru == r) {
    DPGO_DISPATCH_R(r, (k_blk_project<R, R><<<grid, kThreads, 0, stream>>>(nc, V, U, coef, ldc, partial)));
  } else {
    DPGO_DISPATCH_R(r, (k_blk_project<R, R + 1><<<grid, kThreads, 0, stream>>>(nc, V, U, coef, ldc, partial)));
  }
  if (partial != nullptr) k_blk_sum<<<1, kThreads, 0, stream>>>(grid, r, partial, norms);
  return hipGetLastError();
}

hipError_t launch_blk_transform(int r, long nc, double* V, const double* T, hipStream_t stream) {
  if (nc <= 0) return hipErrorInvalidValue;
  DPGO_DISPATCH_R(r, (k_blk_transform<R><<<blk_vec_grid(nc), kThreads, 0, stream>>>(nc, V, T)));
  return hipGetLastError();
}

hipError_t launch_blk_combine(int r, long nc, const BlkCombine& a, hipStream_t stream) {
  if (nc <= 0) return hipErrorInvalidValue;
  const dim3 grid(blk_vec_grid(nc), 2);
  DPGO_DISPATCH_R(r, (k_blk_combine<R><<<grid, kThreads, 0, stream>>>(nc, a)));
  return hipGetLastError();
}

hipError_t launch_blk_precond(int r, int b, long n, double* V, const double* Minv, hipStream_t stream) {
  if (n <= 0) return hipErrorInvalidValue;
  const int grid = static_cast<int>((n + kThreads - 1) / kThreads);
  DPGO_DISPATCH(r, b, (k_blk_precond<R, B><<<grid, kThreads, 0, stream>>>(n, V, Minv)));
  return hipGetLastError();
}

hipError_t launch_blk_orthcoef(int r, const double* G, int ldg, double drop, double* T, hipStream_t stream) {
  DPGO_DISPATCH_R(r, (k_blk_orthcoef<R><<<1, 64, 0, stream>>>(G, ldg, drop, T)));
  return hipGetLastError();
}

#endif  // !DPGO_SPMM_TU

}  // namespace dpgo

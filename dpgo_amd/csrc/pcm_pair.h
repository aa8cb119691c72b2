// The pair test of the pairwise consistency check (include/dpgo_hip.h): one function, compiled into the
// kernel (kernels.hip) and into the host twin (pcm.cpp), so both run the same sums in the same order.  Contraction is
// off inside it on both sides: every multiplication and addition rounds on its own, no FMA is formed, and the device
// and the host give the same bits.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define DPGO_PCM_HD __host__ __device__
#else
#define DPGO_PCM_HD
#endif

namespace dpgo {

// A candidate's record: F (D x (D + 1) column-major: R then t) followed by the lever point x.
template <int D>
constexpr int pcm_record() {
  return D * (D + 1) + D;
}

// e_rot = |R_k - R_l|_F^2, e_tra = 1/2 (|dR x_k + dt|^2 + |dR x_l + dt|^2) of the records a (k) and b (l).
// The differences are formed first, so (b, a) negates every term of (a, b) exactly and both results are symmetric.
template <int D>
DPGO_PCM_HD inline void pcm_pair_errors(const double* a, const double* b, double& e_rot, double& e_tra) {
#pragma clang fp contract(off)
  constexpr int PW = D * (D + 1);
  double dR[D * D], dt[D];
  double rot = 0.0;
#pragma unroll
  for (int x = 0; x < D * D; ++x) {
    dR[x] = a[x] - b[x];
    const double sq = dR[x] * dR[x];
    rot = rot + sq;
  }
#pragma unroll
  for (int i = 0; i < D; ++i) dt[i] = a[D * D + i] - b[D * D + i];
  double s[2];
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const double* lever = (side == 0 ? a : b) + PW;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double v = dR[i] * lever[0];
#pragma unroll
      for (int c = 1; c < D; ++c) {
        const double p = dR[c * D + i] * lever[c];
        v = v + p;
      }
      v = v + dt[i];
      const double sq = v * v;
      acc = acc + sq;
    }
    s[side] = acc;
  }
  e_rot = rot;
  e_tra = 0.5 * (s[0] + s[1]);
}

// A(k, l) for k != l: NaN on either side of a comparison gives false
DPGO_PCM_HD inline bool pcm_consistent(double e_rot, double e_tra, double cR2, double ct2) {
  return e_rot <= cR2 && e_tra <= ct2;
}

}  // namespace dpgo

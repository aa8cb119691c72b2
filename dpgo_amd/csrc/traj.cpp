// Trajectory evaluation against a ground truth (build-defined): the C ABI of the moment,
// error and relative-pose kernels, the host alignment step, the vertex reader and dpgo_graph_evaluate.
// See include/dpgo_hip.h and include/dpgo_rbcd.h.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "graph_internal.h"

using namespace dpgo;

namespace {

constexpr const char* kNoDevice = "no gfx950 device available (no CPU fallback)";

bool overlap(const void* a, size_t bytes_a, const void* b, size_t bytes_b) {
  if (!a || !b) return false;
  const auto pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + bytes_b && pb < pa + bytes_a;
}

struct Span {
  const void* p;
  size_t bytes;
};
// true when an output overlaps an input or another output (null spans never overlap)
bool outputs_overlap(const std::vector<Span>& in, const std::vector<Span>& out) {
  for (size_t i = 0; i < out.size(); ++i) {
    for (const Span& s : in)
      if (overlap(out[i].p, out[i].bytes, s.p, s.bytes)) return true;
    for (size_t j = i + 1; j < out.size(); ++j)
      if (overlap(out[i].p, out[i].bytes, out[j].p, out[j].bytes)) return true;
  }
  return false;
}

int check_traj(const char* who, int d, long long n, const void* That, const void* T) {
  if (d != 2 && d != 3) return fail(DPGO_HIP_EINVAL, std::string(who) + ": d must be 2 or 3");
  if (n <= 0) return fail(DPGO_HIP_EINVAL, std::string(who) + ": need n >= 1 poses");
  if (!That || !T) return fail(DPGO_HIP_EINVAL, std::string(who) + ": null trajectory");
  return DPGO_HIP_OK;
}

double det_small(int d, const double A[3][3]) {
  return d == 2 ? A[0][0] * A[1][1] - A[0][1] * A[1][0]
                : A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                      A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
}

// C = U diag(sig) V^T of a d x d matrix by the one-sided Jacobi sweep of project_rotation (init.cpp): the columns
// of W = C V are made orthogonal, their norms are the singular values, sorted descending.  A zero column of W
// leaves its column of U open: it is completed from the canonical basis by Gram-Schmidt, so U is always orthogonal.
void svd_small(int d, const double C[3][3], double U[3][3], double sig[3], double V[3][3]) {
  double W[3][3], Vv[3][3];
  for (int a = 0; a < d; ++a)
    for (int c = 0; c < d; ++c) {
      W[a][c] = C[a][c];
      Vv[a][c] = a == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rot = false;
    for (int p = 0; p < d - 1; ++p)
      for (int q = p + 1; q < d; ++q) {
        double al = 0, be = 0, ga = 0;
        for (int a = 0; a < d; ++a) {
          al += W[a][p] * W[a][p];
          be += W[a][q] * W[a][q];
          ga += W[a][p] * W[a][q];
        }
        if (std::fabs(ga) <= 1e-17 * std::sqrt(al * be) || ga == 0.0) continue;
        rot = true;
        const double zeta = (be - al) / (2 * ga);
        const double t = std::copysign(1.0, zeta) / (std::fabs(zeta) + std::sqrt(1 + zeta * zeta));
        const double c = 1 / std::sqrt(1 + t * t), s = c * t;
        for (int a = 0; a < d; ++a) {
          const double wp = W[a][p], wq = W[a][q];
          W[a][p] = c * wp - s * wq;
          W[a][q] = s * wp + c * wq;
          const double vp = Vv[a][p], vq = Vv[a][q];
          Vv[a][p] = c * vp - s * vq;
          Vv[a][q] = s * vp + c * vq;
        }
      }
    if (!rot) break;
  }
  double nrm[3];
  int order[3] = {0, 1, 2};
  for (int c = 0; c < d; ++c) {
    double s = 0;
    for (int a = 0; a < d; ++a) s += W[a][c] * W[a][c];
    nrm[c] = std::sqrt(s);
  }
  for (int i = 1; i < d; ++i)  // insertion sort, stable, descending
    for (int j = i; j > 0 && nrm[order[j]] > nrm[order[j - 1]]; --j) std::swap(order[j], order[j - 1]);
  for (int i = 0; i < d; ++i) {
    const int c = order[i];
    sig[i] = nrm[c];
    for (int a = 0; a < d; ++a) {
      U[a][i] = nrm[c] > 0 ? W[a][c] / nrm[c] : 0.0;
      V[a][i] = Vv[a][c];
    }
  }
  for (int i = 0; i < d; ++i) {
    if (sig[i] > 0) continue;
    double best[3] = {0, 0, 0}, best_n = -1.0;
    for (int k = 0; k < d; ++k) {  // the canonical vector that keeps the most after the filled columns are removed
      double v[3] = {0, 0, 0};
      v[k] = 1.0;
      for (int pass = 0; pass < 2; ++pass)
        for (int c = 0; c < d; ++c) {
          if (c >= i && !(sig[c] > 0)) continue;  // not filled yet
          double dot = 0;
          for (int a = 0; a < d; ++a) dot += U[a][c] * v[a];
          for (int a = 0; a < d; ++a) v[a] -= dot * U[a][c];
        }
      double s = 0;
      for (int a = 0; a < d; ++a) s += v[a] * v[a];
      if (s > best_n) {
        best_n = s;
        for (int a = 0; a < d; ++a) best[a] = v[a];
      }
    }
    const double s = std::sqrt(best_n);
    for (int a = 0; a < d; ++a) U[a][i] = best[a] / s;
  }
}

// the alignment step on validated arguments; Aa and info are written only on success
int align_from_moments(int d, const double* shift, const double* mom, double rank_tol, double* Aa,
                       dpgo_align_info* info) {
  const int P = DPGO_TRAJ_MOMENTS(d);
  for (int i = 0; i < P; ++i)
    if (!std::isfinite(mom[i])) return fail(DPGO_HIP_EINVAL, "align_moments: a moment is not finite");
  const double n = mom[0];
  if (!(n >= 1.0)) return fail(DPGO_HIP_EINVAL, "align_moments: no pose counted");
  if (!(rank_tol > 0.0)) rank_tol = 1e-12;
  const double* sa = mom + 3;
  const double* sb = mom + 3 + d;
  const double* M = mom + 3 + 2 * d;
  double muh[3], mu[3], C[3][3], U[3][3], V[3][3], sig[3] = {0, 0, 0};
  for (int i = 0; i < d; ++i) {
    muh[i] = (shift ? shift[i] : 0.0) + sa[i] / n;
    mu[i] = (shift ? shift[d + i] : 0.0) + sb[i] / n;
    if (!std::isfinite(muh[i]) || !std::isfinite(mu[i]))
      return fail(DPGO_HIP_EINVAL, "align_moments: the shift is not finite");
  }
  for (int i = 0; i < d; ++i)
    for (int c = 0; c < d; ++c) C[i][c] = M[c * d + i] - sb[i] * sa[c] / n;
  svd_small(d, C, U, sig, V);
  const double s = det_small(d, U) * det_small(d, V) < 0 ? -1.0 : 1.0;
  double A[3][3];
  const bool zero = !(sig[0] > 0);  // C = 0 (one pose, or all poses equal): A = I
  for (int i = 0; i < d; ++i)
    for (int k = 0; k < d; ++k) {
      double v = 0;
      for (int c = 0; c < d; ++c) v += U[i][c] * (c == d - 1 ? s : 1.0) * V[k][c];
      A[i][k] = zero ? (i == k ? 1.0 : 0.0) : v;
    }
  for (int k = 0; k < d; ++k)
    for (int i = 0; i < d; ++i) Aa[k * d + i] = A[i][k];
  for (int i = 0; i < d; ++i) {
    double v = 0;
    for (int k = 0; k < d; ++k) v += A[i][k] * muh[k];
    Aa[d * d + i] = mu[i] - v;
  }
  if (info) {
    info->count = n;
    info->rank = 0;
    for (int i = 0; i < 3; ++i) info->sigma[i] = i < d ? sig[i] : std::nan("");
    for (int i = 0; i < d; ++i) info->rank += sig[i] > rank_tol * sig[0] ? 1 : 0;
    if (!zero) info->sigma[d - 1] *= s;
  }
  return DPGO_HIP_OK;
}

// the two moment launches and the host step on device trajectories; waits for the stream twice.
// md: DPGO_TRAJ_MOMENTS(d) device doubles, work: dpgo_hip_traj_moments_work_doubles
int align_dev(int d, long long n, const double* That, const double* T, const int* use, double* md, double* work,
              hipStream_t s, double* Aa, dpgo_align_info* info) {
  const int P = DPGO_TRAJ_MOMENTS(d);
  double mom[DPGO_TRAJ_MOMENTS(3)], shift[6];
  HIP_TRY(launch_traj_moments(d, static_cast<long>(n), That, T, use, nullptr, md, work, s));
  HIP_TRY(hipMemcpyAsync(mom, md, sizeof(double) * P, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (!(mom[0] >= 1.0)) return fail(DPGO_HIP_EINVAL, "traj_align: no pose counted");
  for (int i = 0; i < 2 * d; ++i) {
    shift[i] = mom[3 + i] / mom[0];
    if (!std::isfinite(shift[i])) return fail(DPGO_HIP_EINVAL, "traj_align: a used pose is not finite");
  }
  HIP_TRY(launch_traj_moments(d, static_cast<long>(n), That, T, use, shift, md, work, s));
  HIP_TRY(hipMemcpyAsync(mom, md, sizeof(double) * P, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return align_from_moments(d, shift, mom, 0.0, Aa, info);
}

// That, T and the mask on the device, one allocation of doubles and one of ints
struct DevTraj {
  DevBuf<double> buf;
  DevBuf<int> mask;
  double* That = nullptr;
  double* T = nullptr;
  double* extra = nullptr;  // `extra_doubles` doubles behind the trajectories
  int* use = nullptr;
  int upload(int d, int n, const double* That_h, const double* T_h, const int* use_h, size_t extra_doubles,
             hipStream_t s) {
    const size_t len = static_cast<size_t>(d) * (d + 1) * n;
    HIP_TRY(buf.ensure(2 * len + extra_doubles));
    That = buf.p;
    T = buf.p + len;
    extra = buf.p + 2 * len;
    HIP_TRY(hipMemcpyAsync(That, That_h, sizeof(double) * len, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(T, T_h, sizeof(double) * len, hipMemcpyHostToDevice, s));
    if (use_h) {
      HIP_TRY(mask.ensure(n));
      HIP_TRY(hipMemcpyAsync(mask.p, use_h, sizeof(int) * n, hipMemcpyHostToDevice, s));
      use = mask.p;
    }
    return DPGO_HIP_OK;
  }
};

}  // namespace

extern "C" {

// ----------------------------------------------------------------------- moments
long long dpgo_hip_traj_moments_work_doubles(int d, long long n) {
  if ((d != 2 && d != 3) || n <= 0) return 0;
  return static_cast<long long>(traj_blocks(static_cast<long>(n))) * traj_moments_len(d);
}

int dpgo_hip_traj_moments_dev(int d, long long n, const double* That_dev, const double* T_dev, const int* use_dev,
                              const double* shift, double* mom_dev, double* work_dev, void* stream) {
  DPGO_TRY(check_traj("traj_moments", d, n, That_dev, T_dev));
  if (!mom_dev) return fail(DPGO_HIP_EINVAL, "traj_moments: null mom");
  if (!work_dev) return fail(DPGO_HIP_EINVAL, "traj_moments: null work buffer (dpgo_hip_traj_moments_work_doubles)");
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  HIP_TRY(launch_traj_moments(d, static_cast<long>(n), That_dev, T_dev, use_dev, shift, mom_dev, work_dev,
                              static_cast<hipStream_t>(stream)));
  return DPGO_HIP_OK;
}

int dpgo_hip_traj_moments(int d, int n, const double* That, const double* T, const int* use, const double* shift,
                          double* mom) {
  DPGO_TRY(check_traj("traj_moments", d, n, That, T));
  if (!mom) return fail(DPGO_HIP_EINVAL, "traj_moments: null mom");
  const size_t len = sizeof(double) * d * (d + 1) * n, P = DPGO_TRAJ_MOMENTS(d);
  if (outputs_overlap({{That, len}, {T, len}, {use, sizeof(int) * n}, {shift, sizeof(double) * 2 * d}},
                      {{mom, sizeof(double) * P}}))
    return fail(DPGO_HIP_EINVAL, "traj_moments: mom overlaps an input");
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  hipStream_t s = nullptr;
  DevTraj D;
  const size_t work = static_cast<size_t>(dpgo_hip_traj_moments_work_doubles(d, n));
  DPGO_TRY(D.upload(d, n, That, T, use, P + work, s));
  DPGO_TRY(dpgo_hip_traj_moments_dev(d, n, D.That, D.T, D.use, shift, D.extra, D.extra + P, s));
  HIP_TRY(hipMemcpyAsync(mom, D.extra, sizeof(double) * P, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DPGO_HIP_OK;
}

int dpgo_hip_align_moments(int d, const double* shift, const double* mom, double rank_tol, double* Aa,
                           dpgo_align_info* info) {
  if (d != 2 && d != 3) return fail(DPGO_HIP_EINVAL, "align_moments: d must be 2 or 3");
  if (!mom || !Aa) return fail(DPGO_HIP_EINVAL, "align_moments: null mom or Aa");
  const size_t P = DPGO_TRAJ_MOMENTS(d);
  if (outputs_overlap({{mom, sizeof(double) * P}, {shift, sizeof(double) * 2 * d}},
                      {{Aa, sizeof(double) * d * (d + 1)}, {info, sizeof(dpgo_align_info)}}))
    return fail(DPGO_HIP_EINVAL, "align_moments: an output overlaps an input or another output");
  double out[12];
  dpgo_align_info I{};
  DPGO_TRY(align_from_moments(d, shift, mom, rank_tol, out, &I));
  std::memcpy(Aa, out, sizeof(double) * d * (d + 1));
  if (info) *info = I;
  return DPGO_HIP_OK;
}

int dpgo_hip_traj_align(int d, int n, const double* That, const double* T, const int* use, double* Aa,
                        dpgo_align_info* info) {
  DPGO_TRY(check_traj("traj_align", d, n, That, T));
  if (!Aa) return fail(DPGO_HIP_EINVAL, "traj_align: null Aa");
  const size_t len = sizeof(double) * d * (d + 1) * n, P = DPGO_TRAJ_MOMENTS(d);
  if (outputs_overlap({{That, len}, {T, len}, {use, sizeof(int) * n}},
                      {{Aa, sizeof(double) * d * (d + 1)}, {info, sizeof(dpgo_align_info)}}))
    return fail(DPGO_HIP_EINVAL, "traj_align: an output overlaps an input or another output");
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  hipStream_t s = nullptr;
  DevTraj D;
  const size_t work = static_cast<size_t>(dpgo_hip_traj_moments_work_doubles(d, n));
  DPGO_TRY(D.upload(d, n, That, T, use, P + work, s));
  double out[12];
  dpgo_align_info I{};
  DPGO_TRY(align_dev(d, n, D.That, D.T, D.use, D.extra, D.extra + P, s, out, &I));
  std::memcpy(Aa, out, sizeof(double) * d * (d + 1));
  if (info) *info = I;
  return DPGO_HIP_OK;
}

// ----------------------------------------------------------------------- errors
long long dpgo_hip_traj_errors_work_doubles(int d, long long n) {
  if ((d != 2 && d != 3) || n <= 0) return 0;
  return static_cast<long long>(traj_blocks(static_cast<long>(n))) * kTrajSums;
}

int dpgo_hip_traj_errors_dev(int d, long long n, const double* That_dev, const double* T_dev, const int* use_dev,
                             const double* Aa, double* tra_sq_dev, double* rot_sq_dev, double* sums_dev,
                             double* work_dev, void* stream) {
  DPGO_TRY(check_traj("traj_errors", d, n, That_dev, T_dev));
  if (!tra_sq_dev && !rot_sq_dev && !sums_dev) return fail(DPGO_HIP_EINVAL, "traj_errors: no output requested");
  if (sums_dev && !work_dev)
    return fail(DPGO_HIP_EINVAL, "traj_errors: the sums need a work buffer (dpgo_hip_traj_errors_work_doubles)");
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  HIP_TRY(launch_traj_errors(d, static_cast<long>(n), That_dev, T_dev, use_dev, Aa, tra_sq_dev, rot_sq_dev, sums_dev,
                             work_dev, static_cast<hipStream_t>(stream)));
  return DPGO_HIP_OK;
}

int dpgo_hip_traj_errors(int d, int n, const double* That, const double* T, const int* use, const double* Aa,
                         double* tra_sq, double* rot_sq, double* sums) {
  DPGO_TRY(check_traj("traj_errors", d, n, That, T));
  if (!tra_sq && !rot_sq && !sums) return fail(DPGO_HIP_EINVAL, "traj_errors: no output requested");
  const size_t len = sizeof(double) * d * (d + 1) * n, per = sizeof(double) * n;
  if (outputs_overlap({{That, len}, {T, len}, {use, sizeof(int) * n}, {Aa, sizeof(double) * d * (d + 1)}},
                      {{tra_sq, per}, {rot_sq, per}, {sums, sizeof(double) * DPGO_TRAJ_SUMS}}))
    return fail(DPGO_HIP_EINVAL, "traj_errors: an output overlaps an input or another output");
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  hipStream_t s = nullptr;
  DevTraj D;
  const size_t N = static_cast<size_t>(n), work = static_cast<size_t>(dpgo_hip_traj_errors_work_doubles(d, n));
  DPGO_TRY(D.upload(d, n, That, T, use, 2 * N + DPGO_TRAJ_SUMS + work, s));
  double* o = D.extra;  // tra_sq, rot_sq, sums, partials
  DPGO_TRY(dpgo_hip_traj_errors_dev(d, n, D.That, D.T, D.use, Aa, tra_sq ? o : nullptr, rot_sq ? o + N : nullptr,
                                    sums ? o + 2 * N : nullptr, o + 2 * N + DPGO_TRAJ_SUMS, s));
  if (tra_sq) HIP_TRY(hipMemcpyAsync(tra_sq, o, per, hipMemcpyDeviceToHost, s));
  if (rot_sq) HIP_TRY(hipMemcpyAsync(rot_sq, o + N, per, hipMemcpyDeviceToHost, s));
  if (sums) HIP_TRY(hipMemcpyAsync(sums, o + 2 * N, sizeof(double) * DPGO_TRAJ_SUMS, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DPGO_HIP_OK;
}

// ----------------------------------------------------------------------- relative poses
int dpgo_hip_relative_poses_dev(int d, long long n, const double* T_dev, long long m, const int* p1_dev,
                                const int* p2_dev, double* R_out_dev, double* t_out_dev, void* stream) {
  if (d != 2 && d != 3) return fail(DPGO_HIP_EINVAL, "relative_poses: d must be 2 or 3");
  if (n <= 0 || m <= 0) return fail(DPGO_HIP_EINVAL, "relative_poses: need n >= 1 poses and m >= 1 edges");
  if (!T_dev || !p1_dev || !p2_dev || !R_out_dev || !t_out_dev)
    return fail(DPGO_HIP_EINVAL, "relative_poses: null T, p1, p2, R_out or t_out");
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  HIP_TRY(launch_relative_poses(d, static_cast<long>(m), p1_dev, p2_dev, T_dev, R_out_dev, t_out_dev,
                                static_cast<hipStream_t>(stream)));
  return DPGO_HIP_OK;
}

int dpgo_hip_relative_poses(int d, int n, const double* T, int m, const int* p1, const int* p2, double* R_out,
                            double* t_out) {
  if (d != 2 && d != 3) return fail(DPGO_HIP_EINVAL, "relative_poses: d must be 2 or 3");
  if (n <= 0 || m <= 0) return fail(DPGO_HIP_EINVAL, "relative_poses: need n >= 1 poses and m >= 1 edges");
  if (!T || !p1 || !p2 || !R_out || !t_out)
    return fail(DPGO_HIP_EINVAL, "relative_poses: null T, p1, p2, R_out or t_out");
  const size_t M = static_cast<size_t>(m), dd = static_cast<size_t>(d) * d, len = dd + d;
  if (outputs_overlap({{T, sizeof(double) * len * n}, {p1, sizeof(int) * M}, {p2, sizeof(int) * M}},
                      {{R_out, sizeof(double) * dd * M}, {t_out, sizeof(double) * d * M}}))
    return fail(DPGO_HIP_EINVAL, "relative_poses: an output overlaps an input or the other output");
  for (size_t k = 0; k < M; ++k) {
    const int i = p1[k], j = p2[k];
    if (i < 0 || i >= n || j < 0 || j >= n) return fail(DPGO_HIP_EINVAL, "relative_poses: pose index outside [0, n)");
    if (i == j) return fail(DPGO_HIP_EINVAL, "relative_poses: an edge needs two different poses");
  }
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  DevBuf<double> buf;
  DevBuf<int> idx;
  HIP_TRY(buf.ensure(len * n + len * M));
  HIP_TRY(idx.ensure(2 * M));
  hipStream_t s = nullptr;
  double* Ro = buf.p + len * n;
  double* to = Ro + dd * M;
  HIP_TRY(hipMemcpyAsync(buf.p, T, sizeof(double) * len * n, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(idx.p, p1, sizeof(int) * M, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(idx.p + M, p2, sizeof(int) * M, hipMemcpyHostToDevice, s));
  DPGO_TRY(dpgo_hip_relative_poses_dev(d, n, buf.p, m, idx.p, idx.p + M, Ro, to, s));
  HIP_TRY(hipMemcpyAsync(R_out, Ro, sizeof(double) * dd * M, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(t_out, to, sizeof(double) * d * M, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DPGO_HIP_OK;
}

// ----------------------------------------------------------------------- reference trajectories from a g2o file
int dpgo_g2o_read_vertices(const char* path, int d, int n, double* T_out, int* present) {
  if (!path || !T_out) return fail(DPGO_HIP_EINVAL, "read_vertices: null path or T_out");
  if (d != 2 && d != 3) return fail(DPGO_HIP_EINVAL, "read_vertices: d must be 2 or 3");
  if (n <= 0) return fail(DPGO_HIP_EINVAL, "read_vertices: need n >= 1 poses");
  std::ifstream in(path);
  if (!in) return fail(DPGO_HIP_EINVAL, std::string("cannot open ") + path);
  const size_t pw = static_cast<size_t>(d) * (d + 1);
  std::vector<double> Tv(pw * n, std::numeric_limits<double>::quiet_NaN());
  std::vector<int> pres(n, 0);
  std::string line, tok;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    if (!(ss >> tok)) continue;
    const bool se2 = tok == "VERTEX_SE2", se3 = tok == "VERTEX_SE3:QUAT";
    if (!se2 && !se3) continue;
    unsigned long long key;
    double v[7];
    bool ok = static_cast<bool>(ss >> key);
    for (int i = 0; i < (se2 ? 3 : 7); ++i) ok = ok && static_cast<bool>(ss >> v[i]);
    if (!ok) continue;  // a truncated line is skipped, as the edge reader skips one
    if ((se2 ? 2 : 3) != d) return fail(DPGO_HIP_EINVAL, "read_vertices: a vertex of the other dimension");
    const unsigned long long id = key & ((1ULL << 48) - 1);
    if (id >= static_cast<unsigned long long>(n)) return fail(DPGO_HIP_EINVAL, "read_vertices: vertex id >= n");
    double* P = &Tv[pw * id];
    if (se2) {
      const double c = std::cos(v[2]), s = std::sin(v[2]);
      P[0] = c;
      P[1] = s;
      P[2] = -s;
      P[3] = c;
      P[4] = v[0];
      P[5] = v[1];
    } else {
      const double nrm = std::sqrt(v[3] * v[3] + v[4] * v[4] + v[5] * v[5] + v[6] * v[6]);
      if (!(nrm > 0.0) || !std::isfinite(nrm)) return fail(DPGO_HIP_EINVAL, "read_vertices: a zero quaternion");
      const double x = v[3] / nrm, y = v[4] / nrm, z = v[5] / nrm, w = v[6] / nrm;
      const double Rm[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                               {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                               {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
      for (int c = 0; c < 3; ++c)
        for (int a = 0; a < 3; ++a) P[3 * c + a] = Rm[a][c];
      for (int a = 0; a < 3; ++a) P[9 + a] = v[a];
    }
    pres[id] = 1;
  }
  std::memcpy(T_out, Tv.data(), sizeof(double) * pw * n);
  if (present) std::memcpy(present, pres.data(), sizeof(int) * n);
  return DPGO_HIP_OK;
}

// ----------------------------------------------------------------------- a solution against the truth
int dpgo_graph_evaluate(dpgo_graph g, int r, const double* X, const double* T_truth, const int* use, int align,
                        int pose, dpgo_eval_info* info, double* tra_sq, double* rot_sq, double* rpe_rot_sq,
                        double* rpe_tra_sq) {
  if (!g || !X || !T_truth || !info) return fail(DPGO_HIP_EINVAL, "evaluate: null graph, X, T_truth or info");
  const int d = g->d, n = g->n;
  if ((d != 2 && d != 3) || n <= 0) return fail(DPGO_HIP_EINVAL, "evaluate: empty graph");
  if (r < d || !supported_rb(r, d + 1)) return fail(DPGO_HIP_EINVAL, "evaluate: unsupported (r, d)");
  if (align != DPGO_ALIGN_NONE && align != DPGO_ALIGN_POSE && align != DPGO_ALIGN_LSQ)
    return fail(DPGO_HIP_EINVAL, "evaluate: unknown align");
  if (pose < 0 || pose >= n) return fail(DPGO_HIP_EINVAL, "evaluate: pose outside [0, n)");
  if (align == DPGO_ALIGN_POSE && use && use[pose] == 0)
    return fail(DPGO_HIP_EINVAL, "evaluate: DPGO_ALIGN_POSE on an unused pose");
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  const size_t N = static_cast<size_t>(n), b = static_cast<size_t>(d) + 1, pw = d * b, dd = static_cast<size_t>(d) * d;
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  // the edges whose endpoints are both used, in the graph's order: the others would carry weight 0, and leaving
  // them out of the launch keeps a truth that is NaN at its unused poses out of the sums
  std::vector<int> eid, q1, q2;
  for (size_t e = 0; e < g->p1.size(); ++e) {
    const int i = g->p1[e], j = g->p2[e];
    if (i == j || (use && (use[i] == 0 || use[j] == 0))) continue;
    eid.push_back(static_cast<int>(e));
    q1.push_back(i);
    q2.push_back(j);
  }
  const size_t mu = eid.size(), P = DPGO_TRAJ_MOMENTS(d);
  const size_t w_mom = static_cast<size_t>(dpgo_hip_traj_moments_work_doubles(d, n));
  const size_t w_err = static_cast<size_t>(dpgo_hip_traj_errors_work_doubles(d, n));
  const size_t w_edge = static_cast<size_t>(dpgo_hip_edge_errors_work_doubles(static_cast<long long>(mu)));
  hipStream_t s = nullptr;
  DevBuf<double> xb, eb;
  DevTraj D;
  HIP_TRY(D.buf.ensure(2 * pw * N + 2 * N + DPGO_TRAJ_SUMS + P + std::max(w_mom, w_err)));
  D.That = D.buf.p;
  D.T = D.That + pw * N;
  double* o_tra = D.T + pw * N;
  double* o_rot = o_tra + N;
  double* o_sums = o_rot + N;
  double* o_mom = o_sums + DPGO_TRAJ_SUMS;
  double* o_work = o_mom + P;
  if (use) {
    HIP_TRY(D.mask.ensure(N));
    HIP_TRY(hipMemcpyAsync(D.mask.p, use, sizeof(int) * N, hipMemcpyHostToDevice, s));
    D.use = D.mask.p;
  }
  HIP_TRY(hipMemcpyAsync(D.T, T_truth, sizeof(double) * pw * N, hipMemcpyHostToDevice, s));
  if (r > d) {
    HIP_TRY(xb.ensure(r * b * N));
    HIP_TRY(hipMemcpyAsync(xb.p, X, sizeof(double) * r * b * N, hipMemcpyHostToDevice, s));
    DPGO_TRY(dpgo_hip_round_se_dev(r, d, n, xb.p, xb.p + static_cast<size_t>(pose) * r * b, D.That, s));
  } else {
    HIP_TRY(hipMemcpyAsync(D.That, X, sizeof(double) * pw * N, hipMemcpyHostToDevice, s));
  }
  dpgo_eval_info I{};
  for (double& v : I.Aa) v = 0.0;
  for (int i = 0; i < d; ++i) I.Aa[i * d + i] = 1.0;
  for (double& v : I.sigma) v = qnan;
  I.rank = -1;
  if (align == DPGO_ALIGN_POSE) {
    double Ph[12];
    HIP_TRY(hipMemcpyAsync(Ph, D.That + static_cast<size_t>(pose) * pw, sizeof(double) * pw, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const double* Pt = T_truth + static_cast<size_t>(pose) * pw;
    for (int k = 0; k < d; ++k)
      for (int i = 0; i < d; ++i) {  // A = R_p Rhat_p^T
        double v = 0;
        for (int c = 0; c < d; ++c) v += Pt[c * d + i] * Ph[c * d + k];
        I.Aa[k * d + i] = v;
      }
    for (int i = 0; i < d; ++i) {
      double v = 0;
      for (int k = 0; k < d; ++k) v += I.Aa[k * d + i] * Ph[dd + k];
      I.Aa[dd + i] = Pt[dd + i] - v;
    }
  } else if (align == DPGO_ALIGN_LSQ) {
    dpgo_align_info A{};
    DPGO_TRY(align_dev(d, n, D.That, D.T, D.use, o_mom, o_work, s, I.Aa, &A));
    for (int i = 0; i < 3; ++i) I.sigma[i] = A.sigma[i];
    I.rank = A.rank;
  }
  DPGO_TRY(dpgo_hip_traj_errors_dev(d, n, D.That, D.T, D.use, I.Aa, o_tra, o_rot, o_sums, o_work, s));
  double sums[DPGO_TRAJ_SUMS], cost[2] = {0.0, 0.0};
  HIP_TRY(hipMemcpyAsync(sums, o_sums, sizeof(sums), hipMemcpyDeviceToHost, s));
  DevBuf<int> ib;
  double *e_rot = nullptr, *e_tra = nullptr;
  if (mu > 0) {
    // R, t, ones, zeros, rot_sq, tra_sq, the two costs, the partials
    HIP_TRY(eb.ensure((dd + d) * mu + 4 * mu + 2 + w_edge));
    HIP_TRY(ib.ensure(2 * mu));
    double* e_R = eb.p;
    double* e_t = e_R + dd * mu;
    double* e_one = e_t + d * mu;
    double* e_zero = e_one + mu;
    e_rot = e_zero + mu;
    e_tra = e_rot + mu;
    double* e_cost = e_tra + mu;
    double* e_work = e_cost + 2;
    const std::vector<double> ones(mu, 1.0);
    HIP_TRY(hipMemcpyAsync(ib.p, q1.data(), sizeof(int) * mu, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ib.p + mu, q2.data(), sizeof(int) * mu, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e_one, ones.data(), sizeof(double) * mu, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(e_zero, 0, sizeof(double) * mu, s));
    DPGO_TRY(dpgo_hip_relative_poses_dev(d, n, D.T, static_cast<long long>(mu), ib.p, ib.p + mu, e_R, e_t, s));
    const dpgo_edges Lr{static_cast<long long>(mu), ib.p, ib.p + mu, e_R, e_t, e_one, e_zero, nullptr};
    const dpgo_edges Lt{static_cast<long long>(mu), ib.p, ib.p + mu, e_R, e_t, e_zero, e_one, nullptr};
    DPGO_TRY(dpgo_hip_edge_errors_dev(d, d, n, &Lr, D.That, nullptr, e_rot, e_tra, e_cost, e_work, s));
    DPGO_TRY(dpgo_hip_edge_errors_dev(d, d, n, &Lt, D.That, nullptr, nullptr, nullptr, e_cost + 1, e_work, s));
    HIP_TRY(hipMemcpyAsync(cost, e_cost, sizeof(cost), hipMemcpyDeviceToHost, s));
  }
  std::vector<double> er, et;
  if (mu > 0 && (rpe_rot_sq || rpe_tra_sq)) {
    er.resize(mu);
    et.resize(mu);
    HIP_TRY(hipMemcpyAsync(er.data(), e_rot, sizeof(double) * mu, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(et.data(), e_tra, sizeof(double) * mu, hipMemcpyDeviceToHost, s));
  }
  if (tra_sq) HIP_TRY(hipMemcpyAsync(tra_sq, o_tra, sizeof(double) * N, hipMemcpyDeviceToHost, s));
  if (rot_sq) HIP_TRY(hipMemcpyAsync(rot_sq, o_rot, sizeof(double) * N, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (size_t e = 0; e < g->p1.size(); ++e) {  // an edge left out has no residual
    if (rpe_rot_sq) rpe_rot_sq[e] = qnan;
    if (rpe_tra_sq) rpe_tra_sq[e] = qnan;
  }
  for (size_t k = 0; k < er.size(); ++k) {
    if (rpe_rot_sq) rpe_rot_sq[eid[k]] = er[k];
    if (rpe_tra_sq) rpe_tra_sq[eid[k]] = et[k];
  }
  I.count = sums[0];
  I.ate_rmse = std::sqrt(sums[1] / sums[0]);
  I.rot_rmse = std::sqrt(sums[2] / sums[0]);
  I.ate_max = std::sqrt(sums[3]);
  I.rot_max = std::sqrt(sums[4]);
  I.edges_used = static_cast<double>(mu);
  I.rpe_rot_rmse = mu > 0 ? std::sqrt(2.0 * cost[0] / static_cast<double>(mu)) : qnan;
  I.rpe_tra_rmse = mu > 0 ? std::sqrt(2.0 * cost[1] / static_cast<double>(mu)) : qnan;
  *info = I;
  return DPGO_HIP_OK;
}

}  // extern "C"

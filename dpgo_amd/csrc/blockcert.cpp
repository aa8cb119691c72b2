// Block certificate: lambda_min(S(X)) by LOBPCG on the r rows of the lifted r x (d+1) n layout.
// MODE_CERT applies S to every row of that layout in one launch (V -> V S acts row by row), so the r rows are r
// start vectors for the price of one: the iterate X_b, its image S X_b, the search block W (the residuals) and the
// direction block P are r-row blocks, six in all, and the memory does not grow with the iteration count.  The block
// kernels (kernels.hip, k_blk_*) keep every coefficient and Gram matrix on the device; the host solves the small
// (at most 3r x 3r) Rayleigh-Ritz problems and waits once per iteration, for the Gram matrices and the residual
// norms together.  tests/_lobpcg.py restates this file in numpy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "cert_host.h"
#include "host_eig.h"
#include "problem_internal.h"

namespace dpgo {
namespace {

constexpr double kDropGram = 1e-14;  // directions at or below this share of the largest Gram eigenvalue are dropped
constexpr double kDropP = 1e-10;     // lambda_min(B) < kDropP lambda_max(B): the iteration runs without P

// ascending eigenvalues w and eigenvectors (vector c at Z[c * m ..]) of the symmetric part of A (m x m row-major)
void eig_sym(int m, const std::vector<double>& A, std::vector<double>& Z, std::vector<double>& w) {
  std::vector<double> As(static_cast<size_t>(m) * m);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) As[static_cast<size_t>(i) * m + j] = 0.5 * (A[static_cast<size_t>(i) * m + j] + A[static_cast<size_t>(j) * m + i]);
  sym_eig(m, As, w, Z);
}

// T (m x mk row-major) with T^T G T = I on the directions of the Gram matrix G above kDropGram of the largest
void orthonormal_coeffs(int m, const std::vector<double>& G, std::vector<double>& T, int& mk) {
  std::vector<double> Z, w;
  eig_sym(m, G, Z, w);
  std::vector<int> keep;
  for (int c = 0; c < m; ++c)
    if (w[c] > kDropGram * std::max(w[m - 1], 0.0)) keep.push_back(c);
  mk = static_cast<int>(keep.size());
  T.assign(static_cast<size_t>(m) * std::max(mk, 1), 0.0);
  for (int k = 0; k < mk; ++k)
    for (int i = 0; i < m; ++i) T[static_cast<size_t>(i) * mk + k] = Z[static_cast<size_t>(keep[k]) * m + i] / std::sqrt(w[keep[k]]);
}

// Rayleigh-Ritz of the pencil (A, B), m x m row-major, by whitening B: ascending theta (mk values) and the
// coefficient matrix C (m x mk row-major, column k the k-th Ritz vector); bmin / bmax: B's extreme eigenvalues
struct Ritz {
  int mk = 0;
  double bmin = 0.0, bmax = 0.0;
  std::vector<double> theta, C;
};
void ritz(int m, const std::vector<double>& A, const std::vector<double>& B, Ritz& o) {
  std::vector<double> Z, w, T;
  eig_sym(m, B, Z, w);
  o.bmin = w[0];
  o.bmax = w[m - 1];
  std::vector<int> keep;
  for (int c = 0; c < m; ++c)
    if (w[c] > kDropGram * w[m - 1]) keep.push_back(c);
  const int mk = o.mk = static_cast<int>(keep.size());
  o.theta.clear();
  o.C.clear();
  if (mk == 0) return;
  T.assign(static_cast<size_t>(m) * mk, 0.0);
  for (int k = 0; k < mk; ++k)
    for (int i = 0; i < m; ++i) T[static_cast<size_t>(i) * mk + k] = Z[static_cast<size_t>(keep[k]) * m + i] / std::sqrt(w[keep[k]]);
  // At = T^T sym(A) T
  std::vector<double> AT(static_cast<size_t>(m) * mk, 0.0), At(static_cast<size_t>(mk) * mk, 0.0);
  for (int i = 0; i < m; ++i)
    for (int k = 0; k < mk; ++k) {
      double acc = 0.0;
      for (int j = 0; j < m; ++j)
        acc += 0.5 * (A[static_cast<size_t>(i) * m + j] + A[static_cast<size_t>(j) * m + i]) * T[static_cast<size_t>(j) * mk + k];
      AT[static_cast<size_t>(i) * mk + k] = acc;
    }
  for (int a = 0; a < mk; ++a)
    for (int k = 0; k < mk; ++k) {
      double acc = 0.0;
      for (int i = 0; i < m; ++i) acc += T[static_cast<size_t>(i) * mk + a] * AT[static_cast<size_t>(i) * mk + k];
      At[static_cast<size_t>(a) * mk + k] = acc;
    }
  std::vector<double> Y;
  eig_sym(mk, At, Y, o.theta);
  o.C.assign(static_cast<size_t>(m) * mk, 0.0);
  for (int i = 0; i < m; ++i)
    for (int k = 0; k < mk; ++k) {
      double acc = 0.0;
      for (int q = 0; q < mk; ++q) acc += T[static_cast<size_t>(i) * mk + q] * Y[static_cast<size_t>(k) * mk + q];
      o.C[static_cast<size_t>(i) * mk + k] = acc;
    }
}

}  // namespace
}  // namespace dpgo

using namespace dpgo;

extern "C" {

void dpgo_default_block_cert_params(dpgo_block_cert_params* p) {
  if (!p) return;
  p->max_iters = 2000;
  p->tol = 1e-8;
  p->flags = DPGO_CERT_SEED_X;
  p->precon = 0;
  p->refresh = 50;
}

int dpgo_hip_certify_block(dpgo_hip_problem h, const double* X, const dpgo_block_cert_params* params,
                           double* lambda_min, double* eigvec, dpgo_cert_info* info) {
  DPGO_TRY(check_handle(h));
  dpgo_block_cert_params P;
  dpgo_default_block_cert_params(&P);
  if (params) P = *params;
  if (h->K != 1) return fail(DPGO_HIP_EINVAL, "certification needs a single-agent handle");
  if (!X || !lambda_min || P.max_iters < 1 || !std::isfinite(P.tol) || (P.precon != 0 && P.precon != 1) ||
      (P.flags & ~DPGO_CERT_SEED_X) != 0 || P.refresh < 0)
    return fail(DPGO_HIP_EINVAL, "bad block certification arguments");
  const int r = h->r, b = h->b, ru = r + 1;
  const long nc = static_cast<long>(h->N) * b, L = nc * r;
  // the locked block U first (host only), so the size refusal comes before any device work
  std::vector<double> Uh;
  const int nl = (P.flags & DPGO_CERT_SEED_X) ? seed_block(r, b, nc, X, SeedLayout::Interleaved, Uh) : 0;
  if (3L * r > nc - nl)
    return fail(DPGO_HIP_EINVAL, "block certification: three blocks of r rows exceed the free dimension (d+1) n - seeds");
  DPGO_TRY(problem_ready(h));
  DPGO_TRY(ensure_work_public(h));
  hipStream_t st = h->stream;

  // device state: six r-row blocks, U, and the small arrays (Gram output | two sets of row norms; coefficients)
  const int GO = 3 * r * (6 * r + 1);
  DevBuf<double> blocks, U, part, scal, small;
  HIP_TRY(blocks.ensure(static_cast<size_t>(6) * L));
  HIP_TRY(part.ensure(static_cast<size_t>(blk_partial_doubles(r))));
  HIP_TRY(scal.ensure(static_cast<size_t>(GO) + 2 * r));
  HIP_TRY(small.ensure(static_cast<size_t>(r) + r * r + 2 * 3 * r * r + r * ru));
  double *Xb = blocks.p, *SX = Xb + L, *W = SX + L, *SW = W + L, *Pb = SW + L, *SP = Pb + L;
  double *norms = scal.p + GO, *norms2 = norms + r;
  double *theta_d = small.p, *T_d = theta_d + r, *cx_d = T_d + r * r, *cp_d = cx_d + 3 * r * r, *cu_d = cp_d + 3 * r * r;
  if (nl > 0) {
    HIP_TRY(U.ensure(Uh.size()));
    HIP_TRY(hipMemcpyAsync(U.p, Uh.data(), sizeof(double) * Uh.size(), hipMemcpyHostToDevice, st));
  }
  // Lambda(X) into h->S (the S the Riemannian Hessian uses); X itself travels through the W block
  HIP_TRY(hipMemcpyAsync(W, X, sizeof(double) * L, hipMemcpyHostToDevice, st));
  DPGO_TRY(eval_at(h, W, h->tA.p, h->S.p, h->pa.p, FLAG_NONE));
  {  // the start block: the Lanczos certificate's stream in the lifted layout's memory order
    const std::vector<double> q0 = cert_start(CertStart::Lifted, L, r);
    HIP_TRY(hipMemcpyAsync(Xb, q0.data(), sizeof(double) * L, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // q0 and Uh are read
  }

  // host staging of everything uploaded in the loop: each is written at most once between two waits
  std::vector<double> hs(static_cast<size_t>(GO) + 2 * r), h_theta(r), h_T(static_cast<size_t>(r) * r),
      h_cx(static_cast<size_t>(3) * r * r), h_cp(static_cast<size_t>(3) * r * r), h_cu(static_cast<size_t>(r) * ru);
  int passes = 0, restarts = 0;
  double scale = 0.0;
  std::vector<double> theta(r, 0.0);

  auto gram = [&](std::initializer_list<std::pair<const double*, int>> bl, int nleft) -> int {
    BlkList Lb{};
    for (const auto& e : bl) {
      Lb.p[Lb.n] = e.first;
      Lb.ld[Lb.n] = e.second;
      ++Lb.n;
    }
    HIP_TRY(launch_blk_gram(r, nc, Lb, nleft, part.p, scal.p, st));
    return DPGO_HIP_OK;
  };
  auto fetch = [&](size_t off, size_t count) -> int {  // the wait: scal[off .. off + count) into hs (same offsets)
    HIP_TRY(hipMemcpyAsync(hs.data() + off, scal.p + off, sizeof(double) * count, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (size_t i = off; i < off + count; ++i)
      if (!std::isfinite(hs[i])) return fail(DPGO_HIP_EDEVICE, "block certification: a reduction is not finite");
    return DPGO_HIP_OK;
  };
  auto put = [&](double* dst, const std::vector<double>& src) -> int {
    HIP_TRY(hipMemcpyAsync(dst, src.data(), sizeof(double) * src.size(), hipMemcpyHostToDevice, st));
    return DPGO_HIP_OK;
  };
  auto apply = [&](const double* in, double* out) -> int {  // out = in S, all r rows: one operator pass
    const SpmmArgs sa{in, nullptr, nullptr, nullptr, h->S.p, out, nullptr, nullptr, nullptr, PRECON_NONE};
    DPGO_TRY(spmm_launch(h, MODE_CERT, make_ctx(h, FLAG_NONE, nullptr), sa));
    ++passes;
    return DPGO_HIP_OK;
  };
  // V <- V - (V U^T) U; nrm: where the result's |V_i|^2 go (null: nowhere)
  auto project_u = [&](double* V, double* nrm) -> int {
    if (nl == 0) return DPGO_HIP_OK;
    DPGO_TRY(gram({{V, r}, {U.p, ru}}, 1));
    HIP_TRY(launch_blk_project(r, ru, nc, V, U.p, scal.p + r, 2 * r + 1, nrm ? part.p : nullptr, nrm, st));
    return DPGO_HIP_OK;
  };
  // V's rows orthonormalised through their Gram matrix on the device (dropped rows become zero rows at the end)
  auto orthonormalise = [&](double* V) -> int {
    DPGO_TRY(gram({{V, r}}, 1));
    HIP_TRY(launch_blk_orthcoef(r, scal.p, r, kDropGram, T_d, st));
    HIP_TRY(launch_blk_transform(r, nc, V, T_d, st));
    return DPGO_HIP_OK;
  };
  auto track_scale = [&](const std::vector<double>& th) {
    for (double t : th) scale = std::max(scale, std::fabs(t));
  };
  // X_b projected off U and orthonormalised, S X_b by a real operator pass, Rayleigh-Ritz of X_b alone (a wait)
  auto alone = [&]() -> int {
    DPGO_TRY(project_u(Xb, nullptr));
    DPGO_TRY(orthonormalise(Xb));
    DPGO_TRY(apply(Xb, SX));
    DPGO_TRY(gram({{Xb, r}, {SX, r}}, 1));
    DPGO_TRY(fetch(0, static_cast<size_t>(r) * 2 * r));
    std::vector<double> A(static_cast<size_t>(r) * r), B(static_cast<size_t>(r) * r);
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < r; ++j) {
        B[static_cast<size_t>(i) * r + j] = hs[static_cast<size_t>(i) * 2 * r + j];
        A[static_cast<size_t>(i) * r + j] = hs[static_cast<size_t>(i) * 2 * r + r + j];
      }
    for (int i = 0; i < r; ++i)
      if (!(B[static_cast<size_t>(i) * r + i] > 0.0))
        return fail(DPGO_HIP_EDEVICE, "block certification: the iterate lost a row");
    Ritz rz;
    ritz(r, A, B, rz);
    if (rz.mk != r) return fail(DPGO_HIP_EDEVICE, "block certification: the iterate lost a row");
    track_scale(rz.theta);
    theta = rz.theta;
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < r; ++j) h_T[static_cast<size_t>(i) * r + j] = rz.C[static_cast<size_t>(j) * r + i];
    DPGO_TRY(put(T_d, h_T));
    HIP_TRY(launch_blk_transform(r, nc, Xb, T_d, st));
    HIP_TRY(launch_blk_transform(r, nc, SX, T_d, st));
    return DPGO_HIP_OK;
  };

  DPGO_TRY(alone());
  int np = 0, iterations = 0;
  while (iterations < P.max_iters) {
    // the residual block, its norms (off U), the search block W: everything up to the Gram matrices is queued
    // without a wait, so the stopping test of this iterate is read together with them
    h_theta = theta;
    DPGO_TRY(put(theta_d, h_theta));
    HIP_TRY(launch_blk_residual(r, nc, SX, Xb, theta_d, W, part.p, norms, st));
    DPGO_TRY(project_u(W, norms));
    if (P.precon == 1) {
      HIP_TRY(launch_blk_precond(r, b, h->N, W, h->minv.p, st));
      DPGO_TRY(project_u(W, nullptr));
    }
    DPGO_TRY(gram({{W, r}, {Xb, r}}, 1));
    HIP_TRY(launch_blk_project(r, r, nc, W, Xb, scal.p + r, 2 * r, nullptr, nullptr, st));
    DPGO_TRY(orthonormalise(W));
    // the second orthogonalisation runs after the rows were scaled up, against U too: a small row's rounding-level
    // components along U and X_b grow with it, and S has lower eigenvalues on U than on its complement
    if (nl > 0) {
      DPGO_TRY(gram({{W, r}, {Xb, r}, {U.p, ru}}, 1));
      HIP_TRY(launch_blk_project(r, ru, nc, W, U.p, scal.p + 2 * r, 3 * r + 1, nullptr, nullptr, st));
      HIP_TRY(launch_blk_project(r, r, nc, W, Xb, scal.p + r, 3 * r + 1, nullptr, nullptr, st));
    } else {
      DPGO_TRY(gram({{W, r}, {Xb, r}}, 1));
      HIP_TRY(launch_blk_project(r, r, nc, W, Xb, scal.p + r, 2 * r, nullptr, nullptr, st));
    }
    DPGO_TRY(apply(W, SW));
    const int nb = np > 0 ? 3 : 2, ld = 2 * nb * r;  // blocks of Z, row length of [B | A]
    if (np > 0)
      DPGO_TRY(gram({{Xb, r}, {W, r}, {Pb, r}, {SX, r}, {SW, r}, {SP, r}}, 3));
    else
      DPGO_TRY(gram({{Xb, r}, {W, r}, {SX, r}, {SW, r}}, 2));
    HIP_TRY(hipMemcpyAsync(hs.data() + GO, norms, sizeof(double) * r, hipMemcpyDeviceToHost, st));
    DPGO_TRY(fetch(0, static_cast<size_t>(nb) * r * ld));  // the iteration's one wait
    if (!std::isfinite(hs[GO])) return fail(DPGO_HIP_EDEVICE, "block certification: a residual norm is not finite");
    if (std::sqrt(std::max(hs[GO], 0.0)) <= P.tol * scale) break;  // converged before this W: it is discarded
    ++iterations;
    // live rows: all of X_b, W's leading non-zero rows, P's first np
    std::vector<int> idx;
    for (int i = 0; i < r; ++i) idx.push_back(i);
    int nw = 0;
    for (int i = 0; i < r; ++i)
      if (hs[static_cast<size_t>(r + i) * ld + r + i] > 0.0) {
        idx.push_back(r + i);
        ++nw;
      }
    if (nw == 0) break;  // an invariant subspace up to rounding
    for (int i = 0; i < np; ++i) idx.push_back(2 * r + i);
    auto sub = [&](int m, std::vector<double>& A, std::vector<double>& B) {
      A.assign(static_cast<size_t>(m) * m, 0.0);
      B.assign(static_cast<size_t>(m) * m, 0.0);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
          B[static_cast<size_t>(i) * m + j] = hs[static_cast<size_t>(idx[i]) * ld + idx[j]];
          A[static_cast<size_t>(i) * m + j] = hs[static_cast<size_t>(idx[i]) * ld + nb * r + idx[j]];
        }
    };
    int m = r + nw + np;
    std::vector<double> A, B;
    sub(m, A, B);
    Ritz rz;
    ritz(m, A, B, rz);
    if (np > 0 && rz.bmin < kDropP * rz.bmax) {  // [X_b; W; P] has lost its conditioning: this iteration without P
      ++restarts;
      m = r + nw;
      sub(m, A, B);
      ritz(m, A, B, rz);
    }
    if (rz.mk < r) return fail(DPGO_HIP_EDEVICE, "block certification: the Rayleigh-Ritz basis lost its rank");
    track_scale(rz.theta);
    const int mk = rz.mk;
    theta.assign(rz.theta.begin(), rz.theta.begin() + r);
    // x' = C^T Z; p' = the W and P part of C, orthonormalised through its own Gram matrix Cp^T B Cp on the host
    std::fill(h_cx.begin(), h_cx.end(), 0.0);
    std::fill(h_cp.begin(), h_cp.end(), 0.0);
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < m; ++j) h_cx[static_cast<size_t>(i) * 3 * r + idx[j]] = rz.C[static_cast<size_t>(j) * mk + i];
    std::vector<double> Cp(static_cast<size_t>(m) * r, 0.0), BC(static_cast<size_t>(m) * r, 0.0), Gp(static_cast<size_t>(r) * r, 0.0), Tp;
    for (int j = r; j < m; ++j)
      for (int i = 0; i < r; ++i) Cp[static_cast<size_t>(j) * r + i] = rz.C[static_cast<size_t>(j) * mk + i];
    for (int a = 0; a < m; ++a)
      for (int i = 0; i < r; ++i) {
        double acc = 0.0;
        for (int j = 0; j < m; ++j) acc += 0.5 * (B[static_cast<size_t>(a) * m + j] + B[static_cast<size_t>(j) * m + a]) * Cp[static_cast<size_t>(j) * r + i];
        BC[static_cast<size_t>(a) * r + i] = acc;
      }
    for (int i = 0; i < r; ++i)
      for (int k = 0; k < r; ++k) {
        double acc = 0.0;
        for (int a = 0; a < m; ++a) acc += Cp[static_cast<size_t>(a) * r + i] * BC[static_cast<size_t>(a) * r + k];
        Gp[static_cast<size_t>(i) * r + k] = acc;
      }
    int np_new = 0;
    orthonormal_coeffs(r, Gp, Tp, np_new);
    for (int i = 0; i < np_new; ++i)
      for (int j = r; j < m; ++j) {
        double acc = 0.0;
        for (int k = 0; k < r; ++k) acc += Cp[static_cast<size_t>(j) * r + k] * Tp[static_cast<size_t>(k) * np_new + i];
        h_cp[static_cast<size_t>(i) * 3 * r + idx[j]] = acc;
      }
    DPGO_TRY(put(cx_d, h_cx));
    DPGO_TRY(put(cp_d, h_cp));
    HIP_TRY(launch_blk_combine(r, nc, BlkCombine{Xb, W, Pb, SX, SW, SP, cx_d, cp_d, np > 0 ? 1 : 0}, st));
    np = np_new;
    if (P.refresh > 0 && iterations % P.refresh == 0) DPGO_TRY(alone());  // bounds the recurrence's drift
  }

  // finish: the lowest pair's true residuals from a fresh operator pass, on S and on P S P
  DPGO_TRY(alone());
  h_theta = theta;
  DPGO_TRY(put(theta_d, h_theta));
  HIP_TRY(launch_blk_residual(r, nc, SX, Xb, theta_d, W, part.p, norms, st));
  if (nl > 0) DPGO_TRY(project_u(W, norms2));
  DPGO_TRY(fetch(GO, nl > 0 ? 2 * r : r));
  const double theta_c = theta[0];
  double res = std::sqrt(std::max(hs[GO], 0.0));
  const double res_c = nl > 0 ? std::sqrt(std::max(hs[GO + r], 0.0)) : res;
  double lam = theta_c, lam_s = NAN, coupling = 0.0;
  const double* vec_block = Xb;
  if (nl > 0) {
    // U's block A_s = U S U^T and the coupling |(I - U^T U) S U^T|_F, r rows of U per operator pass
    std::vector<double> As(static_cast<size_t>(nl) * nl, 0.0), su2(nl, 0.0), Zs, ws;
    const int go = 2 * r + 1;
    for (int j0 = 0; j0 < nl; j0 += r) {
      const int cnt = std::min(r, nl - j0);
      HIP_TRY(hipMemsetAsync(W, 0, sizeof(double) * L, st));
      for (int i = 0; i < cnt; ++i) HIP_TRY(launch_strided_copy(nc, U.p + j0 + i, ru, W + i, r, st));
      DPGO_TRY(apply(W, SW));
      DPGO_TRY(gram({{SW, r}, {U.p, ru}}, 1));
      DPGO_TRY(fetch(0, static_cast<size_t>(r) * go));
      for (int i = 0; i < cnt; ++i) {
        su2[j0 + i] = hs[static_cast<size_t>(i) * go + i];
        for (int j = 0; j < nl; ++j) As[static_cast<size_t>(j) * nl + j0 + i] = hs[static_cast<size_t>(i) * go + r + j];
      }
    }
    double c2 = 0.0;
    for (int j = 0; j < nl; ++j) {
      double cc = 0.0;
      for (int i = 0; i < nl; ++i) cc += As[static_cast<size_t>(i) * nl + j] * As[static_cast<size_t>(i) * nl + j];
      c2 += std::max(0.0, su2[j] - cc);
    }
    coupling = std::sqrt(c2);
    eig_sym(nl, As, Zs, ws);
    lam_s = ws[0];
    if (lam_s < theta_c) {  // the lowest pair lies in U: y = z_0 U on row 0, its residual by one more pass
      lam = lam_s;
      std::fill(h_cu.begin(), h_cu.end(), 0.0);
      for (int j = 0; j < nl; ++j) h_cu[j] = -Zs[j];
      DPGO_TRY(put(cu_d, h_cu));
      HIP_TRY(hipMemsetAsync(W, 0, sizeof(double) * L, st));
      HIP_TRY(launch_blk_project(r, ru, nc, W, U.p, cu_d, ru, nullptr, nullptr, st));
      DPGO_TRY(apply(W, SW));
      std::fill(h_theta.begin(), h_theta.end(), 0.0);
      h_theta[0] = lam;
      DPGO_TRY(put(theta_d, h_theta));
      HIP_TRY(launch_blk_residual(r, nc, SW, W, theta_d, Pb, part.p, norms, st));
      DPGO_TRY(fetch(GO, r));
      res = std::sqrt(std::max(hs[GO], 0.0));
      vec_block = W;
    }
  }
  std::vector<double> ev;
  if (eigvec) {
    ev.resize(L);
    HIP_TRY(hipMemcpyAsync(ev.data(), vec_block, sizeof(double) * L, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  // outputs, only now that nothing can fail
  *lambda_min = lam;
  if (info) fill_cert_info(info, passes, restarts, nl, res, lam_s, theta_c, res_c, coupling, theta);
  if (eigvec)  // the unit vector on row 0, rows 1.. zero, as dpgo_hip_escape_direction takes it
    for (long x = 0; x < nc; ++x) {
      eigvec[x * r] = ev[x * r];
      for (int i = 1; i < r; ++i) eigvec[x * r + i] = 0.0;
    }
  return DPGO_HIP_OK;
}

}  // extern "C"

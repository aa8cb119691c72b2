// Lanczos certificate: lambda_min(S(X)) by a Krylov chain on the device with the Rayleigh-Ritz problems
// on the host (host_eig.h).  Every step is kept (T tridiagonal) or, with a basis limit, the chain is thick-restarted
// from its lowest Ritz vectors (T dense).  DPGO_CERT_SEED_X locks the block U of cert_host.h's seed_block: the chain
// runs on the complement (P S P, P = I - U U^T) and U's block is resolved exactly at the end.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "cert_host.h"
#include "host_eig.h"
#include "problem_internal.h"

namespace dpgo {

int dot_multi_host(long L, const double* x, const double* B, int k, double* part, hipStream_t stream, double* out) {
  HIP_TRY(launch_dot_multi(L, x, B, k, part, stream));
  std::vector<double> hp(static_cast<size_t>(kDotBlocks) * k);
  HIP_TRY(hipMemcpyAsync(hp.data(), part, sizeof(double) * hp.size(), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  for (int j = 0; j < k; ++j) out[j] = 0.0;
  for (int g = 0; g < kDotBlocks; ++g)
    for (int j = 0; j < k; ++j) out[j] += hp[static_cast<size_t>(g) * k + j];
  return DPGO_HIP_OK;
}

void fill_cert_info(dpgo_cert_info* info, int iters, int restarts, int nl, double res, double lam_s, double theta_c,
                    double res_c, double coupling, const std::vector<double>& theta) {
  info->iters = iters;
  info->restarts = restarts;
  info->seeds = nl;
  info->residual = res;
  info->lambda_seed = lam_s;
  info->lambda_complement = theta_c;
  info->residual_complement = res_c;
  info->coupling = coupling;
  // x = (u, v) in (U, U_perp): x^T S x >= a |u|^2 - 2 beta |u||v| + c |v|^2 with a = lambda_min(A_s),
  // c = theta_C - residual_C, beta = |B|_2 <= |B|_F: the 2 x 2 form's smallest eigenvalue
  const double cl = theta_c - res_c;
  info->lower_bound = nl > 0 ? 0.5 * (lam_s + cl) - std::sqrt(0.25 * (cl - lam_s) * (cl - lam_s) + coupling * coupling) : cl;
  for (int i = 0; i < 8; ++i) info->ritz[i] = i < static_cast<int>(theta.size()) ? theta[i] : NAN;
}

namespace {

// The basis with its small device arrays, and the chain's host state.  With a seed block everything lives on row 0
// of the lifted layout: the basis is stored compact (Lc = (d + 1) n doubles per vector, r x less traffic in the
// orthogonalisation) and expanded around the operator (V -> V S acts row by row, so the search space stays on row 0
// and its spectrum is S's).
struct Lanczos {
  dpgo_hip_problem h = nullptr;
  LanczosPlan plan;
  bool seed_x = false, verbose = false;
  long L = 0, Lc = 0;
  double tol = 0.0;
  DevBuf<double> V, tmp, c, part, xin, xout;
  DevBuf<double> sy, w, y;  // S y of residual_of (X on the way in), the chain's next direction, the Ritz vector
  // the chain: T = V_c^T P S P V_c (alpha / beta while tridiagonal; dense after a restart) and its last Ritz pairs,
  // theta ascending, Z column-major m x m (tridiagonal T: the lowest vector only)
  std::vector<double> T, alpha, beta, Z, theta;
  int nl = 0, nb = 0, k = 0;  // locked vectors V_0..V_{nl-1}, basis vectors in place, the one to expand next
  int total = 0, nrestart = 0, m_final = 0;
  double bk = 0.0, res = 0.0;
  bool breakdown = false;
  double lam = 0.0, lam_s = NAN, theta_c = 0.0, res_c = 0.0, coupling = 0.0;  // resolve()'s

  int init(dpgo_hip_problem hh, bool seeded, int nseed, double tolerance) {
    h = hh;
    seed_x = seeded;
    tol = tolerance;
    verbose = std::getenv("DPGO_VERBOSE_CERT") != nullptr;
    L = static_cast<long>(h->vec_len());
    Lc = seed_x ? L / h->r : L;
    const int slots = nseed + plan.mmax + 1;
    T.assign(static_cast<size_t>(plan.mmax + 1) * (plan.mmax + 1), 0.0);
    for (auto* b : {&sy, &w, &y}) HIP_TRY(b->ensure(L));
    HIP_TRY(V.ensure(static_cast<size_t>(slots) * Lc));
    if (plan.keep > 0) HIP_TRY(tmp.ensure(static_cast<size_t>(plan.keep) * Lc));
    if (seed_x)
      for (auto* b : {&xin, &xout}) HIP_TRY(b->ensure(L));
    HIP_TRY(c.ensure(slots));
    HIP_TRY(part.ensure(static_cast<size_t>(kDotBlocks) * slots));
    return DPGO_HIP_OK;
  }
  double* vec(int j) { return V.p + static_cast<long>(j) * Lc; }
  double& Tat(int i, int j) { return T[static_cast<size_t>(i) * (plan.mmax + 1) + j]; }
  int upload(double* dst, const double* src, size_t n) {
    HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return DPGO_HIP_OK;
  }
  // <x, B_j>, j < count (a wait)
  int dots(const double* x, const double* B, int count, std::vector<double>& out) {
    out.resize(count);
    return dot_multi_host(Lc, x, B, count, part.p, h->stream, out.data());
  }
  // x -= sum_j coef_j B_j (coefficients through the device array c)
  int subtract(double* x, const double* B, int count, const std::vector<double>& coef) {
    if (count == 0) return DPGO_HIP_OK;
    DPGO_TRY(upload(c.p, coef.data(), count));
    HIP_TRY(launch_axpy_multi(Lc, x, B, count, c.p, h->stream));
    return DPGO_HIP_OK;
  }
  // classical Gram-Schmidt twice against V_0..V_{count-1}; the summed coefficients (= <x, V_j> before) in cs
  int orthogonalise(double* x, int count, std::vector<double>& cs) {
    cs.assign(count, 0.0);
    for (int pass = 0; pass < 2 && count > 0; ++pass) {
      std::vector<double> cc;
      DPGO_TRY(dots(x, V.p, count, cc));
      for (int j = 0; j < count; ++j) cs[j] += cc[j];
      DPGO_TRY(subtract(x, V.p, count, cc));
    }
    return DPGO_HIP_OK;
  }
  int apply(const double* x, double* out) {  // out = S x
    const double* xi = seed_x ? xin.p : x;
    if (seed_x) HIP_TRY(launch_strided_copy(Lc, x, 1, xin.p, h->r, h->stream));
    const SpmmArgs sa{xi, nullptr, nullptr, nullptr, h->S.p, seed_x ? xout.p : out, nullptr, nullptr, nullptr, PRECON_NONE};
    DPGO_TRY(spmm_launch(h, MODE_CERT, make_ctx(h, FLAG_NONE, nullptr), sa));
    if (seed_x) HIP_TRY(launch_strided_copy(Lc, xout.p, h->r, out, 1, h->stream));
    return DPGO_HIP_OK;
  }
  // |S x - th x| / |x| (S x into sy); project: |P (S x) - th x| for x orthogonal to the first `project` basis
  // vectors (the locked block: the chain's own operator P S P)
  int residual_of(const double* x, double th, double& out, int project) {
    DPGO_TRY(apply(x, sy.p));
    std::vector<double> pc, xx, xs, ss;
    if (project > 0) DPGO_TRY(orthogonalise(sy.p, project, pc));
    DPGO_TRY(dots(x, x, 1, xx));
    DPGO_TRY(dots(x, sy.p, 1, xs));
    DPGO_TRY(dots(sy.p, sy.p, 1, ss));
    out = std::sqrt(std::max(0.0, ss[0] - 2.0 * th * xs[0] + th * th * xx[0]) / std::max(xx[0], 1e-300));
    return DPGO_HIP_OK;
  }
  int combine(const double* B, int m, const double* z, double* out) {  // out = sum_j z_j B_j, j < m
    std::vector<double> negz(m);
    for (int j = 0; j < m; ++j) negz[j] = -z[j];
    HIP_TRY(hipMemsetAsync(out, 0, sizeof(double) * Lc, h->stream));
    return subtract(out, B, m, negz);
  }
  // chain Ritz vector i of the first m chain vectors into out
  int ritz_vector(int m, int i, double* out) { return combine(vec(nl), m, &Z[static_cast<size_t>(i) * m], out); }

  // The locked block U into the first basis slots and the chain's first vector after them: the seeded random start,
  // orthogonal to U.  X on the host, as the caller passed it.
  int seed_and_start(const double* X) {
    std::vector<double> U, cs, nn;
    if (seed_x) {
      HIP_TRY(hipMemsetAsync(xin.p, 0, sizeof(double) * L, h->stream));  // rows 1.. stay zero
      nl = seed_block(h->r, h->b, Lc, X, SeedLayout::Vectors, U);
      if (nl > 0) DPGO_TRY(upload(V.p, U.data(), static_cast<size_t>(nl) * Lc));
    }
    const std::vector<double> q0 = cert_start(seed_x ? CertStart::Row0 : CertStart::Lifted, L, h->r);
    DPGO_TRY(upload(w.p, q0.data(), Lc));
    DPGO_TRY(orthogonalise(w.p, nl, cs));
    DPGO_TRY(dots(w.p, w.p, 1, nn));  // a wait: U and q0 are read
    HIP_TRY(launch_scale(Lc, w.p, 1.0 / std::sqrt(nn[0]), vec(nl), h->stream));
    nb = nl + 1;
    k = nl;
    return DPGO_HIP_OK;
  }

  // One step: S q_k, its column of T against the chain, the next direction orthogonal to U and the chain
  int expand() {
    // w = S q_k, straight into the next basis slot when there is one: its dots against the basis then carry
    // |w|^2 too (the breakdown test is relative to |S q_k|)
    const bool slot = nb - nl <= plan.mmax;
    double* wk = slot ? vec(nb) : w.p;
    DPGO_TRY(apply(vec(k), wk));
    std::vector<double> c1, sq, cs, nn;
    DPGO_TRY(dots(wk, V.p, slot ? nb + 1 : nb, c1));
    if (slot)
      sq.assign(1, c1[nb]);
    else
      DPGO_TRY(dots(wk, wk, 1, sq));
    cs.assign(c1.begin(), c1.begin() + nb);
    DPGO_TRY(subtract(wk, V.p, nb, cs));
    // classical Gram-Schmidt with the DGKS criterion: a second pass when the first removed more than half of
    // |w|^2 (where rounding can leave components along the basis), otherwise one pass
    double kept = sq[0];
    for (int j = 0; j < nb; ++j) kept -= cs[j] * cs[j];
    if (kept < 0.5 * sq[0]) {
      std::vector<double> c2;
      DPGO_TRY(dots(wk, V.p, nb, c2));
      DPGO_TRY(subtract(wk, V.p, nb, c2));
      for (int j = 0; j < nb; ++j) cs[j] += c2[j];
    }
    const int kc = k - nl;
    for (int j = nl; j < nb; ++j) Tat(j - nl, kc) = Tat(kc, j - nl) = cs[j];
    ++total;
    DPGO_TRY(dots(wk, wk, 1, nn));
    bk = std::sqrt(nn[0]);
    if (!plan.dense) {
      alpha.push_back(cs[k]);
      beta.push_back(bk);
    }
    // an invariant subspace up to rounding (CGS2 leaves ~eps |S q_k| sqrt(k)): the Ritz values are exact
    breakdown = bk <= 1e-10 * std::sqrt(sq[0]);
    if (slot && !breakdown) {
      HIP_TRY(launch_scale(Lc, wk, 1.0 / bk, vec(nb), h->stream));
      Tat(nb - nl, kc) = Tat(kc, nb - nl) = bk;
      ++nb;
    }
    ++k;
    return DPGO_HIP_OK;
  }

  // Rayleigh-Ritz on the first m chain vectors and the lowest pair's residual: the chain's estimate |beta z_last|
  // (Lanczos); after a restart the true one.  *stop: converged, broken down or out of steps.
  int ritz_check(int m, bool full, bool last, bool* stop) {
    if (!plan.dense) {  // eigenvalues, and the lowest one's vector by inverse iteration: O(m^2) at any basis size
      const std::vector<double> am(alpha.begin(), alpha.begin() + m), em(beta.begin(), beta.begin() + m);
      tridiag_eig(am, em, theta, nullptr);
      const double sc = std::max(std::fabs(theta.front()), std::fabs(theta.back()));
      Z = tridiag_lowest_vector(am, em, theta[0], m > 1 ? theta[1] : theta[0], sc);
      res = std::fabs(bk * Z[static_cast<size_t>(m) - 1]);
    } else {
      std::vector<double> A(static_cast<size_t>(m) * m);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) A[static_cast<size_t>(i) * m + j] = Tat(i, j);
      sym_eig(m, A, theta, Z);
      DPGO_TRY(ritz_vector(m, 0, y.p));
      DPGO_TRY(residual_of(y.p, theta[0], res, nl));
    }
    m_final = m;
    if (verbose && (total % 500 < (plan.dense ? 500 : 5) || full || last))
      std::fprintf(stderr, "certify: %d steps, %d restarts, basis %d, theta0 %.6e, residual %.3e\n", total, nrestart,
                   m, theta[0], res);
    const double scale = std::max(std::fabs(theta.back()), std::fabs(theta[0]));
    *stop = res <= tol * std::max(scale, 1e-300) || breakdown || last;
    return DPGO_HIP_OK;
  }

  // Thick restart: the lowest `keep` Ritz vectors and the chain's newest direction (orthogonal to them)
  int thick_restart(int m) {
    const int keep = plan.keep;
    for (int i = 0; i < keep; ++i) DPGO_TRY(ritz_vector(m, i, tmp.p + static_cast<long>(i) * Lc));
    HIP_TRY(hipMemcpyAsync(vec(nl + keep), vec(nb - 1), sizeof(double) * Lc, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(vec(nl), tmp.p, sizeof(double) * keep * Lc, hipMemcpyDeviceToDevice, h->stream));
    std::fill(T.begin(), T.end(), 0.0);
    for (int i = 0; i < keep; ++i) Tat(i, i) = theta[i];
    nb = nl + keep + 1;
    k = nl + keep;
    ++nrestart;
    return DPGO_HIP_OK;
  }

  // The chain's lowest Ritz pair with its true residuals on P S P and on S (the vector in y), then the locked block:
  // A_s = U^T S U and the coupling |(I - U U^T) S U|_F (S = [A_s B^T; B C] in (U, U_perp); lambda_min(S) is bounded
  // below by the 2 x 2 form of the info's lower_bound), and the pair of A_s when it is the lower one
  int resolve() {
    DPGO_TRY(ritz_vector(m_final, 0, y.p));
    DPGO_TRY(residual_of(y.p, theta[0], res, nl));
    lam = theta_c = theta[0];
    res_c = res;
    if (nl == 0) return DPGO_HIP_OK;
    DPGO_TRY(residual_of(y.p, theta_c, res, 0));
    std::vector<double> As(static_cast<size_t>(nl) * nl), col, s2, ws, Zs;
    double c2 = 0.0;
    for (int j = 0; j < nl; ++j) {
      DPGO_TRY(apply(vec(j), sy.p));
      DPGO_TRY(dots(sy.p, V.p, nl, col));
      DPGO_TRY(dots(sy.p, sy.p, 1, s2));
      double cc = 0.0;
      for (int i = 0; i < nl; ++i) {
        As[static_cast<size_t>(i) * nl + j] = col[i];
        cc += col[i] * col[i];
      }
      c2 += std::max(0.0, s2[0] - cc);
    }
    for (int i = 0; i < nl; ++i)
      for (int j = 0; j < i; ++j) {
        const double v = 0.5 * (As[static_cast<size_t>(i) * nl + j] + As[static_cast<size_t>(j) * nl + i]);
        As[static_cast<size_t>(i) * nl + j] = As[static_cast<size_t>(j) * nl + i] = v;
      }
    sym_eig(nl, As, ws, Zs);
    lam_s = ws[0];
    coupling = std::sqrt(c2);
    if (lam_s < theta_c) {  // the lowest Ritz pair lies in U
      lam = lam_s;
      DPGO_TRY(combine(V.p, nl, Zs.data(), y.p));
      DPGO_TRY(residual_of(y.p, lam, res, 0));
    }
    return DPGO_HIP_OK;
  }
};

}  // namespace
}  // namespace dpgo

using namespace dpgo;

extern "C" {

int dpgo_hip_certify(dpgo_hip_problem h, const double* X, int max_iters, double tol, double* lambda_min,
                     double* residual, int* iters, double* eigvec) {
  dpgo_cert_info info;
  DPGO_TRY(dpgo_hip_certify_ex(h, X, max_iters, 0, 0, tol, lambda_min, eigvec, &info));
  if (residual) *residual = info.residual;
  if (iters) *iters = info.iters;
  return DPGO_HIP_OK;
}

int dpgo_hip_certify_ex(dpgo_hip_problem h, const double* X, int max_iters, int basis_max, int flags, double tol,
                        double* lambda_min, double* eigvec, dpgo_cert_info* info) {
  DPGO_TRY(problem_ready(h));
  if (h->K != 1) return fail(DPGO_HIP_EINVAL, "certification needs a single-agent handle");
  if (!X || !lambda_min || max_iters < 2 || basis_max < 0 || (basis_max > 0 && basis_max < 8))
    return fail(DPGO_HIP_EINVAL, "bad certification arguments");
  DPGO_TRY(ensure_work_public(h));
  const long L = static_cast<long>(h->vec_len());
  const int r = h->r;
  const bool seed_x = (flags & DPGO_CERT_SEED_X) != 0;
  const int nseed = seed_x ? r + 1 : 0;
  Lanczos A;
  A.plan = lanczos_plan(max_iters, basis_max, seed_x ? L / r : L, nseed);
  if (!A.plan.ok) return fail(DPGO_HIP_EINVAL, "certification basis too small");
  DPGO_TRY(A.init(h, seed_x, nseed, tol));
  DPGO_TRY(A.upload(A.sy.p, X, L));
  // Lambda(X): S_j = sym(Y_j^T (XQ + G)_Y) (the same S the Riemannian Hessian uses)
  DPGO_TRY(eval_at(h, A.sy.p, h->tA.p, h->S.p, h->pa.p, FLAG_NONE));
  DPGO_TRY(A.seed_and_start(X));
  for (bool stop = false; !stop;) {
    DPGO_TRY(A.expand());
    const int m = A.k - A.nl;
    const bool full = A.nb - A.nl > A.plan.mmax || A.breakdown;
    const bool last = A.total >= max_iters;
    if (!(ritz_check_due(A.plan.dense, m) || full || last)) continue;
    DPGO_TRY(A.ritz_check(m, full, last, &stop));
    if (stop || !full) continue;
    if (!A.plan.dense) break;
    DPGO_TRY(A.thick_restart(m));
  }
  DPGO_TRY(A.resolve());
  *lambda_min = A.lam;
  if (info)
    fill_cert_info(info, A.total, A.nrestart, A.nl, A.res, A.lam_s, A.theta_c, A.res_c, A.coupling, A.theta);
  if (eigvec) {
    std::vector<double> yc(A.Lc);
    HIP_TRY(hipMemcpyAsync(seed_x ? yc.data() : eigvec, A.y.p, sizeof(double) * A.Lc, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (seed_x) {  // row 0 of the lifted layout
      std::fill(eigvec, eigvec + L, 0.0);
      for (long x = 0; x < A.Lc; ++x) eigvec[x * r] = yc[x];
    }
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  return DPGO_HIP_OK;
}

}  // extern "C"

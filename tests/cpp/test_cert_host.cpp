// CPU test of the certificates' host numerics (dpgo_amd/csrc/host_eig.h, cert_host.h): the dense and tridiagonal
// eigen-solvers, the start stream's three placement rules, the locked seed block and the Lanczos plan.  The program
// builds its inputs itself.  No GPU, no libdpgo_hip.so, no HIP.
//
// Bounds.  SymEig: residual max |A z - w z| <= 8 m eps |A|_F and max |Z^T Z - I| <= 8 m eps; the solver measured
// <= 0.48 m eps |A|_F and <= 0.84 m eps on these families up to m = 500, the factor 8 is headroom for another libm
// or compiler.  TridiagValues: both modes run the same QL recurrence on the values (measured difference 0), 4 eps
// scale allows a compiler to order the rotations' arithmetic differently.  TridiagLowestVector: four solves with the
// shift at 1e-3 of the gap below the lowest value leave (1e-3)^4 of the other components: 1e-10.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../dpgo_amd/csrc/cert_host.h"
#include "../../dpgo_amd/csrc/host_eig.h"

using namespace dpgo;

static int g_fail = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      if (++g_fail <= 40) std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                 \
  } while (0)

static const double kEps = DBL_EPSILON;
typedef std::vector<double> Vec;

static double uni(SplitMix64& g, double lo, double hi) { return lo + (hi - lo) * g.uniform(); }

// ---- SymEig --------------------------------------------------------------------------------------------------------
static double g_res_worst = 0.0, g_orth_worst = 0.0;  // in units of m eps |A|_F and m eps

static void check_sym_eig(const char* what, int m, const Vec& A) {
  Vec w, Z;
  sym_eig(m, A, w, Z);
  EXPECT(static_cast<int>(w.size()) == m && static_cast<int>(Z.size()) == m * m);
  if (static_cast<int>(w.size()) != m || static_cast<int>(Z.size()) != m * m) return;
  for (int c = 0; c + 1 < m; ++c) EXPECT(w[c] <= w[c + 1]);
  double fro = 0.0, res = 0.0, orth = 0.0;
  for (double a : A) fro += a * a;
  fro = std::sqrt(fro);
  for (int c = 0; c < m; ++c)
    for (int i = 0; i < m; ++i) {
      double acc = 0.0;
      for (int j = 0; j < m; ++j) acc += A[static_cast<size_t>(i) * m + j] * Z[static_cast<size_t>(c) * m + j];
      res = std::max(res, std::fabs(acc - w[c] * Z[static_cast<size_t>(c) * m + i]));
    }
  for (int a = 0; a < m; ++a)
    for (int c = a; c < m; ++c) {
      double acc = 0.0;
      for (int i = 0; i < m; ++i) acc += Z[static_cast<size_t>(a) * m + i] * Z[static_cast<size_t>(c) * m + i];
      orth = std::max(orth, std::fabs(acc - (a == c ? 1.0 : 0.0)));
    }
  const bool ok = res <= 8.0 * m * kEps * fro && orth <= 8.0 * m * kEps;
  if (!ok) std::printf("  %s m=%d: residual %.3e (|A|_F %.3e), orthogonality %.3e\n", what, m, res, fro, orth);
  EXPECT(res <= 8.0 * m * kEps * fro);
  EXPECT(orth <= 8.0 * m * kEps);
  if (fro > 0.0) g_res_worst = std::max(g_res_worst, res / (m * kEps * fro));
  g_orth_worst = std::max(g_orth_worst, orth / (m * kEps));
}

static Vec random_sym(int m, SplitMix64& g) {
  Vec A(static_cast<size_t>(m) * m);
  for (int i = 0; i < m; ++i)
    for (int j = i; j < m; ++j) A[static_cast<size_t>(i) * m + j] = A[static_cast<size_t>(j) * m + i] = uni(g, -1.0, 1.0);
  return A;
}

// B diag(s) B^T with B m x k random, exactly symmetric
static Vec gram(int m, const Vec& s, SplitMix64& g) {
  const int k = static_cast<int>(s.size());
  Vec B(static_cast<size_t>(m) * k), A(static_cast<size_t>(m) * m);
  for (double& b : B) b = uni(g, -1.0, 1.0);
  for (int i = 0; i < m; ++i)
    for (int j = i; j < m; ++j) {
      double acc = 0.0;
      for (int q = 0; q < k; ++q) acc += B[static_cast<size_t>(i) * k + q] * s[q] * B[static_cast<size_t>(j) * k + q];
      A[static_cast<size_t>(i) * m + j] = A[static_cast<size_t>(j) * m + i] = acc;
    }
  return A;
}

static void test_sym_eig() {
  SplitMix64 g(101);
  for (int m : {1, 2, 3, 4, 9, 15, 24, 40, 200}) check_sym_eig("random", m, random_sym(m, g));
  for (int m : {3, 8, 24}) {
    Vec I(static_cast<size_t>(m) * m, 0.0);
    for (int i = 0; i < m; ++i) I[static_cast<size_t>(i) * m + i] = 1.0;
    check_sym_eig("identity", m, I);
    check_sym_eig("ones", m, Vec(static_cast<size_t>(m) * m, 1.0));
    check_sym_eig("zero", m, Vec(static_cast<size_t>(m) * m, 0.0));
  }
  {  // Wilkinson W21+: diagonal |10 - i|, off-diagonals 1 (pairs of eigenvalues agreeing to ~1e-14)
    const int m = 21;
    Vec W(static_cast<size_t>(m) * m, 0.0);
    for (int i = 0; i < m; ++i) {
      W[static_cast<size_t>(i) * m + i] = std::abs(10 - i);
      if (i + 1 < m) W[static_cast<size_t>(i) * m + i + 1] = W[static_cast<size_t>(i + 1) * m + i] = 1.0;
    }
    check_sym_eig("wilkinson", m, W);
  }
  for (int m : {8, 24}) {
    Vec s(m);
    for (int k = 0; k < m; ++k) s[k] = std::pow(10.0, -2.0 * k);
    check_sym_eig("graded gram", m, gram(m, s, g));
    check_sym_eig("rank-3 gram", m, gram(m, Vec(3, 1.0), g));
  }
  {  // the projected matrix after a thick restart: diagonal Ritz values with an arrowhead column at `keep`, then
     // tridiagonal
    const int m = 40, keep = 10;
    Vec T(static_cast<size_t>(m) * m, 0.0);
    for (int i = 0; i < m; ++i) T[static_cast<size_t>(i) * m + i] = uni(g, -3.0, 3.0);
    for (int i = 0; i < keep; ++i) T[static_cast<size_t>(i) * m + keep] = T[static_cast<size_t>(keep) * m + i] = uni(g, -1.0, 1.0);
    for (int i = keep; i + 1 < m; ++i) T[static_cast<size_t>(i) * m + i + 1] = T[static_cast<size_t>(i + 1) * m + i] = uni(g, 0.1, 1.1);
    check_sym_eig("thick restart", m, T);
  }
  std::printf("  sym_eig worst: residual %.2f m eps |A|_F, orthogonality %.2f m eps\n", g_res_worst, g_orth_worst);
}

// ---- the tridiagonal solvers ---------------------------------------------------------------------------------------
static void test_tridiag(bool lowest_vector) {
  SplitMix64 g(202);
  for (int k : {2, 5, 60, 600}) {
    Vec a(k), e(k - 1);
    for (double& x : a) x = uni(g, -3.0, 3.0);
    for (double& x : e) x = uni(g, 0.1, 1.1);
    Vec w, wv, Z;
    tridiag_eig(a, e, w, nullptr);
    tridiag_eig(a, e, wv, &Z);
    EXPECT(static_cast<int>(w.size()) == k && static_cast<int>(wv.size()) == k && static_cast<int>(Z.size()) == k * k);
    const double scale = std::max(std::fabs(wv.front()), std::fabs(wv.back()));
    if (!lowest_vector) {
      double diff = 0.0;
      for (int i = 0; i < k; ++i) diff = std::max(diff, std::fabs(w[i] - wv[i]));
      for (int i = 0; i + 1 < k; ++i) EXPECT(w[i] <= w[i + 1]);
      std::printf("  k=%d: values-only against vector mode %.3e (scale %.3f)\n", k, diff, scale);
      EXPECT(diff <= 4.0 * kEps * scale);
      continue;
    }
    const Vec z = tridiag_lowest_vector(a, e, w[0], w[1], scale);
    EXPECT(static_cast<int>(z.size()) == k);
    double dot = 0.0, diff = 0.0;
    for (int i = 0; i < k; ++i) dot += z[i] * Z[i];
    for (int i = 0; i < k; ++i) diff = std::max(diff, std::fabs(z[i] - (dot < 0.0 ? -Z[i] : Z[i])));
    std::printf("  k=%d: lowest vector against QL %.3e (gap %.3f)\n", k, diff, w[1] - w[0]);
    EXPECT(diff <= 1e-10);
  }
}

// ---- StartStream ---------------------------------------------------------------------------------------------------
static void test_start_stream() {
  // the values tests/test_lobpcg_reference.py::test_start_block_is_the_certificates_stream pins
  const double first[12] = {-0x1.d838098bf03d6p-1, -0x1.566c5f4f22040p-2, -0x1.1521adcb4a660p-2, -0x1.e5ac92705bb60p-4,
                            -0x1.d03523a419bacp-1, -0x1.0a4036a3563c4p-2, -0x1.5a4cbc34f78a2p-1, -0x1.b5d9659fe8fb8p-1,
                            0x1.6a89fee36b2e6p-1,  -0x1.04bdca98d3030p-1, -0x1.3ad074249f520p-2, -0x1.ae53fbd0584b8p-3};
  for (int r : {3, 5}) {
    const long nc = 7, L = nc * r;
    const Vec full = cert_start(CertStart::Lifted, L, r), row0 = cert_start(CertStart::Row0, L, r),
              dense = cert_start(CertStart::Row0Dense, L, r);
    EXPECT(static_cast<long>(full.size()) == L && static_cast<long>(row0.size()) == nc &&
           static_cast<long>(dense.size()) == L);
    for (int i = 0; i < 12; ++i) EXPECT(full[i] == first[i]);
    for (double u : full) EXPECT(u >= -1.0 && u < 1.0);
    for (long x = 0; x < nc; ++x) EXPECT(row0[x] == full[x * r]);  // the stride-r subsequence
    for (long x = 0; x < L; ++x) EXPECT(dense[x] == (x % r == 0 ? full[x / r] : 0.0));  // the unstrided prefix on row 0
  }
}

// ---- SeedBlock -----------------------------------------------------------------------------------------------------
// |v - U U^T v| / |v| for the nl orthonormal vectors of U (Vectors layout)
static double outside_span(const Vec& U, int nl, long nc, const Vec& v) {
  Vec rem = v;
  for (int j = 0; j < nl; ++j) {
    double c = 0.0;
    for (long x = 0; x < nc; ++x) c += v[x] * U[j * nc + x];
    for (long x = 0; x < nc; ++x) rem[x] -= c * U[j * nc + x];
  }
  double n0 = 0.0, n1 = 0.0;
  for (long x = 0; x < nc; ++x) {
    n0 += v[x] * v[x];
    n1 += rem[x] * rem[x];
  }
  return std::sqrt(n1 / n0);
}

static void check_seed_block(int r, const Vec& X, int want_nl) {
  const int d = 3, n = 4, b = d + 1, ru = r + 1;
  const long nc = static_cast<long>(b) * n;
  Vec U, Ui;
  const int nl = seed_block(r, b, nc, X.data(), SeedLayout::Vectors, U);
  EXPECT(nl == want_nl);
  EXPECT(seed_block(r, b, nc, X.data(), SeedLayout::Interleaved, Ui) == nl);
  EXPECT(static_cast<long>(U.size()) == nc * ru && static_cast<long>(Ui.size()) == nc * ru);
  if (static_cast<long>(U.size()) != nc * ru || static_cast<long>(Ui.size()) != nc * ru || nl > ru) return;
  // the two layouts hold the same numbers; what is not a kept vector is exactly zero (the padding columns)
  for (long x = 0; x < nc; ++x)
    for (int j = 0; j < ru; ++j) {
      EXPECT(Ui[x * ru + j] == U[j * nc + x]);
      if (j >= nl) EXPECT(Ui[x * ru + j] == 0.0);
    }
  for (int a = 0; a < nl; ++a)
    for (int c = a; c < nl; ++c) {
      double acc = 0.0;
      for (long x = 0; x < nc; ++x) acc += U[a * nc + x] * U[c * nc + x];
      EXPECT(std::fabs(acc - (a == c ? 1.0 : 0.0)) <= 8.0 * nc * kEps);
    }
  // every row of X (the span of the kept directions) and the gauge lie in span(U); with nl as expected U spans no more
  Vec v(nc);
  for (int i = 0; i <= r; ++i) {
    for (long x = 0; x < nc; ++x) v[x] = i < r ? X[x * r + i] : (x % b == b - 1 ? 1.0 : 0.0);
    EXPECT(outside_span(U, nl, nc, v) <= 1e-12);
  }
}

static void test_seed_block() {
  SplitMix64 g(303);
  const long nc = 16;
  for (int r : {3, 5}) {
    Vec X(nc * r);
    for (double& x : X) x = uni(g, -1.0, 1.0);
    check_seed_block(r, X, r + 1);  // full rank, the gauge independent of the rows
    Vec X2 = X;
    for (long x = 0; x < nc; ++x) X2[x * r + 1] = X2[x * r];  // two equal rows: one direction less
    check_seed_block(r, X2, r);
    Vec X3 = X;
    for (long x = 0; x < nc; ++x) X3[x * r + r - 1] = x % 4 == 3 ? 1.0 : 0.0;  // a row equal to the gauge: it is dropped
    check_seed_block(r, X3, r);
  }
}

// ---- LanczosPlan ---------------------------------------------------------------------------------------------------
static void test_lanczos_plan() {
  LanczosPlan p = lanczos_plan(300, 0, 1000, 0);  // no basis limit: every step kept
  EXPECT(p.ok && !p.dense && p.mmax == 300 && p.keep == 0);
  p = lanczos_plan(600, 0, 96, 0);  // ... up to the dimension
  EXPECT(p.ok && !p.dense && p.mmax == 96 && p.keep == 0);
  p = lanczos_plan(600, 0, 32, 4);  // ... less the locked block's slots
  EXPECT(p.ok && !p.dense && p.mmax == 28 && p.keep == 0);
  p = lanczos_plan(4000, 8, 1000, 0);
  EXPECT(p.ok && p.dense && p.mmax == 8 && p.keep == 4);  // min(8 / 2, max(8, 2))
  p = lanczos_plan(4000, 40, 1000, 6);
  EXPECT(p.ok && p.dense && p.mmax == 40 && p.keep == 10);  // min(20, max(8, 10))
  p = lanczos_plan(4000, 60, 1000, 6);
  EXPECT(p.ok && p.dense && p.mmax == 60 && p.keep == 15);  // min(30, max(8, 15))
  p = lanczos_plan(4000, 60, 30, 6);  // the basis limit above the free dimension: mmax = 24
  EXPECT(p.ok && p.dense && p.mmax == 24 && p.keep == 8);  // min(12, max(8, 6))
  p = lanczos_plan(300, 0, 5, 4);  // one free dimension: refused
  EXPECT(!p.ok && p.mmax == 1);
  p = lanczos_plan(300, 40, 4, 4);
  EXPECT(!p.ok && p.mmax == 0);
  EXPECT(lanczos_plan(2, 0, 100, 0).ok);
  // a Ritz check is due: tridiagonal every max(5, m / 250 * 5); dense m <= 200 && m % 20 == 0, or m % 500 == 0
  const int ms[6] = {5, 20, 200, 250, 500, 1250};
  const bool tri[6] = {true, true, true, true, true, true}, den[6] = {false, true, true, false, true, false};
  for (int i = 0; i < 6; ++i) {
    EXPECT(ritz_check_due(false, ms[i]) == tri[i]);
    EXPECT(ritz_check_due(true, ms[i]) == den[i]);
  }
  EXPECT(!ritz_check_due(false, 7) && !ritz_check_due(false, 249));
  EXPECT(ritz_check_due(false, 255) && !ritz_check_due(false, 505));  // the step 5 up to 499, 10 from 500
  EXPECT(!ritz_check_due(false, 1260) && ritz_check_due(false, 1275));  // 25 from 1250
  EXPECT(!ritz_check_due(true, 10) && !ritz_check_due(true, 220) && ritz_check_due(true, 1000));
}

static void run(const char* name, void (*fn)()) {
  const int before = g_fail;
  fn();
  std::printf("[%s] %s\n", g_fail == before ? "PASS" : "FAIL", name);
}

int main() {
  run("SymEig", test_sym_eig);
  run("TridiagValues", [] { test_tridiag(false); });
  run("TridiagLowestVector", [] { test_tridiag(true); });
  run("StartStream", test_start_stream);
  run("SeedBlock", test_seed_block);
  run("LanczosPlan", test_lanczos_plan);
  return g_fail == 0 ? 0 : 1;
}

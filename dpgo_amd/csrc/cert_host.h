// Host side of the certificates of lambda_min(S(X)) that needs no device: the random stream, the start values, the
// locked seed block of DPGO_CERT_SEED_X and the Lanczos plan.  No HIP header, no handle: certify.cpp, blockcert.cpp,
// exact.cpp and graph.cpp use it, tests/cpp/test_cert_host.cpp checks it without a GPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace dpgo {

// SplitMix64 (the oracle's generator of the same name)
struct SplitMix64 {
  uint64_t state;
  explicit SplitMix64(uint64_t s) : state(s) {}
  uint64_t next() {
    state += 0x9E3779B97F4A7C15ULL;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
  }
  double uniform() { return static_cast<double>(next() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
};

// The certificates' start values u_1, u_2, ... = 2 uniform() - 1 in [-1, 1) of the stream of seed 0x5EED, in the
// lifted r x (d+1) n layout (L = r (d+1) n doubles, entry x = column x / r, row x % r).  The rules differ only in
// which stream element lands where:
enum class CertStart {
  Lifted,    // L values, entry x = u_{x+1}: all r rows (block certificate, unseeded Lanczos)
  Row0,      // L / r values, compact row 0 of the Lifted vector: entry x = u_{x r + 1} (seeded Lanczos)
  Row0Dense  // L values, row 0 filled without skipping: entry x r = u_{x+1}, rows 1.. zero (Cholesky certificate)
};
std::vector<double> cert_start(CertStart rule, long L, int r);

constexpr double kSeedKeep = 1e-6;   // eigenvalues of X X^T kept for U, relative to the largest
constexpr double kSeedDrop = 1e-10;  // a seed whose remainder is below this share of its norm is dropped

// The locked block U of DPGO_CERT_SEED_X on row 0 of the lifted layout (nc = (d+1) n entries per vector, b = d + 1;
// X as the device holds it, entry x r + i = row i of column x): the principal row directions of X, largest first
// (eigenvalue of X X^T >= kSeedKeep of the largest: S(X) X^T ~ 0 at a critical point, but a row at the noise level of
// a rank-deficient X is in S's null space only to within |RieGrad| / its norm), then the translation gauge (every
// pose's translation entry = 1, an exact null vector of S).  Classical Gram-Schmidt twice; a candidate whose remainder
// is <= kSeedDrop of its norm is dropped.  Returns the number nl <= r + 1 of vectors kept; U has nc (r + 1) doubles,
// zero wherever no kept vector is.
enum class SeedLayout {
  Interleaved,  // entry x of vector j at U[x (r + 1) + j] (the block certificate's device layout)
  Vectors       // vector j at U[j nc .. (j + 1) nc) (the Lanczos basis slots)
};
int seed_block(int r, int b, long nc, const double* X, SeedLayout layout, std::vector<double>& U);

// The Lanczos certificate's plan (Lc: length of a basis vector, nseed: slots reserved for the locked block).
// basis_max = 0: the chain keeps every step (T tridiagonal); otherwise thick restarts from the lowest `keep` Ritz
// vectors once the chain has mmax vectors (T dense: arrowhead + tridiagonal).  ok = false: the basis is too small.
struct LanczosPlan {
  int mmax = 0, keep = 0;
  bool dense = false, ok = false;
};
inline LanczosPlan lanczos_plan(int max_iters, int basis_max, long Lc, int nseed) {
  LanczosPlan p;
  p.mmax = static_cast<int>(std::min<long>(basis_max > 0 ? basis_max : max_iters, Lc - nseed));
  p.dense = basis_max > 0;
  p.keep = p.dense ? std::min(p.mmax / 2, std::max(8, p.mmax / 4)) : 0;
  p.ok = p.mmax >= 2;
  return p;
}
// A Ritz check is due at chain length m: every 5 steps on the tridiagonal T (every ~2 % of the basis beyond 250); with
// restarts (a dense O(m^3) eigensolve on the host) every 20 steps of a small basis, every 500 of a large one
inline bool ritz_check_due(bool dense, int m) {
  return dense ? ((m <= 200 && m % 20 == 0) || m % 500 == 0) : m % std::max(5, m / 250 * 5) == 0;
}

}  // namespace dpgo

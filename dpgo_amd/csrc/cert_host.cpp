// The certificates' host-only parts (cert_host.h).
#include "cert_host.h"

#include <cmath>

#include "host_eig.h"

namespace dpgo {

std::vector<double> cert_start(CertStart rule, long L, int r) {
  SplitMix64 rng(0x5EEDULL);
  auto u = [&]() { return 2.0 * rng.uniform() - 1.0; };
  std::vector<double> q(rule == CertStart::Row0 ? L / r : L, 0.0);
  switch (rule) {
    case CertStart::Lifted:
      for (long x = 0; x < L; ++x) q[x] = u();
      break;
    case CertStart::Row0:
      for (long x = 0; x < L / r; ++x) {
        q[x] = u();
        for (int i = 1; i < r; ++i) rng.next();  // the Lifted vector's rows 1..
      }
      break;
    case CertStart::Row0Dense:
      for (long x = 0; x < L; x += r) q[x] = u();
      break;
  }
  return q;
}

int seed_block(int r, int b, long nc, const double* X, SeedLayout layout, std::vector<double>& U) {
  const int ru = r + 1;
  const long sx = layout == SeedLayout::Interleaved ? ru : 1, sj = layout == SeedLayout::Interleaved ? 1 : nc;
  U.assign(static_cast<size_t>(nc) * ru, 0.0);
  std::vector<double> G(static_cast<size_t>(r) * r, 0.0), Z, w;
  for (long x = 0; x < nc; ++x)
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < r; ++j) G[static_cast<size_t>(i) * r + j] += X[x * r + i] * X[x * r + j];
  sym_eig(r, G, w, Z);
  std::vector<int> dirs;
  for (int e = r - 1; e >= 0; --e)
    if (w[e] >= kSeedKeep * w[r - 1]) dirs.push_back(e);
  int nl = 0;
  std::vector<double> v(nc), c(ru);
  for (size_t q = 0; q <= dirs.size(); ++q) {
    for (long x = 0; x < nc; ++x) {
      double acc = 0.0;
      if (q < dirs.size())
        for (int i = 0; i < r; ++i) acc += Z[static_cast<size_t>(dirs[q]) * r + i] * X[x * r + i];
      else
        acc = x % b == b - 1 ? 1.0 : 0.0;
      v[x] = acc;
    }
    double n0 = 0.0;
    for (long x = 0; x < nc; ++x) n0 += v[x] * v[x];
    n0 = std::sqrt(n0);
    for (int pass = 0; pass < 2 && nl > 0; ++pass) {
      std::fill(c.begin(), c.end(), 0.0);
      for (long x = 0; x < nc; ++x)
        for (int j = 0; j < nl; ++j) c[j] += v[x] * U[x * sx + j * sj];
      for (long x = 0; x < nc; ++x)
        for (int j = 0; j < nl; ++j) v[x] -= c[j] * U[x * sx + j * sj];
    }
    double n1 = 0.0;
    for (long x = 0; x < nc; ++x) n1 += v[x] * v[x];
    n1 = std::sqrt(n1);
    if (!(n1 > kSeedDrop * n0)) continue;  // in the span of the previous ones
    for (long x = 0; x < nc; ++x) U[x * sx + nl * sj] = v[x] / n1;
    ++nl;
  }
  return nl;
}

}  // namespace dpgo

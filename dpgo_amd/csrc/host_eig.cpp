// Dense symmetric eigen-solvers on the host (host_eig.h).
#include "host_eig.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace dpgo {

void tridiag_eig(std::vector<double> a, std::vector<double> e, std::vector<double>& w, std::vector<double>* Zout) {
  const int k = static_cast<int>(a.size());
  const bool vectors = Zout != nullptr;
  std::vector<double> Z(vectors ? static_cast<size_t>(k) * k : 0, 0.0);
  for (int i = 0; i < k && vectors; ++i) Z[static_cast<size_t>(i) * k + i] = 1.0;
  e.resize(k, 0.0);
  for (int l = 0; l < k; ++l) {
    for (int iter = 0; iter < 200; ++iter) {
      int m = l;
      for (; m < k - 1; ++m) {
        const double dd = std::fabs(a[m]) + std::fabs(a[m + 1]);
        if (std::fabs(e[m]) <= 1e-16 * dd) break;
      }
      if (m == l) break;
      double g = (a[l + 1] - a[l]) / (2.0 * e[l]);
      double r = std::hypot(g, 1.0);
      g = a[m] - a[l] + e[l] / (g + std::copysign(r, g));
      double s = 1.0, c = 1.0, p = 0.0;
      int i = m - 1;
      for (; i >= l; --i) {
        double f = s * e[i];
        const double bb = c * e[i];
        r = std::hypot(f, g);
        e[i + 1] = r;
        if (r == 0.0) {
          a[i + 1] -= p;
          e[m] = 0.0;
          break;
        }
        s = f / r;
        c = g / r;
        g = a[i + 1] - p;
        r = (a[i] - g) * s + 2.0 * c * bb;
        p = s * r;
        a[i + 1] = g + p;
        g = c * r - bb;
        for (int q = 0; q < k && vectors; ++q) {
          f = Z[static_cast<size_t>(i + 1) * k + q];
          Z[static_cast<size_t>(i + 1) * k + q] = s * Z[static_cast<size_t>(i) * k + q] + c * f;
          Z[static_cast<size_t>(i) * k + q] = c * Z[static_cast<size_t>(i) * k + q] - s * f;
        }
      }
      if (r == 0.0 && i >= l) continue;
      a[l] -= p;
      e[l] = g;
      e[m] = 0.0;
    }
  }
  if (vectors) {  // a holds the eigenvalues: the vectors in their ascending order
    std::vector<int> idx(k);
    for (int i = 0; i < k; ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int x, int y) { return a[x] < a[y]; });
    Zout->resize(Z.size());
    for (int i = 0; i < k; ++i)
      std::memcpy(Zout->data() + static_cast<size_t>(i) * k, &Z[static_cast<size_t>(idx[i]) * k], sizeof(double) * k);
  }
  std::sort(a.begin(), a.end());
  w.swap(a);
}

std::vector<double> tridiag_lowest_vector(const std::vector<double>& a, const std::vector<double>& e, double th0,
                                          double th1, double scale) {
  const int k = static_cast<int>(a.size());
  const double delta = std::max(1e-3 * std::max(th1 - th0, 0.0), 1e-13 * scale);
  const double sh = th0 - delta;
  std::vector<double> dd(k), l(k, 0.0), x(k, 1.0);
  dd[0] = a[0] - sh;
  for (int i = 1; i < k; ++i) {
    l[i] = e[i - 1] / dd[i - 1];
    dd[i] = a[i] - sh - l[i] * e[i - 1];
  }
  for (int it = 0; it < 4; ++it) {
    for (int i = 1; i < k; ++i) x[i] -= l[i] * x[i - 1];
    x[k - 1] /= dd[k - 1];
    for (int i = k - 2; i >= 0; --i) x[i] = (x[i] - e[i] * x[i + 1]) / dd[i];
    double nrm = 0.0;
    for (double v : x) nrm += v * v;
    nrm = std::sqrt(nrm);
    for (double& v : x) v /= nrm;
  }
  return x;
}

void sym_eig(int m, std::vector<double> A, std::vector<double>& w, std::vector<double>& Z) {
  std::vector<double> Q(static_cast<size_t>(m) * m, 0.0), v(m), p(m), wv(m);
  for (int i = 0; i < m; ++i) Q[static_cast<size_t>(i) * m + i] = 1.0;
  auto a = [&](int i, int j) -> double& { return A[static_cast<size_t>(i) * m + j]; };
  for (int k = 0; k + 2 < m; ++k) {
    double xn = 0.0;
    for (int i = k + 1; i < m; ++i) xn += a(i, k) * a(i, k);
    xn = std::sqrt(xn);
    if (xn == 0.0) continue;
    const double alpha = a(k + 1, k) > 0.0 ? -xn : xn;
    std::fill(v.begin(), v.end(), 0.0);
    for (int i = k + 1; i < m; ++i) v[i] = a(i, k);
    v[k + 1] -= alpha;
    double vn2 = 0.0;
    for (int i = k + 1; i < m; ++i) vn2 += v[i] * v[i];
    if (vn2 == 0.0) continue;
    const double bt = 2.0 / vn2;
    // p = bt A v over rows k.., K = bt / 2 v^T p, w = p - K v; A -= v w^T + w v^T
    double K = 0.0;
    for (int i = k; i < m; ++i) {
      double acc = 0.0;
      for (int j = k + 1; j < m; ++j) acc += a(i, j) * v[j];
      p[i] = bt * acc;
      K += v[i] * p[i];
    }
    K *= 0.5 * bt;
    for (int i = k; i < m; ++i) wv[i] = p[i] - K * v[i];
    for (int i = k; i < m; ++i)
      for (int j = k; j < m; ++j) a(i, j) -= v[i] * wv[j] + wv[i] * v[j];
    // Q <- Q H
    for (int i = 0; i < m; ++i) {
      double acc = 0.0;
      for (int j = k + 1; j < m; ++j) acc += Q[static_cast<size_t>(i) * m + j] * v[j];
      acc *= bt;
      for (int j = k + 1; j < m; ++j) Q[static_cast<size_t>(i) * m + j] -= acc * v[j];
    }
  }
  std::vector<double> d(m), e(m, 0.0), Zt;
  for (int i = 0; i < m; ++i) {
    d[i] = a(i, i);
    if (i + 1 < m) e[i] = a(i, i + 1);
  }
  tridiag_eig(d, e, w, &Zt);
  Z.assign(static_cast<size_t>(m) * m, 0.0);
  for (int c = 0; c < m; ++c)
    for (int i = 0; i < m; ++i) {
      double acc = 0.0;
      for (int q = 0; q < m; ++q) acc += Q[static_cast<size_t>(i) * m + q] * Zt[static_cast<size_t>(c) * m + q];
      Z[static_cast<size_t>(c) * m + i] = acc;
    }
}

void jacobi_eig(int r, double A[8][8], double V[8][8]) {
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  // the rotation that annihilates A[p][q]; |a_pq| counts as zero only when adding 100 |a_pq| changes neither
  // |a_pp| nor |a_qq|
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < r - 1; ++p)
      for (int q = p + 1; q < r; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double g = 100.0 * std::fabs(apq);
        if (sweep > 3 && std::fabs(A[p][p]) + g == std::fabs(A[p][p]) && std::fabs(A[q][q]) + g == std::fabs(A[q][q])) {
          A[p][q] = A[q][p] = 0.0;
          continue;
        }
        rotated = true;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = std::isinf(theta) ? 0.0 : std::copysign(1.0, theta) / (std::fabs(theta) + std::hypot(1.0, theta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
        for (int k = 0; k < r; ++k) {  // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < r; ++k) {  // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = A[q][p] = 0.0;
        for (int k = 0; k < r; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
    if (!rotated) break;
  }
}

}  // namespace dpgo

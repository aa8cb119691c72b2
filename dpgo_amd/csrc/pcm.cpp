// Pairwise consistency of frame candidates (build-defined): the C ABI of the pair-test
// kernel, its host twin, and the maximum clique search.  See include/dpgo_hip.h; the pair test itself is pcm_pair.h.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <deque>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "graph_internal.h"
#include "kernels.h"
#include "pcm_pair.h"

using namespace dpgo;

namespace {

using u64 = unsigned long long;
constexpr const char* kNoDevice = "no gfx950 device available (no CPU fallback)";
constexpr long long kLLMax = std::numeric_limits<long long>::max();

// the checks every entry shares; on success word_off / dense_off hold ngroups + 1 offsets
int check_groups(int d, int m, const void* F, const void* x, int ngroups, const int* group_off, const void* adj,
                 long long adj_capacity, const void* degree, bool dense, std::vector<long long>& word_off,
                 std::vector<long long>& dense_off) {
  if (d != 2 && d != 3) return fail(DPGO_HIP_EINVAL, "pair_consistency: d must be 2 or 3");
  if (m < 0 || ngroups < 0) return fail(DPGO_HIP_EINVAL, "pair_consistency: negative m or ngroups");
  if (!group_off) return fail(DPGO_HIP_EINVAL, "pair_consistency: null group_off");
  if (group_off[0] != 0) return fail(DPGO_HIP_EINVAL, "pair_consistency: group_off must start at 0");
  for (int g = 0; g < ngroups; ++g)
    if (group_off[g + 1] < group_off[g]) return fail(DPGO_HIP_EINVAL, "pair_consistency: group_off descends");
  if (group_off[ngroups] != m) return fail(DPGO_HIP_EINVAL, "pair_consistency: group_off must end at m");
  if (m > 0 && (!F || !x || !degree)) return fail(DPGO_HIP_EINVAL, "pair_consistency: null F, x or degree");
  word_off.assign(static_cast<size_t>(ngroups) + 1, 0);
  DPGO_TRY(dpgo_hip_pair_consistency_words(ngroups, group_off, word_off.data(), adj_capacity));
  if (word_off[ngroups] > 0 && !adj) return fail(DPGO_HIP_EINVAL, "pair_consistency: null adj");
  dense_off.assign(static_cast<size_t>(ngroups) + 1, 0);
  for (int g = 0; g < ngroups; ++g) {
    const long long mg = group_off[g + 1] - group_off[g];
    dense_off[g + 1] = dense_off[g] + mg * mg;  // m < 2^31: the sum stays below 2^62
    if (dense && dense_off[g + 1] > DPGO_PCM_DENSE_MAX)
      return fail(DPGO_HIP_EINVAL, "pair_consistency: the dense e_rot / e_tra outputs are limited to "
                                   "DPGO_PCM_DENSE_MAX (2^26) entries over all groups");
  }
  return DPGO_HIP_OK;
}

template <int D>
void host_groups(const double* F, const double* x, int ngroups, const int* group_off,
                 const std::vector<long long>& word_off, const std::vector<long long>& dense_off, double cR2,
                 double ct2, u64* adj, int* degree, double* e_rot, double* e_tra) {
  constexpr int PW = D * (D + 1), REC = pcm_record<D>();
  std::vector<double> rec;
  for (int g = 0; g < ngroups; ++g) {
    const int g0 = group_off[g], mg = group_off[g + 1] - g0, words = (mg + 63) / 64;
    rec.resize(static_cast<size_t>(mg) * REC);
    for (int k = 0; k < mg; ++k) {
      std::memcpy(&rec[static_cast<size_t>(k) * REC], F + static_cast<size_t>(g0 + k) * PW, sizeof(double) * PW);
      std::memcpy(&rec[static_cast<size_t>(k) * REC + PW], x + static_cast<size_t>(g0 + k) * D, sizeof(double) * D);
    }
    for (int k = 0; k < mg; ++k) {
      u64* row = adj + word_off[g] + static_cast<long long>(k) * words;
      int deg = 0;
      for (int w = 0; w < words; ++w) {
        u64 word = 0;
        const int lend = std::min(mg, (w + 1) * 64);
        for (int l = w * 64; l < lend; ++l) {
          double er, et;
          pcm_pair_errors<D>(&rec[static_cast<size_t>(k) * REC], &rec[static_cast<size_t>(l) * REC], er, et);
          if (k != l && pcm_consistent(er, et, cR2, ct2)) word |= 1ULL << (l - w * 64);
          const long long at = dense_off[g] + static_cast<long long>(k) * mg + l;
          if (e_rot) e_rot[at] = er;
          if (e_tra) e_tra[at] = et;
        }
        row[w] = word;
        deg += __builtin_popcountll(word);
      }
      degree[g0 + k] = deg;
    }
  }
}

// the launch's device tables: the tile list and the three offset arrays
struct PcmTables {
  DevBuf<PcmTile> tiles;
  DevBuf<int> goff;
  DevBuf<long long> off;  // word_off then dense_off
  size_t ntiles = 0, G1 = 0;
  int upload(int ngroups, const int* group_off, const std::vector<long long>& word_off,
             const std::vector<long long>& dense_off, hipStream_t s) {
    std::vector<PcmTile> host;
    for (int g = 0; g < ngroups; ++g) {
      const int nt = (group_off[g + 1] - group_off[g] + 63) / 64;
      for (int rt = 0; rt < nt; ++rt)
        for (int ct = 0; ct < nt; ++ct) host.push_back(PcmTile{g, rt, ct});
    }
    if (host.size() > 0x7fffffffULL) return fail(DPGO_HIP_EINVAL, "pair_consistency: more than 2^31 - 1 tiles");
    ntiles = host.size();
    G1 = static_cast<size_t>(ngroups) + 1;
    HIP_TRY(tiles.ensure(std::max<size_t>(ntiles, 1)));
    HIP_TRY(goff.ensure(G1));
    HIP_TRY(off.ensure(2 * G1));
    if (ntiles) HIP_TRY(hipMemcpyAsync(tiles.p, host.data(), sizeof(PcmTile) * ntiles, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(goff.p, group_off, sizeof(int) * G1, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(off.p, word_off.data(), sizeof(long long) * G1, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(off.p + G1, dense_off.data(), sizeof(long long) * G1, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // the host vectors above leave scope
    return DPGO_HIP_OK;
  }
  hipError_t launch(int d, int m, const double* F, const double* x, double c_R, double c_t, u64* adj, int* degree,
                    double* e_rot, double* e_tra, hipStream_t s) const {
    return launch_pair_consistency(d, static_cast<long>(ntiles), tiles.p, F, x, goff.p, off.p, off.p + G1, c_R * c_R,
                                   c_t * c_t, adj, degree, m, e_rot, e_tra, s);
  }
};

// ---- maximum clique: bitset branch and bound with the greedy colouring bound ------------------------------------
struct CliqueSearch {
  int m, W;
  const u64* adj;
  long long budget, nodes = 0;
  bool aborted = false;
  std::vector<int> best, cur;
  struct Level {
    std::vector<u64> P, U, Q;
    std::vector<int> order, colour;
  };
  std::deque<Level> levels;  // references to earlier levels stay valid as it grows

  const u64* row(int v) const { return adj + static_cast<size_t>(v) * W; }
  static bool any(const std::vector<u64>& s) {
    for (u64 w : s)
      if (w) return true;
    return false;
  }
  static int first(const std::vector<u64>& s) {
    for (size_t w = 0; w < s.size(); ++w)
      if (s[w]) return static_cast<int>(w * 64) + __builtin_ctzll(s[w]);
    return -1;
  }
  Level& level(size_t depth) {
    while (levels.size() <= depth) {
      levels.emplace_back();
      levels.back().P.assign(W, 0);
      levels.back().U.assign(W, 0);
      levels.back().Q.assign(W, 0);
    }
    return levels[depth];
  }

  // the greedy incumbent: vertices by descending degree, ties to the lower index
  void greedy() {
    std::vector<int> deg(m), idx(m);
    for (int v = 0; v < m; ++v) {
      int s = 0;
      for (int w = 0; w < W; ++w) s += __builtin_popcountll(row(v)[w]);
      deg[v] = s;
    }
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return deg[a] > deg[b]; });
    std::vector<u64> P(W, 0);
    for (int v = 0; v < m; ++v) P[v / 64] |= 1ULL << (v % 64);
    for (int v : idx) {
      if (!(P[v / 64] >> (v % 64) & 1)) continue;
      best.push_back(v);
      for (int w = 0; w < W; ++w) P[w] &= row(v)[w];
    }
  }

  // levels[depth].P holds the candidates adjacent to every vertex of cur
  void expand(size_t depth) {
    if (budget >= 0 && nodes >= budget) {
      aborted = true;
      return;
    }
    ++nodes;
    Level& L = level(depth);
    L.order.clear();
    L.colour.clear();
    L.U = L.P;
    for (int k = 1; any(L.U); ++k) {  // colour class k: a maximal independent set of what is left
      L.Q = L.U;
      for (int v = first(L.Q); v >= 0; v = first(L.Q)) {
        const u64* N = row(v);
        for (int w = 0; w < W; ++w) L.Q[w] &= ~N[w];
        L.Q[v / 64] &= ~(1ULL << (v % 64));
        L.U[v / 64] &= ~(1ULL << (v % 64));
        L.order.push_back(v);
        L.colour.push_back(k);
      }
    }
    for (int i = static_cast<int>(L.order.size()) - 1; i >= 0; --i) {
      if (cur.size() + L.colour[i] <= best.size()) return;
      const int v = L.order[i];
      cur.push_back(v);
      Level& C = level(depth + 1);
      const u64* N = row(v);
      for (int w = 0; w < W; ++w) C.P[w] = L.P[w] & N[w];
      if (!any(C.P)) {
        if (cur.size() > best.size()) best = cur;
      } else {
        expand(depth + 1);
      }
      cur.pop_back();
      if (aborted) return;
      L.P[v / 64] &= ~(1ULL << (v % 64));
    }
  }
};

}  // namespace

extern "C" {

int dpgo_hip_pair_consistency_words(int ngroups, const int* group_off, long long* word_off, long long capacity) {
  if (ngroups < 0 || !group_off || !word_off) return fail(DPGO_HIP_EINVAL, "pair_consistency_words: bad argument");
  word_off[0] = 0;
  for (int g = 0; g < ngroups; ++g) {
    const long long mg = static_cast<long long>(group_off[g + 1]) - group_off[g];
    if (mg < 0) return fail(DPGO_HIP_EINVAL, "pair_consistency_words: group_off descends");
    const long long words = mg * ((mg + 63) / 64);  // mg < 2^31: below 2^57
    if (words > kLLMax - word_off[g])
      return fail(DPGO_HIP_EINVAL, "pair_consistency_words: the adjacency words do not fit a long long");
    word_off[g + 1] = word_off[g] + words;
  }
  if (capacity >= 0 && word_off[ngroups] > capacity)
    return fail(DPGO_HIP_EINVAL, "pair_consistency_words: adj needs " + std::to_string(word_off[ngroups]) +
                                     " words, the capacity is " + std::to_string(capacity));
  return DPGO_HIP_OK;
}

int dpgo_pair_consistency_host(int d, int m, const double* F, const double* x, int ngroups, const int* group_off,
                               double c_R, double c_t, unsigned long long* adj, long long adj_capacity, int* degree,
                               double* e_rot, double* e_tra) {
  std::vector<long long> word_off, dense_off;
  DPGO_TRY(check_groups(d, m, F, x, ngroups, group_off, adj, adj_capacity, degree, e_rot || e_tra, word_off,
                        dense_off));
  if (m == 0) return DPGO_HIP_OK;
  const double cR2 = c_R * c_R, ct2 = c_t * c_t;
  if (d == 2)
    host_groups<2>(F, x, ngroups, group_off, word_off, dense_off, cR2, ct2, adj, degree, e_rot, e_tra);
  else
    host_groups<3>(F, x, ngroups, group_off, word_off, dense_off, cR2, ct2, adj, degree, e_rot, e_tra);
  return DPGO_HIP_OK;
}

int dpgo_hip_pair_consistency_dev(int d, int m, const double* F_dev, const double* x_dev, int ngroups,
                                  const int* group_off, double c_R, double c_t, unsigned long long* adj_dev,
                                  long long adj_capacity, int* degree_dev, double* e_rot_dev, double* e_tra_dev,
                                  void* stream) {
  std::vector<long long> word_off, dense_off;
  DPGO_TRY(check_groups(d, m, F_dev, x_dev, ngroups, group_off, adj_dev, adj_capacity, degree_dev,
                        e_rot_dev || e_tra_dev, word_off, dense_off));
  if (m == 0) return DPGO_HIP_OK;
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  hipStream_t s = static_cast<hipStream_t>(stream);
  PcmTables T;
  DPGO_TRY(T.upload(ngroups, group_off, word_off, dense_off, s));
  const hipError_t e = T.launch(d, m, F_dev, x_dev, c_R, c_t, adj_dev, degree_dev, e_rot_dev, e_tra_dev, s);
  const hipError_t w = hipStreamSynchronize(s);  // the tables are released on return
  HIP_TRY(e);
  HIP_TRY(w);
  return DPGO_HIP_OK;
}

int dpgo_hip_pair_consistency_bench(int d, int m, const double* F_dev, const double* x_dev, int ngroups,
                                    const int* group_off, double c_R, double c_t, unsigned long long* adj_dev,
                                    long long adj_capacity, int* degree_dev, int warmup, int reps, double* ms) {
  std::vector<long long> word_off, dense_off;
  DPGO_TRY(check_groups(d, m, F_dev, x_dev, ngroups, group_off, adj_dev, adj_capacity, degree_dev, false, word_off,
                        dense_off));
  if (m <= 0 || warmup < 0 || reps <= 0 || !ms) return fail(DPGO_HIP_EINVAL, "pair_consistency_bench: bad argument");
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  hipStream_t s = nullptr;
  PcmTables T;
  DPGO_TRY(T.upload(ngroups, group_off, word_off, dense_off, s));
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  int rc = DPGO_HIP_OK;
  for (int i = 0; i < warmup + reps && rc == DPGO_HIP_OK; ++i) {
    hipError_t e = hipEventRecord(e0, s);
    if (e == hipSuccess) e = T.launch(d, m, F_dev, x_dev, c_R, c_t, adj_dev, degree_dev, nullptr, nullptr, s);
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float t = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    if (e != hipSuccess) rc = fail(DPGO_HIP_EDEVICE, std::string("pair_consistency_bench: ") + hipGetErrorString(e));
    if (i >= warmup) ms[i - warmup] = t;
  }
  (void)hipStreamSynchronize(s);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return rc;
}

int dpgo_hip_pair_consistency(int d, int m, const double* F, const double* x, int ngroups, const int* group_off,
                              double c_R, double c_t, unsigned long long* adj, long long adj_capacity, int* degree,
                              double* e_rot, double* e_tra) {
  std::vector<long long> word_off, dense_off;
  DPGO_TRY(check_groups(d, m, F, x, ngroups, group_off, adj, adj_capacity, degree, e_rot || e_tra, word_off,
                        dense_off));
  if (m == 0) return DPGO_HIP_OK;
  if (usable_devices() == 0) return fail(DPGO_HIP_ENODEV, kNoDevice);
  const size_t M = static_cast<size_t>(m), nF = M * d * (d + 1), nx = M * d;
  const size_t words = static_cast<size_t>(word_off[ngroups]), dense = static_cast<size_t>(dense_off[ngroups]);
  DevBuf<double> din, de;
  DevBuf<u64> dadj;
  DevBuf<int> ddeg;
  HIP_TRY(din.ensure(nF + nx));
  HIP_TRY(dadj.ensure(std::max<size_t>(words, 1)));
  HIP_TRY(ddeg.ensure(M));
  const int ne = (e_rot ? 1 : 0) + (e_tra ? 1 : 0);
  if (ne) HIP_TRY(de.ensure(std::max<size_t>(ne * dense, 1)));
  double* der = e_rot ? de.p : nullptr;
  double* det = e_tra ? de.p + (e_rot ? dense : 0) : nullptr;
  hipStream_t s = nullptr;
  HIP_TRY(hipMemcpyAsync(din.p, F, sizeof(double) * nF, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(din.p + nF, x, sizeof(double) * nx, hipMemcpyHostToDevice, s));
  DPGO_TRY(dpgo_hip_pair_consistency_dev(d, m, din.p, din.p + nF, ngroups, group_off, c_R, c_t, dadj.p,
                                         static_cast<long long>(words), ddeg.p, der, det, s));
  if (words) HIP_TRY(hipMemcpyAsync(adj, dadj.p, sizeof(u64) * words, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(degree, ddeg.p, sizeof(int) * M, hipMemcpyDeviceToHost, s));
  if (e_rot && dense) HIP_TRY(hipMemcpyAsync(e_rot, der, sizeof(double) * dense, hipMemcpyDeviceToHost, s));
  if (e_tra && dense) HIP_TRY(hipMemcpyAsync(e_tra, det, sizeof(double) * dense, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return DPGO_HIP_OK;
}

int dpgo_max_clique(int m, int words_per_row, const unsigned long long* adj_rows, long long node_budget, int* clique,
                    int* size, int* proven) {
  if (m < 0 || !size || !proven || (m > 0 && (!adj_rows || !clique)))
    return fail(DPGO_HIP_EINVAL, "max_clique: negative m or a null pointer");
  if (words_per_row < (m + 63) / 64) return fail(DPGO_HIP_EINVAL, "max_clique: words_per_row below ceil(m / 64)");
  if (m == 0) {
    *size = 0;
    *proven = 1;
    return DPGO_HIP_OK;
  }
  CliqueSearch S;
  S.m = m;
  S.W = words_per_row;
  S.adj = adj_rows;
  S.budget = node_budget;
  S.greedy();
  if (node_budget == 0) {
    S.aborted = true;
  } else {
    CliqueSearch::Level& L = S.level(0);
    for (int v = 0; v < m; ++v) L.P[v / 64] |= 1ULL << (v % 64);
    S.expand(0);
  }
  std::sort(S.best.begin(), S.best.end());
  std::copy(S.best.begin(), S.best.end(), clique);
  *size = static_cast<int>(S.best.size());
  *proven = S.aborted ? 0 : 1;
  return DPGO_HIP_OK;
}

}  // extern "C"

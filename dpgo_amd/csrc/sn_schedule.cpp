// The exact preconditioner's launch schedule (sn_schedule.h): index arithmetic only.
#include "sn_schedule.h"

#include <algorithm>

namespace dpgo {
namespace {

struct Batch {  // what every step below reads
  const std::vector<SupernodalFactor>& Fs;
  const std::vector<long>& pose_off;
  int b, r;
  std::vector<int> base;                   // [agents + 1] first batch node of each agent
  std::vector<std::vector<int>> by_depth;  // per depth its nodes: agents ascending, then postorder index ascending
};

inline int s_pad(const SnSchedule& S, int g, int b) { return sn_pad(S.s[g] * b); }
inline int t_pad(const SnSchedule& S, int g, int b) { return sn_pad(S.t[g] * b); }

// ---- the batch's node list (agents in order, each in postorder): sizes, offsets, poses, extend-add lists
void node_layout(const Batch& B, bool guard, SnSchedule& S) {
  const int b = B.b, K = static_cast<int>(B.Fs.size()), nn = B.base[K];
  S.nodes = nn;
  for (auto* v : {&S.panel_off, &S.f_off, &S.u_off}) v->resize(nn);
  for (auto* v : {&S.s, &S.t, &S.poses_off, &S.cpos_off, &S.node_agent}) v->resize(nn);
  // guard (debug runs): a one-tile gap after EVERY supernode's panel, so a write past a node's panel into the next
  // changes a gap and a read past it meets the gap's NaN
  const long kGap = guard ? static_cast<long>(kSnTile) * kSnTile : 0;
  for (int a = 0; a < K; ++a) {
    const auto& nodes = B.Fs[a].nodes;
    const long off = B.pose_off[a];
    for (size_t x = 0; x < nodes.size(); ++x) {
      const int g = B.base[a] + static_cast<int>(x);
      const SnNode& nd = nodes[x];
      const int s = static_cast<int>(nd.S.size()), t = static_cast<int>(nd.R.size());
      S.s[g] = s;
      S.t[g] = t;
      S.node_agent[g] = a;
      {  // scalars: POTRF of the frontal S block, TRSM of the R rows, the update of the R x R frontal block
        const double ss = static_cast<double>(s) * b, ts = static_cast<double>(t) * b;
        S.flops += ss * ss * ss / 3.0 + ss * ss * ts + ss * ts * ts;
        S.inv_flops += ss * ss * ss / 3.0 + ss * ss * ts;
      }
      S.panel_off[g] = S.po;
      S.po += sn_panel_tiles(s * b, t * b) * kSnTile * kSnTile;
      if (guard) {
        S.guards.emplace_back(S.po, kGap);
        S.po += kGap;
      }
      S.f_off[g] = S.fo;
      S.fo += static_cast<long>(sn_pad(s * b) + sn_pad(t * b)) * B.r;
      S.u_off[g] = S.uo;
      S.uo += static_cast<long>(t) * b * B.r;
      S.poses_off[g] = static_cast<int>(S.poses.size());
      for (int v : nd.S) S.poses.push_back(static_cast<int>(off + v));
      for (int v : nd.R) S.poses.push_back(static_cast<int>(off + v));
      // per frontal position, its children's contributions in child order
      std::vector<std::vector<SnPair>> at(s + t);
      for (int c : nd.children) {
        const SnNode& ch = nodes[c];
        for (size_t i = 0; i < ch.R.size(); ++i) at[ch.to_parent[i]].push_back({B.base[a] + c, static_cast<int>(i)});
      }
      S.cpos_off[g] = static_cast<int>(S.cpos.size());
      S.cpos.push_back(static_cast<int>(S.contrib.size()));
      for (int p = 0; p < s + t; ++p) {
        S.contrib.insert(S.contrib.end(), at[p].begin(), at[p].end());
        S.cpos.push_back(static_cast<int>(S.contrib.size()));
      }
    }
  }
}

// ---- the sweeps' work lists per tree level
void sweep_items(const Batch& B, bool fwd_small, SnSchedule& S) {
  const int b = B.b, nd = S.max_depth + 1;
  auto& items = S.items;
  S.levels.assign(nd, {});
  S.level_small.assign(nd, 0);
  for (int dep = 0; dep < nd; ++dep) {
    SnLevel& L = S.levels[dep];
    const std::vector<int>& lev = B.by_depth[dep];
    L.asm0 = static_cast<int>(items.size());
    for (int g : lev) {
      const int rows = s_pad(S, g, b) + t_pad(S, g, b);
      for (int blk = 0; blk * kSnAsmRows < rows; ++blk) items.push_back({g, blk});
    }
    L.asm_n = static_cast<int>(items.size()) - L.asm0;
    // The sweeps' work items, nodes in order: forward one per row tile I of a node (it streams the row's
    // min(I + 1, ns) tiles) -- on a level of narrow nodes only (ns <= kSnSmallNs) through k_sn_fwd_small, else k_sn_fwd;
    // backward one per column tile J (nI - J tiles).  (Runs of a narrow node's row tiles in one workgroup measured
    // slower: 3.76 vs 3.48 ms per C5 forward sweep.)
    // (a level with both kinds runs every item through k_sn_fwd: a second launch there cost more than the narrow
    // nodes' items gained, profiles/r05k_levels.txt)
    bool small = fwd_small;
    for (int g : lev) small = small && s_pad(S, g, b) / kSnTile <= kSnSmallNs;
    for (int pass = 0; pass < 2; ++pass) {
      (pass == 0 ? L.fws0 : L.fwd0) = static_cast<int>(items.size());
      for (int g : lev) {
        if (small != (pass == 0)) continue;
        const int nI = (s_pad(S, g, b) + t_pad(S, g, b)) / kSnTile;
        for (int I = 0; I < nI; ++I) items.push_back({g, I});
      }
      if (pass == 0) L.fws_n = static_cast<int>(items.size()) - L.fws0;
    }
    S.level_small[dep] = small ? 1 : 0;
    L.fwd_n = static_cast<int>(items.size()) - L.fwd0;
    L.bwd0 = static_cast<int>(items.size());
    for (int g : lev) {
      const int nJ = s_pad(S, g, b) / kSnTile;
      for (int J = 0; J < nJ; ++J) items.push_back({g, J});
    }
    L.bwd_n = static_cast<int>(items.size()) - L.bwd0;
  }
}

// ---- narrow supernodes (<= kSnSmallNs S column tiles): a compact (s b + t b) x ld copy the sweeps read instead
// (k_sn_bwd reads every narrow node compact; the forward sweep only through k_sn_fwd_small, i.e. on levels of
// narrow nodes only -- k_sn_fwd keeps to the tiles); the bytes a sweep then reads; every sweep item's record
void compact_and_records(const Batch& B, bool compact, SnSchedule& S) {
  const int b = B.b, K = static_cast<int>(B.Fs.size());
  S.coff.assign(S.nodes, -1);
  for (int a = 0; a < K; ++a)
    for (size_t x = 0; x < B.Fs[a].nodes.size(); ++x) {
      const int g = B.base[a] + static_cast<int>(x);
      const int sb = S.s[g] * b, tb = S.t[g] * b;
      const double tiles = 8.0 * static_cast<double>(sn_panel_tiles(sb, tb) * kSnTile * kSnTile);
      if (compact && sn_pad(sb) / kSnTile <= kSnSmallNs) {
        S.coff[g] = S.co;
        const long dbl = static_cast<long>(sb + tb) * sn_compact_ld(sb);
        S.co += (dbl + 15) / 16 * 16;  // 128-byte aligned nodes
        S.sweep_bytes_bwd += 8.0 * static_cast<double>(dbl);
        S.sweep_bytes_fwd += S.level_small[B.Fs[a].nodes[x].depth] ? 8.0 * static_cast<double>(dbl) : tiles;
        for (int r0 = 0; r0 < sb + tb; r0 += kSnTile) S.citems.push_back({g, r0 / kSnTile});
      } else {
        S.sweep_bytes_fwd += tiles;
        S.sweep_bytes_bwd += tiles;
      }
    }
  S.desc.resize(S.items.size());
  for (size_t i = 0; i < S.items.size(); ++i) {
    const int g = S.items[i].x;
    SnItem& d = S.desc[i];
    d.node = g;
    d.tile = S.items[i].y;
    d.agent = S.node_agent[g];
    d.s = S.s[g];
    d.t = S.t[g];
    d.pad = 0;
    d.f_off = S.f_off[g];
    d.u_off = S.u_off[g];
    d.panel_off = S.panel_off[g];
    d.cpanel_off = S.coff[g];
    d.poses_off = S.poses_off[g];
  }
}

// ---- the device factorisation's tables: per tree level its nodes, per node its children, the positions of its R
// entries in its parent's frontal order, and the original entries of its S columns from the edge-stream Q
void factor_tables(const Batch& B, const std::vector<int>& n_agent, const std::vector<int>& inc_ptr,
                   const std::vector<SnPair>& inc, SnSchedule& S) {
  const int b = B.b, K = static_cast<int>(B.Fs.size()), nn = S.nodes, maxd = S.max_depth;
  S.level_off.assign(maxd + 2, 0);
  S.ch_off.assign(nn + 1, 0);
  S.tp_off.assign(nn, 0);
  S.ent_off.assign(nn + 1, 0);
  S.fac_off.assign(nn, 0);
  for (int dep = 0; dep <= maxd; ++dep) {
    S.level_off[dep] = static_cast<int>(S.fac_nodes.size());
    long lo = 0;
    for (int g : B.by_depth[dep]) {
      S.fac_nodes.push_back(g);
      const long M = s_pad(S, g, b) + t_pad(S, g, b);
      S.fac_off[g] = lo;
      lo += M * M;
    }
    S.level_size[dep & 1] = std::max(S.level_size[dep & 1], lo);
  }
  S.level_off[maxd + 1] = static_cast<int>(S.fac_nodes.size());
  std::vector<int> fpos;
  std::vector<std::pair<int, int>> rows;  // (q, code)
  for (int a = 0; a < K; ++a) {
    const auto& nodes = B.Fs[a].nodes;
    const long off = B.pose_off[a];
    fpos.assign(n_agent[a], -1);
    for (size_t x = 0; x < nodes.size(); ++x) {
      const int g = B.base[a] + static_cast<int>(x);
      const SnNode& nd = nodes[x];
      for (int c : nd.children) S.ch.push_back(B.base[a] + c);
      S.ch_off[g + 1] = static_cast<int>(S.ch.size());
      S.tp_off[g] = static_cast<int>(S.tp.size());
      S.tp.insert(S.tp.end(), nd.to_parent.begin(), nd.to_parent.end());
      const int s = static_cast<int>(nd.S.size());
      for (int p = 0; p < s; ++p) fpos[nd.S[p]] = p;
      for (size_t q = 0; q < nd.R.size(); ++q) fpos[nd.R[q]] = s + static_cast<int>(q);
      for (int p = 0; p < s; ++p) {
        S.ent.push_back(SnEntry{p, p, 0, 0});  // the diagonal block (+ shift)
        const long gv = off + nd.S[p];
        // incidences of the column's pose (ascending edge id), grouped by the frontal row they land in
        rows.clear();
        for (int k = inc_ptr[gv]; k < inc_ptr[gv + 1]; ++k) {
          const SnPair ie = inc[k];
          const int q = fpos[ie.y - off];
          if (q >= p) rows.emplace_back(q, ie.x);  // q < 0: eliminated below; q < p: the upper triangle
        }
        std::stable_sort(rows.begin(), rows.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
        for (size_t i = 0; i < rows.size();) {
          size_t j = i;
          const int s0 = static_cast<int>(S.src.size());
          for (; j < rows.size() && rows[j].first == rows[i].first; ++j) S.src.push_back(rows[j].second);
          S.ent.push_back(SnEntry{rows[i].first, p, s0, static_cast<int>(S.src.size())});
          i = j;
        }
      }
      S.ent_off[g + 1] = static_cast<int>(S.ent.size());
      for (int v : nd.S) fpos[v] = -1;
      for (int v : nd.R) fpos[v] = -1;
    }
  }
}

// ---- tile-parallel levels: every level by default (with the A strips in registers the tile kernels beat one
// workgroup per node at every depth: C5 151 -> 142 ms); tiled_max_nodes / tiled_min_tiles restrict them (0: never)
void tiled_sequence(const Batch& B, int tiled_max, int tiled_min_rows, SnSchedule& S) {
  const int b = B.b;
  S.fac_seq.assign(S.max_depth + 1, {});
  for (int dep = 0; dep <= S.max_depth; ++dep) {
    const int* lev = S.fac_nodes.data() + S.level_off[dep];
    const int n = S.level_off[dep + 1] - S.level_off[dep];
    int max_nt = 0, max_ns = 0, max_ch = 0;
    std::vector<int> ns(n), NT(n);  // per node of the level: S column tiles, row tiles
    for (int x = 0; x < n; ++x) {
      const int g = lev[x];
      ns[x] = s_pad(S, g, b) / kSnTile;
      NT[x] = ns[x] + t_pad(S, g, b) / kSnTile;
      max_nt = std::max(max_nt, NT[x]);
      max_ns = std::max(max_ns, ns[x]);
      max_ch = std::max(max_ch, S.ch_off[g + 1] - S.ch_off[g]);
    }
    if (n > tiled_max || max_nt < tiled_min_rows) continue;
    auto launch = [&](int kind, int param, const std::vector<SnPair>& it) {
      if (it.empty()) return;
      S.fac_seq[dep].push_back({kind, param, static_cast<int>(S.titems.size()), static_cast<int>(it.size())});
      S.titems.insert(S.titems.end(), it.begin(), it.end());
    };
    std::vector<SnPair> it;
    for (int phase = 0; phase < 2 + max_ch; ++phase) {  // assembly: zero, entries, children in order
      it.clear();
      for (int x = 0; x < n; ++x) {
        const int g = lev[x];
        long cnt = 0;
        if (phase == 0)
          cnt = NT[x];
        else if (phase == 1)
          cnt = (S.ent_off[g + 1] - S.ent_off[g] + kSnAsmRows - 1) / kSnAsmRows;
        else if (phase - 2 < S.ch_off[g + 1] - S.ch_off[g])
          cnt = (static_cast<long>(S.t[S.ch[S.ch_off[g] + phase - 2]]) * b + kSnTile - 1) / kSnTile;
        for (int y = 0; y < cnt; ++y) it.push_back({g, y});
      }
      launch(0, phase, it);
    }
    // right-looking over blocks of kBK columns: inside a block every K updates only the block's own columns
    // (the next diagonal tiles and L_IK depend on them); the tiles right of the block take the block's kBK
    // updates in one pass (kind 5: one load / store of F_IJ instead of kBK, the same MFMA order)
    for (int KB = 0; KB < max_ns; KB += kBK) {
      for (int K = KB; K < std::min(KB + kBK, max_ns); ++K) {
        std::vector<SnPair> dg, ts, up;
        for (int x = 0; x < n; ++x) {
          if (K >= ns[x]) continue;
          dg.push_back({lev[x], 0});
          for (int I = K + 1; I < NT[x]; ++I) {
            ts.push_back({lev[x], I});
            for (int J = K + 1; J <= std::min(I, KB + kBK - 1); ++J) up.push_back({lev[x], (I << 16) | J});
          }
        }
        launch(1, K, dg);
        launch(2, K, ts);
        launch(3, K, up);
      }
      it.clear();
      for (int x = 0; x < n; ++x) {
        if (KB >= ns[x]) continue;
        for (int I = KB + kBK; I < NT[x]; ++I)
          for (int J = KB + kBK; J <= I; ++J) it.push_back({lev[x], (I << 16) | J});
      }
      launch(5, KB, it);
    }
    for (int J = max_ns - 1; J >= 0; --J) {
      it.clear();
      for (int x = 0; x < n; ++x) {
        if (J >= ns[x]) continue;
        for (int I = J + 1; I < NT[x]; ++I) it.push_back({lev[x], I});
      }
      launch(4, J, it);
    }
  }
}

}  // namespace

SnSchedule build_sn_schedule(const std::vector<SupernodalFactor>& Fs, const std::vector<long>& pose_off,
                             const std::vector<int>& n_agent, int b, int r, const std::vector<int>& inc_ptr,
                             const std::vector<SnPair>& inc, const SnScheduleOptions& opt) {
  const int K = static_cast<int>(Fs.size());
  Batch B{Fs, pose_off, b, r, std::vector<int>(K + 1, 0), {}};
  SnSchedule S;
  for (int a = 0; a < K; ++a) {
    B.base[a + 1] = B.base[a] + static_cast<int>(Fs[a].nodes.size());
    for (const SnNode& nd : Fs[a].nodes) S.max_depth = std::max(S.max_depth, nd.depth);
  }
  // one pass over agents ascending and postorder index ascending files each node under its depth in exactly the
  // order a scan of all nodes per depth meets them
  B.by_depth.assign(S.max_depth + 1, {});
  for (int a = 0; a < K; ++a)
    for (size_t x = 0; x < Fs[a].nodes.size(); ++x) B.by_depth[Fs[a].nodes[x].depth].push_back(B.base[a] + static_cast<int>(x));
  node_layout(B, opt.guard, S);
  sweep_items(B, opt.fwd_small, S);
  compact_and_records(B, opt.compact, S);
  if (opt.device) {
    factor_tables(B, n_agent, inc_ptr, inc, S);
    tiled_sequence(B, opt.tiled_max_nodes, opt.tiled_min_tiles, S);
  }
  return S;
}

}  // namespace dpgo

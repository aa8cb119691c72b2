// The exact preconditioner's launch schedule: every index table the sweeps and the device factorisation read,
// computed on the host from the batch's supernodal trees.  Pure index arithmetic: no HIP header, no handle, no
// environment -- exact.cpp uploads the result, tests/cpp/test_sn_schedule.cpp checks it without a GPU.
#pragma once
#include <utility>
#include <vector>

#include "chol_internal.h"

namespace dpgo {

// An item pair as the kernels read it (int2: x then y); exact.cpp asserts the layout against int2
struct SnPair {
  int x, y;
};

struct SnLevel {  // item ranges into SnSchedule::items of one tree depth
  int asm0 = 0, asm_n = 0, fws0 = 0, fws_n = 0, fwd0 = 0, fwd_n = 0, bwd0 = 0, bwd_n = 0;  // fws: k_sn_fwd_small's
};

struct FacLaunch {  // one launch_sn_factor_tiled: titems[off .. off + count)
  int kind, param, off, count;
};

struct SnScheduleOptions {
  bool fwd_small = true;  // levels of narrow nodes only run their forward items through k_sn_fwd_small
  bool compact = true;    // narrow nodes keep a compact copy of their panel
  bool guard = false;     // a one-tile gap after every node's panel
  int tiled_max_nodes = 1 << 30, tiled_min_tiles = 1;  // levels factorised tile-parallel (0 nodes: never)
  bool device = false;    // also the device factorisation's tables
};

struct SnSchedule {
  int nodes = 0, max_depth = 0;
  // node layout (agents in order, each in postorder)
  std::vector<long> panel_off, f_off, u_off;
  std::vector<int> s, t, poses_off, poses, cpos_off, cpos, node_agent;
  std::vector<SnPair> contrib;
  // sweep schedule
  std::vector<SnPair> items;
  std::vector<SnLevel> levels;      // index = depth (0 = the roots)
  std::vector<char> level_small;    // per depth: every node narrow (its forward items through k_sn_fwd_small)
  // compact panels
  std::vector<long> coff;           // per node its compact offset, -1: tiles only
  std::vector<SnPair> citems;       // (node, 64-row block) of the compact copy
  long co = 0;                      // compact doubles in all
  // item records
  std::vector<SnItem> desc;
  // accounting
  double sweep_bytes_fwd = 0.0, sweep_bytes_bwd = 0.0, flops = 0.0, inv_flops = 0.0;
  std::vector<std::pair<long, long>> guards;  // (offset, doubles) of every gap
  long po = 0, fo = 0, uo = 0;                // doubles of panels (gaps included), frontal and update vectors
  // factor tables (device)
  std::vector<int> fac_nodes, level_off, ch_off, ch, tp_off, tp, ent_off, src;
  std::vector<long> fac_off;
  std::vector<SnEntry> ent;
  // tiled factor launches (device)
  std::vector<SnPair> titems;
  std::vector<std::vector<FacLaunch>> fac_seq;  // per depth; empty: one workgroup per node
  long level_size[2] = {0, 0};                  // frontal buffer doubles of the even / odd depths
};

// inc_ptr / inc: per batch-global pose its incidences in edge order, (2 edge + (pose == p1), other endpoint's
// global id), as sync_q_edges builds them; read only when opt.device
SnSchedule build_sn_schedule(const std::vector<SupernodalFactor>& Fs, const std::vector<long>& pose_off,
                             const std::vector<int>& n_agent, int b, int r, const std::vector<int>& inc_ptr,
                             const std::vector<SnPair>& inc, const SnScheduleOptions& opt);

}  // namespace dpgo

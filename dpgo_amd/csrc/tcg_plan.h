// What one trust-region Run queues and how: the flags of the tCG sequence and the queueing regime, decided from the
// optimiser parameters, the batch's tile counts and the tuning keys.  Pure arithmetic over plain ints: no HIP header,
// no handle, no environment -- optimize.cpp acts on the result, tests/cpp/test_tcg_plan.cpp checks it without a GPU.
#pragma once
#include <vector>

namespace dpgo {

struct TcgPlanIn {
  bool rtr = true;  // the algorithm is RTR (the plan is RTR's; RGD queues no tCG)
  bool single = true;  // RTR with one outer iteration (the RBCD setting)
  bool exact = false;  // the exact preconditioner
  int tr_max_inner = 0;
  bool status = false;  // the caller asked for the PGOAgent status
  bool predict_boundary = true;  // the previous call's first tCG step stopped every agent (may change between Runs)
  int fuse_finalize = 0;
  int K = 1, num_tiles = 0;
  // the handle's values of TUNE_FUSE_TCG, TUNE_FIRST_STEP, TUNE_CLASSIC_TCG, TUNE_TCG_LOOKAHEAD, TUNE_STATUS_PASS,
  // TUNE_SPLIT_STREAMS, TUNE_TAIL_FUSE and TUNE_TCG_BLOCK
  int fuse_tcg = 0, first_step = 0, classic_tcg = 0, lookahead = 0, status_pass = 0, split_streams = 0, tail_fuse = 0,
      tcg_block = 0;
};

// How a Run's tCG iterations are queued.  One-ahead: one published status per iteration, the host keeps one
// iteration queued ahead of the status it waits for.  All-ahead: every iteration queued at once, no status inside tCG.
enum class TcgRegime {
  None,             // tr_max_inner == 0
  ClassicOneAhead,  // the five-launch sequence (exact preconditioner, TUNE_FUSE_TCG, TUNE_CLASSIC_TCG)
  ClassicAllAhead,  // the same, every iteration at once (TUNE_TCG_LOOKAHEAD = 2 only)
  MergedOneAhead,   // the merged iteration
  MergedAllAhead,   // the merged iteration, the whole batch on the launch stream
  MergedSplit,      // ... in agent groups on the split streams (TUNE_SPLIT_STREAMS)
  MergedBlocked     // ... in agent blocks queued depth-first (TUNE_TCG_BLOCK)
};

// no status is published inside tCG: the rho test's status word tells whether any agent took a CG step
inline bool queued_all_ahead(TcgRegime r) {
  return r == TcgRegime::ClassicAllAhead || r == TcgRegime::MergedAllAhead || r == TcgRegime::MergedSplit ||
         r == TcgRegime::MergedBlocked;
}

struct TcgPlan {
  bool qf0 = false, full0 = false, spec = false, fuse_tcg = false, merged = false, tail_fuse = false,
       status_fold = false;
  TcgRegime regime = TcgRegime::None;
  std::vector<int> blocks;  // MergedBlocked: the blocks' agent boundaries, blocks[0] = 0 < ... < blocks.back() = K
};

// TUNE_SPLIT_STREAMS applies to batches of at least two agents and at most kSplitMaxTiles tiles: a small batch's
// kernels leave the chip part-idle and two half-batch streams fill it (-4.6 % ms/step at the 125 k-pose share),
// while at 1M (7,800 tiles per colour) the halves only share the chip (-0.7 %, within noise) and the per-launch
// timing of one half beside the other would no longer be a kernel's own duration.
inline bool merged_split(int K, int num_tiles, int fuse_finalize, int split_streams) {
  constexpr int kSplitMaxTiles = 4096;
  return K >= 2 && num_tiles <= kSplitMaxTiles && fuse_finalize == 0 && split_streams > 0;
}

// TUNE_TCG_BLOCK: the agent boundaries of the blocks the merged tCG loop is queued in, blocks[0] = 0 < ... <
// blocks.back() = K.  Runs of consecutive agents formed greedily: an agent joins the current block while the block
// stays within the target tile count, and a block has at least one agent (an agent larger than the target is a block
// of its own).  Left with fewer than two blocks -- the unblocked queueing -- when the key is off, the finalize is fused
// into the SpMM, or the whole batch fits in one block.  agent_tile_off: [K + 1] first tile of every agent.
inline void merged_blocks(int K, int num_tiles, int fuse_finalize, int target, const int* agent_tile_off,
                          std::vector<int>* blocks) {
  blocks->clear();
  if (target <= 0 || K < 2 || fuse_finalize != 0 || num_tiles <= target) return;
  blocks->push_back(0);
  int t_block = agent_tile_off[0];  // first tile of the current block
  for (int a = 1; a < K; ++a)
    if (agent_tile_off[a + 1] - t_block > target) {
      blocks->push_back(a);
      t_block = agent_tile_off[a];
    }
  blocks->push_back(K);
}

// f(x1), grad(x1), S(x1) at the start of a call: for RTR the first tCG start (delta = -Prec(grad), <z, grad>) is fused
// into the same pass.  (The exact solve runs as its own stages.)
inline bool tcg_start_fused(const TcgPlanIn& in) { return in.rtr && in.tr_max_inner > 0 && !in.exact; }

// Whether that first pass stores grad(x1).  grad(x1) itself is only read by a CG step (r = grad + alpha Hdelta), a
// retry Run or the explicit <g, eta>: when the previous call's first step stopped every agent (single Run), it is not
// stored and is recomputed, by the same MODE_EVAL_TCG pass (bitwise the same g), if it is needed.  This only chooses
// between storing and recomputing identical values: no result depends on it, so an agent's arithmetic does not depend
// on which other agents share its handle.
// (a first step forced to the full pass reads grad(x1) in that pass already: the merged HESS_QF_M's r_0)
inline bool tcg_start_stores_grad(const TcgPlanIn& in) {
  return !(tcg_start_fused(in) && in.single && in.predict_boundary && in.tr_max_inner > 0 && in.first_step != 2);
}

// One Run's plan.  Called once per Run: predict_boundary may have changed since the last one.
inline TcgPlan plan_run(const TcgPlanIn& in, const int* agent_tile_off) {
  TcgPlan p;
  // Consumer-side finalize (TUNE_FUSE_TCG): the step test's scalar logic runs in the update kernel's
  // prologue and the stopping test's in the direction update's, three launches per tCG iteration.
  p.fuse_tcg = in.fuse_tcg > 0 && !in.exact;
  // First step: only d_Hd is evaluated (MODE_QF: each edge once, no Hess[delta] vector).  A
  // boundary / negative-curvature exit needs nothing more (eta = tau delta stays implicit, <eta, Heta>
  // = tau^2 d_Hd); agents that take a CG step get Hess[delta] from a HESS pass over their tiles only.
  // Always the same formula for the first d_Hd, so an agent's result does not depend on the batch.
  p.qf0 = !in.exact && in.tr_max_inner > 0;
  // When the previous call took CG steps the first step test is the full pass (MODE_HESS_QF): same
  // d_Hd, and Hess[delta] is there for the agents that continue (no second pass over them).
  p.full0 = p.qf0 && (in.first_step == 2 || (in.first_step == 0 && !in.predict_boundary));
  // Single Run, first steps predicted on the boundary: the candidate, f(x2) and the rho test of the
  // agents whose first step already ended tCG are queued right behind the step test, before the host
  // learns whether any agent continues (those are retracted, evaluated and tested after their tCG:
  // the *_EXPL launches).
  p.spec = p.qf0 && in.single && !p.full0;
  // PGOAgent status folded into the retraction + rho test of a single Run (no k_sqdiff / OP_STATUS pass);
  // agents that never ran this call (|grad| < tol) are the separate pass's, run only when some did
  p.status_fold = in.status && in.single && in.status_pass == 0;
  // Merged tCG iteration (the default with block-Jacobi / no preconditioner): HESS_M, one finalize for
  // the step test and the stopping test (OP_TCG_STEP_CHECK), then k_tcg_updir -- three launches per
  // iteration instead of five, no z vector.  The exact preconditioner and TUNE_FUSE_TCG keep the
  // classic sequence (TUNE_CLASSIC_TCG forces it).
  p.merged = p.qf0 && !p.fuse_tcg && in.classic_tcg == 0;
  // TUNE_TAIL_FUSE: the last iteration's k_tcg_updir (eta += step delta and the <eta_old, Hdelta> partial, nothing
  // else) is not launched; the retraction that follows applies the step from registers (RetractTail).
  p.tail_fuse = p.merged && in.tail_fuse > 0;
  // Every iteration queued at once, no status published inside tCG (the CG regime, where tCG runs
  // to MAXITER or close: agents that stop skip their tiles, an all-stopped iteration costs three
  // near-empty launches).  Adaptive (default): when the previous call's tCG took CG steps.
  const int la = in.lookahead;
  const bool all_ahead = p.merged && in.single && p.full0 && la != 1 && (la == 2 || !in.predict_boundary);
  // TUNE_TCG_BLOCK: the batch's agents in blocks of consecutive agents, each block's iterations queued depth-first
  // (fewer than two blocks: not applied)
  if (all_ahead) merged_blocks(in.K, in.num_tiles, in.fuse_finalize, in.tcg_block, agent_tile_off, &p.blocks);
  const bool blocked = p.blocks.size() > 2;
  const bool split = all_ahead && !blocked && merged_split(in.K, in.num_tiles, in.fuse_finalize, in.split_streams);
  // The classic sequence (the exact preconditioner) queued the same way on request (TUNE_TCG_LOOKAHEAD = 2 only):
  // every iteration at once, agents that stopped skip their tiles and their supernodes, no status round trip
  // inside tCG.  Bitwise the one-ahead sequence (test_exact_lookahead_bitwise) but not the default: the dead
  // iterations cost more than the round trips they save (same-process A/B: C4 17.4 vs 16.7 ms/step, C5 101.8 vs
  // 100.8, profiles/r03ze_*).
  const bool classic_ahead = !p.merged && in.single && !p.qf0 && in.tr_max_inner > 0 && la == 2;
  if (blocked)
    p.regime = TcgRegime::MergedBlocked;
  else if (split)
    p.regime = TcgRegime::MergedSplit;
  else if (all_ahead)
    p.regime = TcgRegime::MergedAllAhead;
  else if (p.merged)
    p.regime = TcgRegime::MergedOneAhead;
  else if (in.tr_max_inner > 0)
    p.regime = classic_ahead ? TcgRegime::ClassicAllAhead : TcgRegime::ClassicOneAhead;
  return p;
}

}  // namespace dpgo

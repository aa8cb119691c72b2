// CPU test of the trust-region driver's plan (dpgo_amd/csrc/tcg_plan.h): which flags and which queueing regime a Run
// gets from the optimiser parameters, the batch and the tuning keys.  Invariants over every combination of inputs,
// named rows derived by hand from the definitions, and the agent-block rule.  No GPU, no libdpgo_hip.so, no HIP.
#include <cstdio>
#include <vector>

#include "../../dpgo_amd/csrc/tcg_plan.h"

using namespace dpgo;

static int g_fail = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      if (++g_fail <= 40) std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                 \
  } while (0)

// a => b
static bool implies(bool a, bool b) { return !a || b; }

struct Batch {
  int K;
  std::vector<int> tile_off;  // [K + 1]
  int num_tiles() const { return tile_off.back(); }
};

static Batch batch_of(const std::vector<int>& tiles_per_agent) {
  Batch B;
  B.K = static_cast<int>(tiles_per_agent.size());
  B.tile_off.push_back(0);
  for (int t : tiles_per_agent) B.tile_off.push_back(B.tile_off.back() + t);
  return B;
}

static TcgPlan plan_for(TcgPlanIn in, const Batch& B) {
  in.K = B.K;
  in.num_tiles = B.num_tiles();
  return plan_run(in, B.tile_off.data());
}

// ---- every combination of inputs: what must hold whatever the keys say ---------------------------------------------
static void check_invariants(const TcgPlanIn& in, const Batch& B) {
  const TcgPlan p = plan_for(in, B);
  const TcgRegime g = p.regime;
  int named = 0;  // exactly one of the seven regimes
  for (TcgRegime k : {TcgRegime::None, TcgRegime::ClassicOneAhead, TcgRegime::ClassicAllAhead,
                      TcgRegime::MergedOneAhead, TcgRegime::MergedAllAhead, TcgRegime::MergedSplit,
                      TcgRegime::MergedBlocked})
    named += g == k ? 1 : 0;
  EXPECT(named == 1);
  EXPECT((g == TcgRegime::None) == (in.tr_max_inner == 0));
  const bool at_once = g == TcgRegime::MergedBlocked || g == TcgRegime::MergedSplit || g == TcgRegime::MergedAllAhead;
  EXPECT(implies(at_once, p.merged && p.full0 && in.single && in.lookahead != 1));
  const bool one_ahead = g == TcgRegime::ClassicOneAhead || g == TcgRegime::MergedOneAhead;
  EXPECT(implies(p.spec, in.single && !p.full0 && one_ahead));
  EXPECT(implies(p.tail_fuse, p.merged));
  EXPECT(implies(p.merged, !in.exact && !p.fuse_tcg));
  EXPECT(implies(g == TcgRegime::ClassicAllAhead, in.exact && in.lookahead == 2 && in.single));
  EXPECT(implies(in.exact, !p.qf0 && !p.merged && !p.spec));
  const bool grouped = g == TcgRegime::MergedBlocked || g == TcgRegime::MergedSplit;
  EXPECT(implies(grouped, in.fuse_finalize == 0 && B.K >= 2));
  if (g == TcgRegime::MergedBlocked) {
    EXPECT(p.blocks.size() >= 3);  // at least two blocks
    EXPECT(!p.blocks.empty() && p.blocks.front() == 0 && p.blocks.back() == B.K);
    for (size_t i = 1; i < p.blocks.size(); ++i) EXPECT(p.blocks[i - 1] < p.blocks[i]);
  }
  EXPECT(p.status_fold == (in.status && in.single && in.status_pass == 0));
  EXPECT(queued_all_ahead(g) == (at_once || g == TcgRegime::ClassicAllAhead));
}

static long enumerate(const Batch& B) {
  long n = 0;
  TcgPlanIn in;
  in.rtr = true;
  for (int single = 0; single < 2; ++single)
    for (int exact = 0; exact < 2; ++exact)
      for (int inner : {0, 1, 10})
        for (int status = 0; status < 2; ++status)
          for (int pb = 0; pb < 2; ++pb)
            for (int ff = 0; ff < 3; ++ff)
              for (int fuse_tcg = 0; fuse_tcg < 2; ++fuse_tcg)
                for (int first = 0; first < 3; ++first)
                  for (int classic = 0; classic < 2; ++classic)
                    for (int la = 0; la < 3; ++la)
                      for (int sp = 0; sp < 2; ++sp)
                        for (int split = 0; split < 5; ++split)
                          for (int tail = 0; tail < 2; ++tail)
                            for (int block : {0, 3, 2000}) {
                              in.single = single != 0;
                              in.exact = exact != 0;
                              in.tr_max_inner = inner;
                              in.status = status != 0;
                              in.predict_boundary = pb != 0;
                              in.fuse_finalize = ff;
                              in.fuse_tcg = fuse_tcg;
                              in.first_step = first;
                              in.classic_tcg = classic;
                              in.lookahead = la;
                              in.status_pass = sp;
                              in.split_streams = split;
                              in.tail_fuse = tail;
                              in.tcg_block = block;
                              check_invariants(in, B);
                              ++n;
                            }
  return n;
}

// ---- named rows: the library's default keys, block-Jacobi, a single Run, tr_max_inner = 10 -------------------------
// Each expectation is worked out by hand from the definitions:
//   qf0 = !exact && inner > 0;  full0 = qf0 && (FIRST_STEP == 2 || (FIRST_STEP == 0 && !predict_boundary));
//   spec = qf0 && single && !full0;  merged = qf0 && !(FUSE_TCG && !exact) && !CLASSIC_TCG;
//   at once = merged && single && full0 && LOOKAHEAD != 1 && (LOOKAHEAD == 2 || !predict_boundary);
//   blocked = at once && the block rule gives >= 2 blocks;  split = at once && !blocked && K >= 2 && tiles <= 4096 &&
//   fuse_finalize == 0 && SPLIT_STREAMS > 0;  classic at once = !merged && single && !qf0 && inner > 0 && LOOKAHEAD == 2.
static TcgPlanIn defaults() {
  TcgPlanIn in;
  in.rtr = true;
  in.single = true;
  in.exact = false;
  in.tr_max_inner = 10;
  in.status = false;
  in.predict_boundary = true;
  in.fuse_finalize = 0;
  in.fuse_tcg = 0;
  in.first_step = 0;
  in.classic_tcg = 0;
  in.lookahead = 0;
  in.status_pass = 0;
  in.split_streams = 1;
  in.tail_fuse = 1;
  in.tcg_block = 2000;
  return in;
}

static void check_cg_flags(const TcgPlan& p) {
  EXPECT(p.qf0 && p.full0 && !p.spec && p.merged && p.tail_fuse && !p.fuse_tcg);
}

static void named_rows() {
  const Batch one = batch_of({5}), four = batch_of({2, 2, 2, 1});
  for (const Batch* B : {&one, &four}) {
    {  // Boundary: the first step alone (MODE_QF), the candidate queued speculatively behind it, grad(x1) not stored
      TcgPlanIn in = defaults();
      in.predict_boundary = true;
      const TcgPlan p = plan_for(in, *B);
      EXPECT(p.regime == TcgRegime::MergedOneAhead);
      EXPECT(p.qf0 && p.spec && !p.full0 && p.merged && p.tail_fuse);
      in.K = B->K;
      in.num_tiles = B->num_tiles();
      EXPECT(tcg_start_fused(in));
      EXPECT(!tcg_start_stores_grad(in));
      in.predict_boundary = false;
      EXPECT(tcg_start_stores_grad(in));
    }
    for (int pb = 0; pb < 2; ++pb) {  // Exact: the classic sequence, one ahead unless LOOKAHEAD = 2
      TcgPlanIn in = defaults();
      in.exact = true;
      in.predict_boundary = pb != 0;
      TcgPlan p = plan_for(in, *B);
      EXPECT(p.regime == TcgRegime::ClassicOneAhead);
      EXPECT(!p.qf0 && !p.merged && !p.spec && !p.full0 && !p.tail_fuse);
      in.lookahead = 2;
      p = plan_for(in, *B);
      EXPECT(p.regime == TcgRegime::ClassicAllAhead);
      EXPECT(!p.qf0 && !p.merged && !p.spec);
      in.K = B->K;
      in.num_tiles = B->num_tiles();
      EXPECT(!tcg_start_fused(in) && tcg_start_stores_grad(in));
    }
    {  // Multi-iteration RTR: the full first pass, one iteration ahead, nothing speculative
      TcgPlanIn in = defaults();
      in.single = false;
      in.predict_boundary = false;
      const TcgPlan p = plan_for(in, *B);
      EXPECT(p.regime == TcgRegime::MergedOneAhead);
      EXPECT(p.full0 && !p.spec && p.merged);
    }
  }
  {  // CG, small: 7 tiles fit one block of 2000 and are at most 4096, two agents or more: the split streams
    TcgPlanIn in = defaults();
    in.predict_boundary = false;
    const TcgPlan p = plan_for(in, four);
    EXPECT(p.regime == TcgRegime::MergedSplit);
    check_cg_flags(p);
  }
  {  // CG, TCG_BLOCK = 3: tiles {2, 2, 2, 1}: 2 + 2 > 3 closes a block after agents 0 and 1, 2 + 1 <= 3 keeps 2 and 3
    TcgPlanIn in = defaults();
    in.predict_boundary = false;
    in.tcg_block = 3;
    const TcgPlan p = plan_for(in, four);
    EXPECT(p.regime == TcgRegime::MergedBlocked);
    EXPECT((p.blocks == std::vector<int>{0, 1, 2, 4}));
    check_cg_flags(p);
  }
  {  // CG, K = 1: neither blocks nor groups for one agent
    TcgPlanIn in = defaults();
    in.predict_boundary = false;
    const TcgPlan p = plan_for(in, one);
    EXPECT(p.regime == TcgRegime::MergedAllAhead);
    check_cg_flags(p);
    in.tcg_block = 3;
    EXPECT(plan_for(in, one).regime == TcgRegime::MergedAllAhead);
  }
}

// ---- the block rule on the batches tests/test_gpu_tcg_block.py runs: 27 one-tile agents in colours of 14 and 13 -----
static std::vector<int> block_sizes(int K, int target) {
  const Batch B = batch_of(std::vector<int>(K, 1));
  std::vector<int> blocks, sizes;
  merged_blocks(B.K, B.num_tiles(), 0, target, B.tile_off.data(), &blocks);
  for (size_t i = 1; i < blocks.size(); ++i) sizes.push_back(blocks[i] - blocks[i - 1]);
  return sizes;
}

static void block_rule() {
  EXPECT((block_sizes(14, 4) == std::vector<int>{4, 4, 4, 2}));
  EXPECT((block_sizes(13, 4) == std::vector<int>{4, 4, 4, 1}));
  EXPECT((block_sizes(14, 3) == std::vector<int>{3, 3, 3, 3, 2}));
  EXPECT((block_sizes(13, 3) == std::vector<int>{3, 3, 3, 3, 1}));
  // off, one block, one agent, or a fused finalize: the unblocked queueing
  EXPECT(block_sizes(14, 0).empty());
  EXPECT(block_sizes(14, 14).empty());
  EXPECT(block_sizes(1, 0).empty());
  const Batch B = batch_of(std::vector<int>(14, 1));
  std::vector<int> blocks;
  merged_blocks(B.K, B.num_tiles(), 1, 4, B.tile_off.data(), &blocks);
  EXPECT(blocks.empty());
  // an agent larger than the target is a block of its own
  const Batch big = batch_of({1, 7, 1, 1});
  merged_blocks(big.K, big.num_tiles(), 0, 3, big.tile_off.data(), &blocks);
  EXPECT((blocks == std::vector<int>{0, 1, 2, 4}));
  // the split applies to two agents or more, at most 4096 tiles, no fused finalize, the key on
  EXPECT(merged_split(2, 4096, 0, 1));
  EXPECT(!merged_split(1, 5, 0, 1) && !merged_split(2, 4097, 0, 1) && !merged_split(2, 7, 1, 1) &&
         !merged_split(2, 7, 0, 0));
}

int main() {
  struct Case {
    const char* name;
    void (*run)();
  };
  static long combos = 0;
  const Case cases[] = {{"Invariants", [] { combos = enumerate(batch_of({5})) + enumerate(batch_of({2, 2, 2, 1})); }},
                        {"NamedRows", named_rows},
                        {"BlockRule", block_rule}};
  for (const Case& c : cases) {
    const int before = g_fail;
    c.run();
    std::printf("[%s] %s\n", g_fail == before ? "PASS" : "FAIL", c.name);
  }
  std::printf("%ld input combinations\n", combos);
  std::printf("%s\n", g_fail ? "SOME TESTS FAILED" : "ALL TESTS PASSED");
  return g_fail ? 1 : 0;
}

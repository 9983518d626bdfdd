// Host-side unit test of the int8 shared-prefix and beam-reorder launch plans in csrc/kernels/host_plan.h: a
// stand-alone program, built and run plain and with -fsanitize=address,undefined by tests/test_shared_prefix_q8_plans.py.
#include "host_plan.h"

#include <cstdio>

using namespace penroz;

static int fails = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                 \
    }                                                          \
  } while (0)

int main() {
  // production shapes: 64 rows on GPT-2 124M (12 MHA heads of 64) and Gemma-3 1B (4:1 GQA, head_dim 256) heads
  for (int64_t capP : {128, 1024, 4096}) {
    const SharedPrefixPlan g = plan_shared_prefix_q8(64, 12, 12, 64, capP), b = plan_shared_prefix(64, 12, 12, 64, capP);
    EXPECT(g.ok && g.tile_rows == b.tile_rows && g.tiles == b.tiles && g.splits == b.splits && g.grid == b.grid &&
           g.ws_floats == b.ws_floats);
    EXPECT(g.lds_bytes == 4 * 64 * 64 * 2 + 4 * 64 * 4);  // two stages of K and V tiles and of their scales
    const SharedPrefixPlan m = plan_shared_prefix_q8(64, 4, 1, 256, capP);
    EXPECT(m.ok && m.tile_rows == 128 && m.tiles == 2 && m.lds_bytes == 4 * 32 * 256 * 2 + 128 * 256 * 2 + 4 * 32 * 4);
  }
  // every admitted shape: LDS within a CU's 160 KiB and no smaller than either kind of workgroup needs
  for (int64_t D : {64, 128, 256})
    for (int64_t G : {1, 2, 4, 8})
      for (int64_t R : {2, 3, 33, 64}) {
        const SharedPrefixPlan p = plan_shared_prefix_q8(R, G * 2, 2, D, 300);
        EXPECT(p.ok && p.lds_bytes <= kCuLdsBytes && p.lds_bytes >= sp_q8_suffix_lds((int)D) &&
               p.lds_bytes >= sp_q8_prefix_lds((int)D, p.tile_rows));
        const SharedPrefixPrefillPlan f = plan_shared_prefix_prefill_q8(R, 33, G * 2, 2, D, 300, 64);
        const SharedPrefixPrefillPlan h = plan_shared_prefix_prefill(R, 33, G * 2, 2, D, 300, 64);
        EXPECT(f.ok && f.lds_bytes <= kCuLdsBytes && f.splits == h.splits && f.tiles == h.tiles && f.ws_floats == h.ws_floats);
        EXPECT(f.copy_wgs == (R * 33 * 2 * (D / 16) + 1023) / 1024 && f.grid == h.grid - h.copy_wgs + f.copy_wgs);
      }
  // degenerate and refused shapes are the bf16 plans'
  EXPECT(!plan_shared_prefix_q8(1, 4, 4, 64, 64).ok && !plan_shared_prefix_q8(65, 4, 4, 64, 64).ok);
  EXPECT(!plan_shared_prefix_q8(4, 4, 4, 96, 64).ok && !plan_shared_prefix_q8(4, 12, 4, 64, 64).ok);
  EXPECT(!plan_shared_prefix_q8(4, 4, 0, 64, 64).ok && !plan_shared_prefix_q8(4, 4, 4, 64, 0).ok);
  EXPECT(plan_shared_prefix_q8(2, 1, 1, 64, 1).splits == 1 && plan_shared_prefix_q8(2, 1, 1, 64, 1, 99).splits == kSharedPrefixMaxSplits);
  EXPECT(!plan_shared_prefix_prefill_q8(4, 0, 4, 4, 64, 64, 64).ok && !plan_shared_prefix_prefill_q8(4, 65, 4, 4, 64, 64, 64).ok);
  EXPECT(plan_shared_prefix_prefill_q8(2, 1, 1, 1, 64, 1, 1).copy_wgs == 1);
  // beam_reorder over bytes: int8 planes move in 16-B units, scale planes in 4-B units
  EXPECT(plan_beam_reorder_bytes(2, 64, 64).pieces == 1 && plan_beam_reorder_bytes(2, 64, 64).workgroups == 4);
  EXPECT(plan_beam_reorder_bytes(1, 65, 256).pieces == 5);  // 16640 B in 4-KiB pieces
  EXPECT(plan_beam_reorder_bytes(3, 70, 4).pieces == 1 && plan_beam_reorder_bytes(3, 257, 4).pieces == 2);
  EXPECT(plan_beam_reorder_bytes(3, 257, 4).workgroups == 12);
  std::printf(fails ? "shared_prefix_q8_plan_test: %d failure(s)\n" : "shared_prefix_q8_plan_test: ok\n", fails);
  return fails ? 1 : 0;
}

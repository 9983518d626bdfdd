// Host-side unit test of plan_logit_bias (csrc/kernels/host_plan.h), built and run by
// tests/test_logit_bias_plan.py with -fsanitize=address,undefined (any report aborts the run). It
// also walks the launch's index arithmetic — the functions of host_plan.h that the kernel itself calls —
// on the host over a byte per logit and a word array of exactly the planned size: every workgroup's
// reads stay inside the mask, every write inside its row, the mask parts cover every token of every row exactly once and nothing beyond V.
#include "host_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      ++fails;                                                      \
    }                                                               \
  } while (0)

using namespace penroz;

static void test_plan() {
  const int64_t lim = int64_t(1) << 31;
  LogitBiasPlan p = plan_logit_bias(1, 8, false);
  EXPECT(p.per_row == 1 && p.grid == 1 && p.mask_words == 1);
  p = plan_logit_bias(64, 262144, false);
  EXPECT(p.per_row == 1 && p.grid == 64 && p.mask_words == 8192);
  p = plan_logit_bias(64, 262144, true);
  EXPECT(p.per_row == 1 + 128 && p.grid == 64 * 129 && p.mask_words == 8192);
  p = plan_logit_bias(3, 50257, true);
  EXPECT(p.per_row == 1 + 25 && p.grid == 78 && p.mask_words == 1571);
  for (int64_t V : {int64_t(1), int64_t(31), int64_t(32), int64_t(33), int64_t(kBiasSpan - 1), int64_t(kBiasSpan),
                    int64_t(kBiasSpan + 1), lim - 1}) {
    p = plan_logit_bias(1, V, true);
    EXPECT(p.per_row >= 2 && (int64_t)(p.per_row - 1) * kBiasSpan >= V && (int64_t)(p.per_row - 2) * kBiasSpan < V);
    EXPECT(p.mask_words * 32 >= V && (p.mask_words - 1) * 32 < V && p.grid == p.per_row);
  }
  // refused: no rows, no vocabulary, V of 2^31 or more, a grid of 2^31 or more
  for (bool mask : {false, true}) {
    EXPECT(plan_logit_bias(0, 8, mask).grid == 0 && plan_logit_bias(-1, 8, mask).grid == 0);
    EXPECT(plan_logit_bias(1, 0, mask).grid == 0 && plan_logit_bias(1, -5, mask).grid == 0);
    EXPECT(plan_logit_bias(1, lim, mask).grid == 0 && plan_logit_bias(1, INT64_MAX, mask).grid == 0);
    EXPECT(plan_logit_bias(INT64_MAX, lim - 1, mask).grid == 0 && plan_logit_bias(lim, 8, mask).grid == 0);
  }
  EXPECT(plan_logit_bias(lim - 1, 8, false).grid == lim - 1 && plan_logit_bias(lim - 1, 8, true).grid == 0);
  p = plan_logit_bias(lim / 2, 8, true);  // 2 workgroups per row: 2^31 in all
  EXPECT(p.grid == 0 && p.per_row == 0 && p.mask_words == 0);
  p = plan_logit_bias(lim / 2 - 1, 8, true);
  EXPECT(p.grid == lim - 2 && p.per_row == 2);
}

// every workgroup, thread and round of the mask form, through the kernel's own index functions
static void walk(int64_t B, int64_t V) {
  const LogitBiasPlan p = plan_logit_bias(B, V, true);
  EXPECT(p.grid == B * p.per_row);
  std::vector<unsigned char> hit((size_t)(B * V), 0);
  std::vector<unsigned> allow((size_t)p.mask_words, 0u);  // nothing allowed: every token is written
  for (int64_t wg = 0; wg < p.grid; ++wg) {
    const int64_t row = bias_row_of(wg, p.per_row);
    const int part = bias_part_of(wg, p.per_row);
    EXPECT(row >= 0 && row < B);
    if (part == 0) continue;
    for (int tid = 0; tid < kBiasThreads; ++tid)
      for (int k = 0; k < kBiasMaskRounds; ++k) {
        const int64_t v = bias_mask_token(part, tid, k);
        EXPECT(v >= 0);
        if (v >= V) continue;
        const unsigned w = allow.at((size_t)bias_mask_word(v));
        if (!bias_allowed(w, v)) ++hit.at((size_t)(row * V + v));
      }
  }
  for (unsigned char h : hit) EXPECT(h == 1);
}

int main() {
  test_plan();
  for (int64_t V : {1, 8, 31, 32, 33, 2047, 2048, 2049, 50257}) walk(V > 4096 ? 2 : 3, V);
  if (fails) {
    std::printf("logit_bias_plan_test: %d failure(s)\n", fails);
    return 1;
  }
  std::printf("logit_bias_plan_test: ok\n");
  return 0;
}

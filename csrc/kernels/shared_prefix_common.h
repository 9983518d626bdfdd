// What the bf16 and the int8 shared-prefix attention kernels (shared_prefix_attn.hip,
// shared_prefix_attn_q8.hip) share: the partials' constants and launch 2, which folds them. Both forms
// write the same fp32 partials (o[D], m, l) per (row, head) into [S + 1, R, H, ·], so one merge serves both.
#pragma once
#include "attn_common.h"

namespace penroz {
namespace {

typedef uint32_t sp_u32x4 __attribute__((ext_vector_type(4)));

constexpr float kSpFloor = -1e30f;  // running maximum before any key (finite: exp2(floor − m) is 0, never NaN)
constexpr int kSpGroup = 8;         // largest query group H / Hkv

__device__ __forceinline__ int sp_swz(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }

// ---- launch 2: fold the np partials of every (row, head) in index order; thread = 4 output columns -----
__global__ void __launch_bounds__(256) shared_prefix_merge_kernel(const float* __restrict__ ws_o,
                                                                  const float* __restrict__ ws_ml,
                                                                  bf16* __restrict__ out, int rows, int D, int np) {
  const int64_t i4 = blockIdx.x * (int64_t)256 + threadIdx.x;
  const int dq = D / 4;
  if (i4 >= (int64_t)rows * dq) return;
  const int64_t r = i4 / dq;
  const int d = (int)(i4 - r * dq) * 4;
  float M = kSpFloor;
  for (int s = 0; s < np; ++s) M = fmaxf(M, ws_ml[2 * ((int64_t)s * rows + r)]);
  float L = 0.f;
  float4_t O = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < np; ++s) {
    const int64_t rr = (int64_t)s * rows + r;
    const float f = fexp2(ws_ml[2 * rr] - M);  // an empty range: exp2(floor − M) = 0
    L += ws_ml[2 * rr + 1] * f;
    const float4_t po = *reinterpret_cast<const float4_t*>(ws_o + rr * D + d);
    O[0] += po[0] * f;
    O[1] += po[1] * f;
    O[2] += po[2] * f;
    O[3] += po[3] * f;
  }
  const float inv = L > 0.f ? 1.f / L : 0.f;
  store4(out + r * D + d, O[0] * inv, O[1] * inv, O[2] * inv, O[3] * inv);
}

}  // namespace
}  // namespace penroz

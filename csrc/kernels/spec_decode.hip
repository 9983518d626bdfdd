// Prompt-lookup speculative decoding, the last kernel of a speculative decode step (definition:
// ops/speculative.py; the step: models/graph_decode.py, GraphDecoder(speculate=k)).
//
// A step runs R = k + 1 <= 4 rows, consecutive positions of ONE sequence: row 0 is fed the last known
// token, row i >= 1 the draft token i - 1. State, all static device buffers, so one captured graph
// serves every history and every limit:
//   hist       int32 [cap]   the sequence so far (prompt and emitted tokens), n of them in use
//   n_t        int32 [1]     n
//   cand       int64 [R]     this step's greedy choice per row (the sampler's output)
//   idx        int64 [R, 1]  the step's input: row 0 = hist[n - 1], rows 1..k = the draft
//   pos_t      int64 [R]     the rows' positions and cache slots, n - 1 + i
//   len_t      int64 [1]     the cache length the attention reads, n + k
//   emitted_t  int32 [1]     tokens emitted since the host set the state
//   limit_t    int32 [1]     ... and how many are wanted
//   steps_t    int32 [1]     steps that emitted
//   accepted_t int32 [1]     draft tokens confirmed and emitted
//
// spec_advance: with a the number of leading drafts idx[1 + i] == cand[i], emits
// e = min(a + 1, limit - emitted, cap - k - n) tokens of cand into hist[n ..] (the last bound keeps
// the next step's rows inside the cache); e <= 0 is a frozen step and writes nothing at all. Then the
// draft for the next step: the longest suffix of hist, m = min(3, n - 1) down to 1 tokens, that occurs
// earlier (a start j in 0 .. n - m - 1), its latest occurrence; the k tokens behind it, continued
// through the draft itself; without a match k copies of the last token. Every thread scans starts
// strided over hist and keeps the largest key (m, j); the keys are reduced through the wave and LDS;
// one lane builds the draft and writes idx, pos_t and len_t. draft_only: the second half alone, which
// the host runs once, eagerly, when it sets the state.
// One workgroup. Integers only, no atomics, plain vector stores: exactly reproducible.
#include "common.h"
#include "launch_args.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {

constexpr int kSpecThreads = 256;
constexpr int kSpecMaxK = 3;
constexpr int kSpecMaxNgram = 3;
constexpr int kSpecJBits = 26;  // key = m << kSpecJBits | j: histories up to 2^26 tokens

__global__ __launch_bounds__(kSpecThreads) void spec_advance_kernel(int* hist, int cap, int* n_t, const int64_t* cand,
                                                                    int64_t* idx, int64_t* pos_t, int64_t* len_t,
                                                                    int* emitted_t, const int* __restrict__ limit_t,
                                                                    int* steps_t, int* accepted_t, int k,
                                                                    int draft_only) {
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  __shared__ int red[kSpecThreads / 64];
  int n = n_t[0];
  PZ_DEVICE_CHECK(n >= 1 && n + k <= cap);
  if (n < 1 || n + k > cap) return;  // (uniform) the rows would leave the cache: frozen, as e <= 0 below
  if (!draft_only) {
    const int emitted = emitted_t[0], limit = limit_t[0];
    // every thread reads the step's drafts and choices before any of them is overwritten
    int64_t c[kSpecMaxK + 1], d[kSpecMaxK];
#pragma unroll
    for (int i = 0; i <= kSpecMaxK; ++i) c[i] = i <= k ? cand[i] : 0;
#pragma unroll
    for (int i = 0; i < kSpecMaxK; ++i) d[i] = i < k ? idx[1 + i] : -1;
    int a = 0;
#pragma unroll
    for (int i = 0; i < kSpecMaxK; ++i)
      if (a == i && i < k && d[i] == c[i]) a = i + 1;
    const int e = min(min(a + 1, limit - emitted), cap - k - n);
    if (e <= 0) return;  // (uniform) frozen: nothing is written
#pragma unroll
    for (int i = 0; i <= kSpecMaxK; ++i)
      if (t == i && i < e) hist[n + i] = (int)c[i];
    __syncthreads();  // the emitted tokens are visible to the scan; every read of n_t lies before its store
    n += e;
    if (t == 0) {
      n_t[0] = n;
      emitted_t[0] = emitted + e;
      steps_t[0] += 1;
      accepted_t[0] += e - 1;
    }
  }
  // the draft: the largest (m, j) over the starts this thread scans
  const int mmax = min(kSpecMaxNgram, n - 1);
  int tail[kSpecMaxNgram];  // tail[x] = hist[n - 1 - x]
#pragma unroll
  for (int x = 0; x < kSpecMaxNgram; ++x) tail[x] = x < mmax ? hist[n - 1 - x] : -1;
  int best = -1;
  for (int j = t; j + 1 < n; j += kSpecThreads) {
#pragma unroll
    for (int m = 1; m <= kSpecMaxNgram; ++m) {
      if (m > mmax || j + m > n - 1) continue;  // start j of an m-gram that ends before the suffix's last token
      bool hit = true;
#pragma unroll
      for (int x = 0; x < m; ++x) hit = hit && hist[j + m - 1 - x] == tail[x];
      if (hit) best = max(best, (m << kSpecJBits) | j);
    }
  }
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
  if (lane == 0) red[wid] = best;
  __syncthreads();
  if (t != 0) return;
#pragma unroll
  for (int w = 0; w < kSpecThreads / 64; ++w) best = max(best, red[w]);
  const int last = hist[n - 1];
  int dr[kSpecMaxK];
#pragma unroll
  for (int i = 0; i < kSpecMaxK; ++i) {
    if (best < 0) {
      dr[i] = last;
    } else {
      const int p = (best & ((1 << kSpecJBits) - 1)) + (best >> kSpecJBits) + i;  // j + m + i <= n - 1 + i
      int v = p < n ? hist[p] : last;
#pragma unroll
      for (int x = 0; x < kSpecMaxK; ++x)
        if (x < i && p - n == x) v = dr[x];  // the draft continues through itself
      dr[i] = v;
    }
  }
  idx[0] = last;
  pos_t[0] = n - 1;
#pragma unroll
  for (int i = 0; i < kSpecMaxK; ++i) {
    if (i < k) {
      idx[1 + i] = dr[i];
      pos_t[1 + i] = n + i;
    }
  }
  len_t[0] = n + k;
}

}  // namespace penroz

using namespace penroz;

// See the head of this file. draft_only: cand is not read (any int64 [R] tensor, idx itself will do).
void spec_advance(torch::Tensor hist, torch::Tensor n_t, torch::Tensor cand, torch::Tensor idx, torch::Tensor pos_t,
                  torch::Tensor len_t, torch::Tensor emitted_t, torch::Tensor limit_t, torch::Tensor steps_t,
                  torch::Tensor accepted_t, int64_t k, bool draft_only) {
  const char* who = "spec_advance";
  TORCH_CHECK(k >= 1 && k <= kSpecMaxK, who, ": k must be in [1, ", kSpecMaxK, "], got ", k);
  const int64_t R = k + 1;
  la_one_device(who, hist, {n_t, cand, idx, pos_t, len_t, emitted_t, limit_t, steps_t, accepted_t});
  TORCH_CHECK(hist.dim() == 1 && hist.size(0) > k && hist.size(0) <= (int64_t(1) << kSpecJBits), who,
              ": hist must be int32 [k < cap <= 2^", kSpecJBits, "]");
  const int64_t cap = hist.size(0);
  int* hp = la_i32_shape(who, "hist", hist, {cap});
  int* np = la_i32_shape(who, "n_t", n_t, {1});
  int* ep = la_i32_shape(who, "emitted_t", emitted_t, {1});
  const int* lp = la_i32_shape(who, "limit_t", limit_t, {1});
  int* sp = la_i32_shape(who, "steps_t", steps_t, {1});
  int* ap = la_i32_shape(who, "accepted_t", accepted_t, {1});
  for (const auto* t : {&cand, &idx})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kInt64 && t->is_contiguous() && t->numel() == R &&
                    (t->dim() == 1 || (t->dim() == 2 && t->size(0) == R)),
                who, ": cand and idx must be contiguous int64 [R = k + 1] or [R, 1]");
  TORCH_CHECK(pos_t.is_cuda() && pos_t.scalar_type() == torch::kInt64 && pos_t.is_contiguous() && pos_t.dim() == 1 &&
                  pos_t.numel() == R, who, ": pos_t must be contiguous int64 [R = k + 1]");
  int64_t* ltp = la_i64_scalar(who, "len_t", len_t);
  hipLaunchKernelGGL(spec_advance_kernel, dim3(1), dim3(kSpecThreads), 0, at::hip::getCurrentHIPStream(), hp, (int)cap,
                     np, cand.data_ptr<int64_t>(), idx.data_ptr<int64_t>(), pos_t.data_ptr<int64_t>(), ltp, ep, lp, sp, ap,
                     (int)k, (int)draft_only);
}

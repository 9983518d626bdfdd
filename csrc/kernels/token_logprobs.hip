// Per-token log-probabilities of a decode step (definition: ops/logprobs.py). For row b with the
// logits x the sampler received and the token t it chose:
//   lse = log Σ_v exp(x_v),  lp = x_t - lse,  top(n) = the n largest x_v as (v, x_v - lse),
//   ordered by x_v descending and, among equal logits, by v ascending.
// Two launches, shaped like the two-stage sampler (sampling.hip); stream order between them is the
// only synchronisation (no arrival counters, no float atomics: results are bitwise reproducible).
//
// logprob_part_kernel   grid (P, B), 256 threads: part p covers logits [4096 p, 4096 (p + 1)) of a
//   row, 16 per thread (two 8-element chunks) plus one ragged element. A row of odd V starts at any
//   element, so the part reads single elements up to the first 16-B boundary and after the last whole
//   chunk, and 16-B vectors in between; every load is issued before the first use. It writes the
//   part's maximum m_p, s_p = Σ exp(x - m_p) (per thread, then a fixed tree) and, for n > 0, its n
//   best candidates in the definition's order.
// logprob_merge_kernel  one workgroup per row: m = max m_p, s = Σ s_p exp(m_p - m) (a fixed tree
//   over the parts), lse = m + log s; x_t by one load from the row; the n best of the P n candidates.
//
// Candidates are 64-bit keys, unique per element: the sampler's order-preserving map of the fp32
// value in the high word, ~v in the low word — a larger key is a larger logit or, at equal logits, a
// smaller index. Selection is n rounds of a workgroup-wide maximum (DPP within the wave, LDS across
// the four waves), the winner retired each round; 0 is no key (it would be index 2^32 - 1).
//
// n comes from a device int32 [1] and the token from a device tensor, so a captured step replays
// with another n; every loop bound on n is a run-time value capped by kLogprobMaxN.
//
// Workspace per row, in floats (plan_logprobs, host_plan.h): m [P], s [P], keys uint64 [P, 20].
#include "common.h"
#include "launch_args.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {

constexpr int kLpThreads = 256;

__device__ __forceinline__ uint32_t lp_order_key(float f) {  // (sampling.hip order_key)
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float lp_key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ uint64_t lp_key(float x, int v) {
  return ((uint64_t)lp_order_key(x) << 32) | (uint32_t)~(uint32_t)v;
}

template <int CTRL>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// maximum over the wave (all 64 lanes active; every lane gets it): common.h wave_reduce on 64 bits
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  v = max_u64(v, dpp_u64<0xB1>(v));
  v = max_u64(v, dpp_u64<0x4E>(v));
  v = max_u64(v, dpp_u64<0x124>(v));
  v = max_u64(v, dpp_u64<0x128>(v));
  return max_u64(max_u64(lane_u64(v, 0), lane_u64(v, 16)), max_u64(lane_u64(v, 32), lane_u64(v, 48)));
}

// maximum over the workgroup's four waves; red: 2 x 4 LDS words, alternated by the caller's round
// so one barrier per round is enough (round r + 2 rewrites what every thread read before the
// barrier of round r + 1). Every thread calls it.
__device__ __forceinline__ uint64_t block_max_u64(uint64_t v, uint64_t (*red)[4], int round) {
  v = wave_max_u64(v);
  uint64_t* r = red[round & 1];
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  return max_u64(max_u64(r[0], r[1]), max_u64(r[2], r[3]));
}

__device__ __forceinline__ int lp_read_n(const int* n_dev) { return min(max(*n_dev, 0), kLogprobMaxN); }

template <typename T>
__global__ void __launch_bounds__(kLpThreads) logprob_part_kernel(const T* __restrict__ logits, int V, int P,
                                                                  const int* __restrict__ n_dev,
                                                                  float* __restrict__ ws, int64_t ws_row) {
  __shared__ float fred[2][4];
  __shared__ uint64_t kred[2][4];
  const int part = blockIdx.x, row = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int base = part * kLogprobPartN;
  const int len = min(kLogprobPartN, V - base);  // >= 1: the grid has ceil(V / 4096) parts
  const T* pp = logits + (size_t)row * V + base;
  // [0, head): single elements up to the first 16-B boundary; then nch chunks of 8; then the tail
  constexpr int kPer16 = 16 / (int)sizeof(T);
  const int mis = (int)((reinterpret_cast<uintptr_t>(pp) & 15u) / sizeof(T));
  const int head = min(len, mis ? kPer16 - mis : 0);
  const int nch = (len - head) / 8;
  const int tail0 = head + nch * 8;
  const int rag = head + (len - tail0);  // <= 7 + 7 single elements, one per thread

  float v[2][8];
  bool ok[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int j = t + kLpThreads * c;
    ok[c] = j < nch;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[c][e] = -INFINITY;
    if (ok[c]) Vec8<T>::load(pp + head + 8 * j, v[c]);
  }
  const int ri = t < head ? t : tail0 + (t - head);
  float r = -INFINITY;
  if (t < rag) r = to_f<T>(pp[ri]);

  float tm = r;
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) tm = fmaxf(tm, v[c][e]);
  tm = wave_max(tm);
  if (lane == 0) fred[0][w] = tm;
  __syncthreads();
  const float m = fmaxf(fmaxf(fred[0][0], fred[0][1]), fmaxf(fred[0][2], fred[0][3]));
  float ts = expf(r - m);  // an absent element is -inf: it adds exp(-inf) = 0
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) ts += expf(v[c][e] - m);
  ts = wave_sum(ts);
  if (lane == 0) fred[1][w] = ts;
  __syncthreads();
  float* wr = ws + (size_t)row * ws_row;
  if (t == 0) {
    wr[part] = m;
    wr[P + part] = (fred[1][0] + fred[1][1]) + (fred[1][2] + fred[1][3]);
  }

  const int n = lp_read_n(n_dev);
  if (n == 0) return;
  uint64_t key[17];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      key[8 * c + e] = ok[c] ? lp_key(v[c][e], base + head + 8 * (t + kLpThreads * c) + e) : 0;
  key[16] = t < rag ? lp_key(r, base + ri) : 0;
  uint64_t mine = 0, out = 0;
#pragma unroll
  for (int i = 0; i < 17; ++i) mine = max_u64(mine, key[i]);
  for (int round = 0; round < n; ++round) {
    const uint64_t win = block_max_u64(mine, kred, round);
    if (t == round) out = win;
    if (mine == win && win != 0) {  // keys are unique: one thread retires its best and finds its next
      mine = 0;
#pragma unroll
      for (int i = 0; i < 17; ++i) {
        if (key[i] == win) key[i] = 0;
        mine = max_u64(mine, key[i]);
      }
    }
  }
  // slot j < n of this part: its j-th best, 0 once the part has run out of elements
  uint64_t* keys = reinterpret_cast<uint64_t*>(wr + 2 * (size_t)P) + (size_t)part * kLogprobMaxN;
  if (t < n) keys[t] = out;
}

// tok int64 [B]; step: nullptr (column 0 of cap = 1) or the burst's step counter, already advanced:
// the column written is *step - 1. lp_out [B, cap], id_out / tlp_out [B, cap, kLogprobMaxN]; slots
// from n (or from the number of logits) on get id -1 and -inf.
template <typename T>
__global__ void __launch_bounds__(kLpThreads) logprob_merge_kernel(const T* __restrict__ logits, int V, int P,
                                                                   const int* __restrict__ n_dev,
                                                                   const int64_t* __restrict__ tok,
                                                                   const int64_t* __restrict__ step,
                                                                   const float* __restrict__ ws, int64_t ws_row,
                                                                   float* __restrict__ lp_out, int* __restrict__ id_out,
                                                                   float* __restrict__ tlp_out, int64_t cap) {
  __shared__ float fred[2][4];
  __shared__ uint64_t kred[2][4];
  const int row = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t col = step ? *step - 1 : 0;
  PZ_DEVICE_CHECK(col >= 0 && col < cap);
  if (col < 0 || col >= cap) return;  // (uniform: nothing is written outside the burst buffers)
  const float* wr = ws + (size_t)row * ws_row;
  const bool has = t < P;  // P <= 256: one part per thread
  const float mp = has ? wr[t] : -INFINITY;
  const float sp = has ? wr[P + t] : 0.f;
  const int n = lp_read_n(n_dev);
  const uint64_t* keys = reinterpret_cast<const uint64_t*>(wr + 2 * (size_t)P) + (size_t)t * kLogprobMaxN;
  uint64_t k[kLogprobMaxN];  // this part's candidates, best first
#pragma unroll
  for (int j = 0; j < kLogprobMaxN; ++j) k[j] = (has && j < n) ? keys[j] : 0;
  const int64_t tk = tok[row];
  PZ_DEVICE_CHECK(tk >= 0 && tk < V);
  float xt = __builtin_nanf("");
  if (t == 0 && tk >= 0 && tk < V) xt = to_f<T>(logits[(size_t)row * V + tk]);

  const float wm = wave_max(mp);
  if (lane == 0) fred[0][w] = wm;
  __syncthreads();
  const float m = fmaxf(fmaxf(fred[0][0], fred[0][1]), fmaxf(fred[0][2], fred[0][3]));
  const float term = has ? sp * expf(mp - m) : 0.f;
  const float wsum = wave_sum(term);
  if (lane == 0) fred[1][w] = wsum;
  __syncthreads();
  const float lse = m + logf((fred[1][0] + fred[1][1]) + (fred[1][2] + fred[1][3]));
  const size_t o = (size_t)row * cap + col;
  if (t == 0) lp_out[o] = xt - lse;

  uint64_t out = 0;
  for (int round = 0; round < n; ++round) {
    const uint64_t win = block_max_u64(k[0], kred, round);
    if (t == round) out = win;
    if (k[0] == win && win != 0) {
#pragma unroll
      for (int j = 0; j + 1 < kLogprobMaxN; ++j) k[j] = k[j + 1];
      k[kLogprobMaxN - 1] = 0;
    }
  }
  if (t < kLogprobMaxN) {
    const bool used = t < n && out != 0;
    id_out[o * kLogprobMaxN + t] = used ? (int)~(uint32_t)out : -1;
    tlp_out[o * kLogprobMaxN + t] = used ? lp_key_value((uint32_t)(out >> 32)) - lse : -INFINITY;
  }
}

struct LogprobOut {
  float* lp;
  int* id;
  float* tlp;
  int64_t cap;
};

// Checks logits / tok / n_t / workspace, then the two launches. The output pointers are the entry
// point's to check; `rest` lists every other operand for the one-device check.
static void launch_logprobs(const char* who, const torch::Tensor& logits, const torch::Tensor& tok,
                            const torch::Tensor& n_t, const int64_t* step, const torch::Tensor& workspace,
                            const LogprobOut& out, std::initializer_list<OptTensor> rest) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2 && logits.size(0) >= 1 &&
                  logits.size(1) >= 1, who, ": contiguous device logits [B >= 1, V >= 1]");
  const int64_t B = logits.size(0), V = logits.size(1);
  la_one_device(who, logits, rest);
  la_one_device(who, logits, {tok, n_t, workspace});
  const LogprobPlan p = plan_logprobs(V);
  TORCH_CHECK(p.parts > 0, who, ": V = ", V, " is above the ", (int64_t)kLogprobMaxParts * kLogprobPartN, " logits supported");
  TORCH_CHECK(B <= 65535, who, ": at most 65535 rows");
  TORCH_CHECK(tok.scalar_type() == torch::kInt64 && tok.is_contiguous() && tok.numel() == B, who,
              ": tokens must be contiguous int64 [B = ", B, "]");
  TORCH_CHECK(n_t.scalar_type() == torch::kInt32 && n_t.numel() == 1, who, ": n must be a device int32 [1]");
  TORCH_CHECK(workspace.scalar_type() == torch::kFloat32 && workspace.is_contiguous() &&
                  workspace.numel() >= B * p.ws_floats && la_aligned(workspace, 8),
              who, ": workspace must be contiguous 8-B aligned fp32 of at least ", B * p.ws_floats, " (", B, " x ",
              p.ws_floats, ")");
  auto stream = at::hip::getCurrentHIPStream();
  la_by_elem(who, logits.scalar_type(), [&](auto tag) {
    using T = decltype(tag);
    const T* lg = reinterpret_cast<const T*>(logits.data_ptr());
    hipLaunchKernelGGL(logprob_part_kernel<T>, dim3(p.parts, (unsigned)B), dim3(kLpThreads), 0, stream, lg, (int)V,
                       p.parts, n_t.data_ptr<int>(), workspace.data_ptr<float>(), p.ws_floats);
    hipLaunchKernelGGL(logprob_merge_kernel<T>, dim3((unsigned)B), dim3(kLpThreads), 0, stream, lg, (int)V, p.parts,
                       n_t.data_ptr<int>(), tok.data_ptr<int64_t>(), step, workspace.data_ptr<float>(), p.ws_floats,
                       out.lp, out.id, out.tlp, out.cap);
  });
}

}  // namespace penroz

using namespace penroz;

// The launch plan (host_plan.h): (parts per row, workspace floats per row) (host only)
std::tuple<int64_t, int64_t> token_logprobs_plan(int64_t V) {
  const LogprobPlan p = plan_logprobs(V);
  TORCH_CHECK(p.parts > 0, "token_logprobs_plan: 1 <= V <= ", (int64_t)kLogprobMaxParts * kLogprobPartN, ", got ", V);
  return {p.parts, p.ws_floats};
}

// Eager steps: (lp fp32 [B], top_id int64 [B, min(n, V)], top_lp fp32 [B, min(n, V)]) of
// logits [B, V] (bf16 / fp16 / fp32) and tokens int64 [B] or [B, 1].
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> token_logprobs(torch::Tensor logits, torch::Tensor tokens,
                                                                       int64_t n) {
  const char* who = "token_logprobs";
  TORCH_CHECK(n >= 0 && n <= kLogprobMaxN, who, ": n must be in [0, ", kLogprobMaxN, "], got ", n);
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, who, ": device logits [B, V]");
  const int64_t B = logits.size(0), V = logits.size(1);
  const LogprobPlan p = plan_logprobs(V);
  auto f32 = logits.options().dtype(torch::kFloat32), i32 = logits.options().dtype(torch::kInt32);
  auto lp = torch::empty({B}, f32);
  auto id = torch::empty({B, kLogprobMaxN}, i32);
  auto tlp = torch::empty({B, kLogprobMaxN}, f32);
  auto ws = torch::empty({B * std::max<int64_t>(p.ws_floats, 1)}, f32);
  auto n_t = torch::full({1}, n, i32);
  launch_logprobs(who, logits, tokens, n_t, nullptr, ws, {lp.data_ptr<float>(), id.data_ptr<int>(), tlp.data_ptr<float>(), 1},
                  {});
  const int64_t k = std::min(n, V);
  return {lp, id.slice(1, 0, k).to(torch::kInt64), tlp.slice(1, 0, k).contiguous()};
}

// Graph-replayed decode, after the sampler and the counter advance: row r's token idx[r], its
// log-probability -> lp_buf[r, *step - 1], the n_t[0] best -> top_id_buf / top_lp_buf[r, *step - 1, :].
void token_logprobs_step(torch::Tensor logits, torch::Tensor idx, torch::Tensor step, torch::Tensor n_t,
                         torch::Tensor lp_buf, torch::Tensor top_id_buf, torch::Tensor top_lp_buf,
                         torch::Tensor workspace) {
  const char* who = "token_logprobs_step";
  TORCH_CHECK(logits.dim() == 2, who, ": logits [B, V]");
  const int64_t B = logits.size(0);
  TORCH_CHECK(lp_buf.dim() == 2 && lp_buf.size(0) == B && lp_buf.size(1) >= 1, who, ": lp_buf must be [B = ", B, ", cap >= 1]");
  const int64_t cap = lp_buf.size(1);
  float* lp = la_f32_shape(who, "lp_buf", lp_buf, {B, cap});
  float* tlp = la_f32_shape(who, "top_lp_buf", top_lp_buf, {B, cap, kLogprobMaxN});
  TORCH_CHECK(top_id_buf.is_cuda() && top_id_buf.scalar_type() == torch::kInt32 && top_id_buf.is_contiguous() &&
                  top_id_buf.sizes() == at::IntArrayRef({B, cap, kLogprobMaxN}),
              who, ": int32 contiguous top_id_buf [", B, ", ", cap, ", ", kLogprobMaxN, "]");
  launch_logprobs(who, logits, idx, n_t, la_i64_scalar(who, "step", step), workspace,
                  {lp, top_id_buf.data_ptr<int>(), tlp, cap}, {step, lp_buf, top_id_buf, top_lp_buf});
}

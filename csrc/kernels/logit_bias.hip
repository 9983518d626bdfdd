// Logit bias, banned and allowed tokens and min_tokens on the logits of a decode step, between the
// penalties and the sampler (definition: ops/logit_bias.py).
//
// The canonical form, shared by all rows and read on the device, so other values, another allowed set
// and another min_tokens replay the same captured graph:
//   ids       int32 [1024]          the entries' token ids, ascending, each id once
//   bias      fp32  [1024]          what is added to the logit; -inf: the token is banned
//   until     int32 [1024]          the entry means FLOOR while t < until (an end token under min_tokens)
//   n_entries int32 [1]             how many are in use
//   allow     int32 [ceil(V / 32)]  bit v % 32 of word v / 32 set: token v is allowed (mask form only)
//   base_t, step_t int64 [1]        t = *base_t + *step_t: the index, in the generate call, of the token
//                                   about to be sampled (step_t absent: an eager step, t = *base_t)
// FLOOR is finite on purpose (ops/logit_bias.py): -2^100 for bf16 and fp32 logits, -2^15 for fp16.
//
// logit_bias_apply is one launch of 256-thread workgroups, 1 + parts per row (host_plan.h):
//   part 0         walks the entries, four per thread, every load of id / bias / until issued before the
//                  first use; each entry rewrites exactly one logit with a single-element load and store
//                  (rows of odd V have no vector alignment): FLOOR, or the fp32 sum rounded once.
//   parts 1 ...    (mask form only) each covers 2048 consecutive tokens: FLOOR is stored where the bit is
//                  clear. Pure stores, no read of the logits; consecutive lanes take consecutive tokens,
//                  so a wave's stores coalesce; the tokens beyond V and the bits of the last word beyond
//                  V are never touched.
// No logit has two writers: the mask parts write only tokens whose bit is clear, part 0 skips an entry
// whose bit is clear (the canonical form holds none), and the ids are distinct. No atomics, nothing
// shared between workgroups; bit-identical to ops/logit_bias.py reference_bias.
#include "common.h"
#include "launch_args.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {

static_assert(kBiasMaxEntries % kBiasThreads == 0 && kBiasSpan % kBiasThreads == 0, "whole rounds of the workgroup");
constexpr int kBiasPerThread = kBiasMaxEntries / kBiasThreads;  // entries a thread holds

template <typename T> __device__ __forceinline__ float bias_floor() { return -0x1p100f; }
template <> __device__ __forceinline__ float bias_floor<__half>() { return -32768.f; }

template <typename T>
__global__ __launch_bounds__(kBiasThreads) void logit_bias_kernel(T* logits, const int* __restrict__ ids,
                                                                  const float* __restrict__ bias,
                                                                  const int* __restrict__ until,
                                                                  const int* __restrict__ n_entries,
                                                                  const unsigned* __restrict__ allow,
                                                                  const int64_t* __restrict__ base_t,
                                                                  const int64_t* __restrict__ step_t, int V,
                                                                  int per_row) {
  const int64_t row = bias_row_of(blockIdx.x, per_row);
  const int part = bias_part_of(blockIdx.x, per_row);
  T* x = logits + (size_t)row * V;
  const T floor_v = from_f<T>(bias_floor<T>());
  if (part > 0) {
    // the allowed mask over tokens [base, base + kBiasSpan): the words first, then the stores
    PZ_DEVICE_CHECK(allow != nullptr);
    unsigned w[kBiasMaskRounds];
#pragma unroll
    for (int k = 0; k < kBiasMaskRounds; ++k) {
      const int64_t v = bias_mask_token(part, threadIdx.x, k);
      w[k] = v < V ? allow[bias_mask_word(v)] : ~0u;
    }
#pragma unroll
    for (int k = 0; k < kBiasMaskRounds; ++k) {
      const int64_t v = bias_mask_token(part, threadIdx.x, k);
      if (v < V && !bias_allowed(w[k], v)) x[v] = floor_v;
    }
    return;
  }
  const int n = n_entries[0];
  PZ_DEVICE_CHECK(n >= 0 && n <= kBiasMaxEntries);
  const int64_t t = base_t[0] + (step_t != nullptr ? step_t[0] : 0);
  PZ_DEVICE_CHECK(t >= 0);
  int id[kBiasPerThread], u[kBiasPerThread];
  float b[kBiasPerThread];
#pragma unroll
  for (int k = 0; k < kBiasPerThread; ++k) {
    const int i = k * kBiasThreads + threadIdx.x;
    const bool in = i < n && i < kBiasMaxEntries;
    id[k] = in ? ids[i] : -1;
    b[k] = in ? bias[i] : 0.f;
    u[k] = in ? until[i] : 0;
  }
#pragma unroll
  for (int k = 0; k < kBiasPerThread; ++k) {
    const int i = k * kBiasThreads + threadIdx.x;
    if (i >= n || i >= kBiasMaxEntries) continue;
    const int tok = id[k];
    PZ_DEVICE_CHECK(tok >= 0 && tok < V);
    PZ_DEVICE_CHECK(i == 0 || ids[i - 1] < tok);  // ascending: no id twice, so no logit has two writers
    if ((unsigned)tok >= (unsigned)V) continue;
    if (allow != nullptr && !bias_allowed(allow[bias_mask_word(tok)], tok)) continue;  // a mask part's to write
    const bool masked = t < (int64_t)u[k] || b[k] == -INFINITY;
    x[tok] = masked ? floor_v : from_f<T>(to_f<T>(x[tok]) + b[k]);
  }
}

}  // namespace penroz

using namespace penroz;

// One rewrite of logits [B, V] (bf16 / fp32 / fp16, contiguous), in place, in front of the sampler.
// allow_on chooses the launch form: false, the entries alone (one workgroup per row; allow is not looked
// at); true, the entries and the allowed mask (allow int32 [ceil(V / 32)] is required).
void logit_bias_apply(torch::Tensor logits, torch::Tensor ids, torch::Tensor bias, torch::Tensor until,
                      torch::Tensor n_entries, c10::optional<torch::Tensor> allow, bool allow_on, torch::Tensor base_t,
                      c10::optional<torch::Tensor> step_t) {
  const char* who = "logit_bias_apply";
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2, who,
              ": contiguous device logits [B, V]");
  const int64_t B = logits.size(0), V = logits.size(1);
  const LogitBiasPlan plan = plan_logit_bias(B, V, allow_on);
  TORCH_CHECK(plan.grid > 0, who, ": B >= 1, 1 <= V < 2^31 and B x (1 + parts) workgroups below 2^31, got B = ", B,
              ", V = ", V);
  la_one_device(who, logits, {ids, bias, until, n_entries, base_t, step_t});
  const int* ip = la_i32_shape(who, "ids", ids, {kBiasMaxEntries});
  const float* bp = la_f32_vec(who, "bias", bias, kBiasMaxEntries);
  const int* up = la_i32_shape(who, "until", until, {kBiasMaxEntries});
  const int* np = la_i32_shape(who, "n_entries", n_entries, {1});
  const unsigned* ap = nullptr;
  if (allow_on) {
    TORCH_CHECK(la_defined(allow), who, ": the mask form needs allow");
    la_one_device(who, logits, {allow});
    ap = reinterpret_cast<const unsigned*>(la_i32_shape(who, "allow", *allow, {plan.mask_words}));
  }
  const int64_t* bt = la_i64_scalar(who, "base_t", base_t);
  const int64_t* st = la_defined(step_t) ? la_i64_scalar(who, "step_t", *step_t) : nullptr;
  auto stream = at::hip::getCurrentHIPStream();
  la_by_elem(who, logits.scalar_type(), [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(logit_bias_kernel<T>, dim3((unsigned)plan.grid), dim3(kBiasThreads), 0, stream,
                       reinterpret_cast<T*>(logits.data_ptr()), ip, bp, up, np, ap, bt, st, (int)V, plan.per_row);
  });
}

// (parts per row, workgroups, mask words) of the launch: host only
std::tuple<int64_t, int64_t, int64_t> logit_bias_plan(int64_t B, int64_t V, bool allow_on) {
  const LogitBiasPlan p = plan_logit_bias(B, V, allow_on);
  return {p.per_row, p.grid, p.mask_words};
}

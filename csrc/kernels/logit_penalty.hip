// Repetition, presence and frequency penalties on the logits of a decode step, between the lm_head
// and the sampler (definition: ops/penalties.py, vLLM's).
//
// State per decoder, for B rows over a vocabulary of V:
//   cnt    int32 [B, V]  bit 31: the token occurs in the row's prompt; low 31 bits: how often this
//                        call generated it in this row
//   uniq   int32 [B, V]  the tokens whose cnt entry is non-zero, in no particular order
//   n_uniq int32 [B]     how many of them
//   params fp32  [3]     (repetition, presence, frequency): read on the device, so other values
//                        replay the same captured graph
// Both kernels walk `uniq`, never the row: a step's cost follows the distinct tokens seen (a few
// thousand at most), not V (Gemma: 262 144 logits x 64 rows would be 67 MB per token).
//
// penalty_begin  once per generate call: clears the previous call's entries through its own list,
//                then registers the prompt (atomicOr on bit 31; whoever saw 0 appends the token).
// penalty_apply  once per sampling: thread 0 counts the token the previous step sampled, then each
//                listed token's logit is rewritten by exactly one thread (no atomics, no races),
//                one element per store (rows of odd V have no vector alignment).
// The arithmetic is fp32 with no contraction (each product and sum rounded on its own, as torch
// does), rounded once to the logits' dtype: bit-identical to ops/penalties.py reference_penalise.
#include "common.h"
#include "launch_args.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {

constexpr int kPenThreads = 256;
constexpr unsigned kInPrompt = 1u << 31;

__global__ __launch_bounds__(kPenThreads) void penalty_begin_kernel(int* cnt, int* uniq, int* n_uniq,
                                                                    const int64_t* __restrict__ prompt, int T, int V) {
  __shared__ int n_new;
  const int row = blockIdx.x;
  int* c = cnt + (size_t)row * V;
  int* u = uniq + (size_t)row * V;
  const int n_old = n_uniq[row];
  PZ_DEVICE_CHECK(n_old >= 0 && n_old <= V);
  for (int i = threadIdx.x; i < n_old && i < V; i += kPenThreads) {
    const int tok = u[i];
    PZ_DEVICE_CHECK(tok >= 0 && tok < V);
    if ((unsigned)tok < (unsigned)V) c[tok] = 0;
  }
  if (threadIdx.x == 0) n_new = 0;
  __threadfence();  // the cleared entries are in place before any atomicOr below reads them
  __syncthreads();
  const int64_t* p = prompt + (size_t)row * T;
  for (int t = threadIdx.x; t < T; t += kPenThreads) {
    const int64_t tok = p[t];
    PZ_DEVICE_CHECK(tok >= 0 && tok < V);
    if ((uint64_t)tok >= (uint64_t)V) continue;  // (the Python wrapper refuses such a prompt)
    const unsigned old = atomicOr(reinterpret_cast<unsigned*>(c) + tok, kInPrompt);
    if (old == 0) {  // first to see the token of a cleared row: at most V appends
      const int slot = atomicAdd(&n_new, 1);
      PZ_DEVICE_CHECK(slot < V);
      if (slot < V) u[slot] = (int)tok;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) n_uniq[row] = min(n_new, V);
}

template <typename T>
__global__ __launch_bounds__(kPenThreads) void penalty_apply_kernel(T* logits, int* cnt, int* uniq, int* n_uniq,
                                                                    const float* __restrict__ params,
                                                                    const int64_t* __restrict__ new_tok, int V) {
#pragma clang fp contract(off)
  const int row = blockIdx.x;
  int* c = cnt + (size_t)row * V;
  int* u = uniq + (size_t)row * V;
  T* x = logits + (size_t)row * V;
  if (new_tok != nullptr) {
    // the token the previous step sampled is not counted yet: one thread, before anyone reads
    if (threadIdx.x == 0) {
      const int64_t tok = new_tok[row];
      PZ_DEVICE_CHECK(tok >= 0 && tok < V);
      if ((uint64_t)tok < (uint64_t)V) {
        const int old = c[tok];
        if (old == 0) {
          const int n = n_uniq[row];
          PZ_DEVICE_CHECK(n >= 0 && n < V);
          if (n >= 0 && n < V) {
            u[n] = (int)tok;
            n_uniq[row] = n + 1;
            c[tok] = 1;
          }
        } else {
          c[tok] = old + 1;
        }
      }
    }
    __threadfence_block();
    __syncthreads();
  }
  const int n = n_uniq[row];
  PZ_DEVICE_CHECK(n >= 0 && n <= V);
  const float rep = params[0], pres = params[1], freq = params[2];
  for (int i = threadIdx.x; i < n && i < V; i += kPenThreads) {
    const int tok = u[i];
    PZ_DEVICE_CHECK(tok >= 0 && tok < V);
    if ((unsigned)tok >= (unsigned)V) continue;
    const unsigned e = (unsigned)c[tok];
    const int gen = (int)(e & ~kInPrompt);
    float y = to_f<T>(x[tok]);
    if (e != 0) y = y > 0.f ? y / rep : y * rep;
    if (gen > 0) {
      const float scaled = freq * (float)gen;
      const float pen = pres + scaled;
      y = y - pen;
    }
    x[tok] = from_f<T>(y);
  }
}

// cnt / uniq int32 [B, V] and n_uniq int32 [B], contiguous, on `first`'s device
static void check_state(const char* who, const torch::Tensor& first, const torch::Tensor& cnt,
                        const torch::Tensor& uniq, const torch::Tensor& n_uniq, int64_t B, int64_t V) {
  la_one_device(who, first, {cnt, uniq, n_uniq});
  for (const torch::Tensor* t : {&cnt, &uniq})
    TORCH_CHECK(t->scalar_type() == torch::kInt32 && t->is_contiguous() && t->dim() == 2 && t->size(0) == B &&
                    t->size(1) == V, who, ": cnt and uniq must be contiguous int32 [B = ", B, ", V = ", V, "]");
  TORCH_CHECK(n_uniq.scalar_type() == torch::kInt32 && n_uniq.is_contiguous() && n_uniq.numel() == B, who,
              ": n_uniq must be contiguous int32 [B = ", B, "]");
  TORCH_CHECK(cnt.data_ptr() != uniq.data_ptr(), who, ": cnt and uniq must be two buffers");
  TORCH_CHECK(B >= 1 && V >= 1 && V < (int64_t(1) << 31), who, ": B >= 1 and 1 <= V < 2^31");
}

}  // namespace penroz

using namespace penroz;

// Start of a generate call: forget the previous call's tokens (sparsely) and mark the prompt's.
// prompt int64 [B, T]; ids outside [0, V) are the caller's to refuse (they are skipped here).
void penalty_begin(torch::Tensor cnt, torch::Tensor uniq, torch::Tensor n_uniq, torch::Tensor prompt) {
  const char* who = "penalty_begin";
  TORCH_CHECK(cnt.dim() == 2, who, ": cnt must be int32 [B, V]");
  const int64_t B = cnt.size(0), V = cnt.size(1);
  check_state(who, cnt, cnt, uniq, n_uniq, B, V);
  la_one_device(who, cnt, {prompt});
  TORCH_CHECK(prompt.scalar_type() == torch::kInt64 && prompt.is_contiguous() && prompt.dim() == 2 &&
                  prompt.size(0) == B && prompt.size(1) < (int64_t(1) << 31),
              who, ": prompt must be contiguous int64 [B = ", B, ", T]");
  hipLaunchKernelGGL(penalty_begin_kernel, dim3((unsigned)B), dim3(kPenThreads), 0, at::hip::getCurrentHIPStream(),
                     cnt.data_ptr<int>(), uniq.data_ptr<int>(), n_uniq.data_ptr<int>(), prompt.data_ptr<int64_t>(),
                     (int)prompt.size(1), (int)V);
}

// One sampling: count new_tok (int64 [B] or [B, 1], the previous step's tokens; None: nothing to
// count) and penalise the listed tokens' logits in place. logits [B, V] bf16 / fp32 / fp16.
void penalty_apply(torch::Tensor logits, torch::Tensor cnt, torch::Tensor uniq, torch::Tensor n_uniq,
                   torch::Tensor params, c10::optional<torch::Tensor> new_tok) {
  const char* who = "penalty_apply";
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2, who,
              ": contiguous device logits [B, V]");
  const int64_t B = logits.size(0), V = logits.size(1);
  check_state(who, logits, cnt, uniq, n_uniq, B, V);
  la_one_device(who, logits, {params, new_tok});
  const float* pp = la_f32_vec(who, "params (repetition, presence, frequency)", params, 3);
  const int64_t* nt = nullptr;
  if (la_defined(new_tok)) {
    TORCH_CHECK(new_tok->scalar_type() == torch::kInt64 && new_tok->is_contiguous() && new_tok->numel() == B, who,
                ": new_tok must be contiguous int64 [B = ", B, "]");
    nt = new_tok->data_ptr<int64_t>();
  }
  auto stream = at::hip::getCurrentHIPStream();
  la_by_elem(who, logits.scalar_type(), [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(penalty_apply_kernel<T>, dim3((unsigned)B), dim3(kPenThreads), 0, stream,
                       reinterpret_cast<T*>(logits.data_ptr()), cnt.data_ptr<int>(), uniq.data_ptr<int>(),
                       n_uniq.data_ptr<int>(), pp, nt, (int)V);
  });
}

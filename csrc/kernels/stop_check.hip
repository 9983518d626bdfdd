// Stop sequences checked on the device, at the end of a decode step (definition: ops/stopping.py).
//
// The stop set, shared by all rows and read on the device, so another set replays the same graph:
//   seqs    int32 [16, 8]  the sequences' token ids, each from slot 0
//   seq_len int32 [16]     their lengths (1..8)
//   n_seqs  int32 [1]      how many are in use
// State per row, for B rows:
//   tail      int32 [B, 8]  the last 8 tokens this call generated, the newest in slot 7; -1: none yet
//   n_gen     int32 [B]     how many it generated
//   done      int32 [B]     0: running; else 1 + the index of the sequence that finished the row
//   finish_at int32 [B]     the number of generated tokens at which it finished
//
// stop_begin    once per generate call: clears the state.
// stop_observe  one generated token per row (int64 [B], in place): a running row shifts it into its
//               tail and compares; a finished row is frozen — its token is overwritten with the one it
//               finished on (tail slot 7) and its state is left alone.
// stop_step     the same inside the captured step, behind the sampler and the counter advance: the
//               token is the next step's input idx, and column *step - 1 of the burst buffer is
//               rewritten with it for the frozen rows.
// One 64-lane workgroup per row: lane s compares sequence s, aligned to its end, against the shifted
// tail; the lowest matching lane wins by a wave-wide minimum; lane 0 writes the row's state. Integers
// only, no atomics, nothing shared between rows: exactly reproducible.
#include "common.h"
#include "launch_args.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {

constexpr int kStopMaxSeqs = 16;
constexpr int kStopMaxLen = 8;
constexpr int kStopLanes = 64;
static_assert(kStopMaxSeqs <= kStopLanes, "one lane per sequence");

__global__ __launch_bounds__(kStopLanes) void stop_begin_kernel(int* __restrict__ tail, int* __restrict__ n_gen,
                                                                int* __restrict__ done, int* __restrict__ finish_at) {
  const int row = blockIdx.x, lane = threadIdx.x;
  if (lane < kStopMaxLen) tail[(size_t)row * kStopMaxLen + lane] = -1;
  if (lane == 0) {
    n_gen[row] = 0;
    done[row] = 0;
    finish_at[row] = 0;
  }
}

// tok int64 [B]; out_buf: nullptr, or int64 [B, cap] with step the burst's counter, already advanced
__global__ __launch_bounds__(kStopLanes) void stop_observe_kernel(const int* __restrict__ seqs,
                                                                  const int* __restrict__ seq_len,
                                                                  const int* __restrict__ n_seqs, int* tail, int* n_gen,
                                                                  int* done, int* finish_at, int64_t* tok,
                                                                  int64_t* out_buf, int64_t cap,
                                                                  const int64_t* __restrict__ step) {
  const int row = blockIdx.x, lane = threadIdx.x;
  int* tl = tail + (size_t)row * kStopMaxLen;
  if (done[row] != 0) {  // (uniform over the workgroup) frozen: every later token is the finishing one
    if (lane == 0) {
      const int64_t keep = tl[kStopMaxLen - 1];
      tok[row] = keep;
      if (out_buf != nullptr) {
        const int64_t col = *step - 1;
        PZ_DEVICE_CHECK(col >= 0 && col < cap);
        if (col >= 0 && col < cap) out_buf[(size_t)row * cap + col] = keep;
      }
    }
    return;
  }
  // the shifted tail, in registers of every lane: the stores below come after all of these loads
  int t[kStopMaxLen];
#pragma unroll
  for (int i = 0; i + 1 < kStopMaxLen; ++i) t[i] = tl[i + 1];
  t[kStopMaxLen - 1] = (int)tok[row];
  const int n = n_gen[row] + 1;
  const int ns = min(max(n_seqs[0], 0), kStopMaxSeqs);
  int win = kStopLanes;
  if (lane < ns) {
    const int L = seq_len[lane];
    PZ_DEVICE_CHECK(L >= 1 && L <= kStopMaxLen);
    bool hit = L >= 1 && L <= kStopMaxLen && L <= n;  // (a match lies wholly inside the generated tokens)
#pragma unroll
    for (int j = 0; j < kStopMaxLen; ++j) {
      // slot j of the tail belongs to the sequence's element j - (8 - L)
      const int e = j - (kStopMaxLen - L);
      if (hit && e >= 0 && seqs[lane * kStopMaxLen + e] != t[j]) hit = false;
    }
    if (hit) win = lane;
  }
  for (int o = kStopLanes / 2; o > 0; o >>= 1) win = min(win, __shfl_xor(win, o, kStopLanes));
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < kStopMaxLen; ++i) tl[i] = t[i];
    n_gen[row] = n;
    if (win < kStopLanes) {
      done[row] = win + 1;
      finish_at[row] = n;
    }
  }
}

struct StopArgs {
  const int *seqs, *seq_len, *n_seqs;
  int *tail, *n_gen, *done, *finish_at;
  int64_t B;
};

static StopArgs check_stop_state(const char* who, const torch::Tensor& seqs, const torch::Tensor& seq_len,
                                 const torch::Tensor& n_seqs, const torch::Tensor& tail, const torch::Tensor& n_gen,
                                 const torch::Tensor& done, const torch::Tensor& finish_at) {
  TORCH_CHECK(tail.dim() == 2 && tail.size(0) >= 1 && tail.size(0) < (int64_t(1) << 31), who,
              ": tail must be int32 [B >= 1, ", kStopMaxLen, "]");
  const int64_t B = tail.size(0);
  la_one_device(who, tail, {seqs, seq_len, n_seqs, n_gen, done, finish_at});
  StopArgs a;
  a.B = B;
  a.seqs = la_i32_shape(who, "seqs", seqs, {kStopMaxSeqs, kStopMaxLen});
  a.seq_len = la_i32_shape(who, "seq_len", seq_len, {kStopMaxSeqs});
  a.n_seqs = la_i32_shape(who, "n_seqs", n_seqs, {1});
  a.tail = la_i32_shape(who, "tail", tail, {B, kStopMaxLen});
  a.n_gen = la_i32_shape(who, "n_gen", n_gen, {B});
  a.done = la_i32_shape(who, "done", done, {B});
  a.finish_at = la_i32_shape(who, "finish_at", finish_at, {B});
  return a;
}

static int64_t* check_tokens(const char* who, const torch::Tensor& tok, int64_t B) {
  TORCH_CHECK(tok.is_cuda() && tok.scalar_type() == torch::kInt64 && tok.is_contiguous() && tok.numel() == B &&
                  (tok.dim() == 1 || (tok.dim() == 2 && tok.size(0) == B)),
              who, ": tokens must be contiguous int64 [B = ", B, "] or [B, 1]");
  return tok.data_ptr<int64_t>();
}

}  // namespace penroz

using namespace penroz;

// Start of a generate call: no tokens generated, no row finished.
void stop_begin(torch::Tensor tail, torch::Tensor n_gen, torch::Tensor done, torch::Tensor finish_at) {
  const char* who = "stop_begin";
  TORCH_CHECK(tail.dim() == 2 && tail.size(0) >= 1 && tail.size(0) < (int64_t(1) << 31), who,
              ": tail must be int32 [B >= 1, ", kStopMaxLen, "]");
  const int64_t B = tail.size(0);
  la_one_device(who, tail, {n_gen, done, finish_at});
  int* tl = la_i32_shape(who, "tail", tail, {B, kStopMaxLen});
  int* ng = la_i32_shape(who, "n_gen", n_gen, {B});
  int* dn = la_i32_shape(who, "done", done, {B});
  int* fa = la_i32_shape(who, "finish_at", finish_at, {B});
  hipLaunchKernelGGL(stop_begin_kernel, dim3((unsigned)B), dim3(kStopLanes), 0, at::hip::getCurrentHIPStream(), tl, ng,
                     dn, fa);
}

// One generated token per row, eager: tok int64 [B] (or [B, 1]) is checked, and overwritten for the
// rows that had finished before.
void stop_observe(torch::Tensor seqs, torch::Tensor seq_len, torch::Tensor n_seqs, torch::Tensor tail,
                  torch::Tensor n_gen, torch::Tensor done, torch::Tensor finish_at, torch::Tensor tok) {
  const char* who = "stop_observe";
  const StopArgs a = check_stop_state(who, seqs, seq_len, n_seqs, tail, n_gen, done, finish_at);
  la_one_device(who, tail, {tok});
  int64_t* tp = check_tokens(who, tok, a.B);
  hipLaunchKernelGGL(stop_observe_kernel, dim3((unsigned)a.B), dim3(kStopLanes), 0, at::hip::getCurrentHIPStream(),
                     a.seqs, a.seq_len, a.n_seqs, a.tail, a.n_gen, a.done, a.finish_at, tp, (int64_t*)nullptr,
                     (int64_t)0, (const int64_t*)nullptr);
}

// The captured step's form, last in the step: idx int64 [B, 1] holds the tokens just chosen (the next
// step's input), out_buf int64 [B, cap] the burst's tokens, step the burst's counter, already
// advanced: idx[b] and out_buf[b, *step - 1] are rewritten for the rows that had finished before.
void stop_step(torch::Tensor seqs, torch::Tensor seq_len, torch::Tensor n_seqs, torch::Tensor tail,
               torch::Tensor n_gen, torch::Tensor done, torch::Tensor finish_at, torch::Tensor idx,
               torch::Tensor out_buf, torch::Tensor step) {
  const char* who = "stop_step";
  const StopArgs a = check_stop_state(who, seqs, seq_len, n_seqs, tail, n_gen, done, finish_at);
  la_one_device(who, tail, {idx, out_buf, step});
  int64_t* tp = check_tokens(who, idx, a.B);
  TORCH_CHECK(out_buf.is_cuda() && out_buf.scalar_type() == torch::kInt64 && out_buf.is_contiguous() &&
                  out_buf.dim() == 2 && out_buf.size(0) == a.B && out_buf.size(1) >= 1,
              who, ": out_buf must be contiguous int64 [B = ", a.B, ", cap >= 1]");
  const int64_t* sp = la_i64_scalar(who, "step", step);
  hipLaunchKernelGGL(stop_observe_kernel, dim3((unsigned)a.B), dim3(kStopLanes), 0, at::hip::getCurrentHIPStream(),
                     a.seqs, a.seq_len, a.n_seqs, a.tail, a.n_gen, a.done, a.finish_at, tp, out_buf.data_ptr<int64_t>(),
                     (int64_t)out_buf.size(1), sp);
}

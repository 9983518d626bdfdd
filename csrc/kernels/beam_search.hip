// Beam search inside the decode step (definition: ops/beam_search.py). W live beams of one prompt, each
// with a cumulative log-probability c_b; a step takes the R_in rows of bf16 logits the lm_head wrote,
// scores every continuation s(b, v) = c_b + (x_b[v] - logsumexp(x_b)) in fp32, takes the 2W best under
// the total order (s descending, b ascending, v ascending), walks them into the next live beams and the
// finished list, and re-parents the rows' suffix K/V caches.
//
// beam_step: two launches; stream order is the only synchronisation, no atomics, every reduction a fixed
// tree, so the result is bitwise reproducible. Step index, R_in, stop token, c and inv_norm come from the
// device: one captured step serves every step, every length penalty and every stop token.
//
// beam_part_kernel    grid (P, rows), 256 threads: part p covers logits [4096 p, 4096 (p + 1)) of a row
//   of any stride, 16 per thread (two 8-element chunks) plus one ragged element, read as in
//   token_logprobs.hip: single elements up to the first 16-B boundary and behind the last whole chunk,
//   16-B vectors in between, every load issued before the first use. It writes the part's maximum,
//   s_p = Σ exp(x - m_p) (per thread, then a fixed tree) and its K = 2W best as unique 64-bit keys
//   (order-preserving bits of x, ~v), best first. Within a row s is monotone in x, so the part's order by
//   x is the definition's order up to collisions of s for distinct logits, which the merge key decides.
// beam_merge_kernel   one workgroup: per-row lse from the partials in part order (one wave per row, one
//   lane per part, fixed tree), then keys (order-preserving bits of fp32 s, ~b, ~v) of the
//   R_in · P · K <= 8192 candidates, the K best of them, and the walk by one thread.
//
// Selection (select_top, both kernels). token_logprobs.hip runs n dependent rounds of a workgroup-wide
// maximum, each a DPP tree plus a barrier; here the dependent chain is four barriers whatever K is:
//   1. every thread keeps its NK keys in registers and publishes their maximum (256 maxima in LDS);
//   2. every thread counts the maxima above its own (ties by thread index): a rank. Keys are unique, so
//      exactly K threads get a rank below K, and the maximum of rank K - 1 is a threshold tau that at
//      least K keys reach — and no thread outside those K holds a key >= tau;
//   3. the thread of rank r < K copies its keys >= tau into row r of a K x NK survivor table
//      (0 elsewhere): the slots are owned, no counter is bumped, the table's content is deterministic;
//   4. every survivor counts the survivors above it — its rank in the part — and the ranks below K are
//      the output, already sorted.
// A threshold from per-wave maxima would have only four waves to draw on at 256 threads; the
// per-thread maxima give a threshold with the same proof and a bound of K · NK survivors, so they are
// used instead. All LDS reads of steps 2 and 4 are broadcasts (every lane reads the same address).
// LDS: 2 KiB maxima + K·NK·8 B survivors: 4.3 KiB in the part kernel (NK = 18), 6.1 KiB in the merge
// kernel (NK = 32) — the merge never stages all 8192 keys in LDS; what bounds W is K <= 16 output
// slots and the P <= 64 lanes of the lse wave (V <= 262144).
//
// beam_reorder_kernel  the step's last kernel: row r of every layer's suffix K and V cache becomes row
//   parent[r], slots [0, n) with n read from the device, in place, one launch for all layers. A
//   workgroup owns one 4-KiB piece of one (layer, K or V, KV head) plane for ALL W rows: thread i loads
//   its 16 B of row parent[r] for every r — all loads are issued before the first store — then stores
//   them to row r. No two workgroups touch the same bytes, so any parent (a swap, all-from-one) is
//   safe without a second buffer. The layers come from a device table (base pointers, Hkv, D, capacity,
//   first workgroup): layer lists mix head shapes. A workgroup behind slot n leaves at once, and one that
//   reads an identity parent leaves without touching the cache. Registers are indexed by the unrolled
//   row, never by parent[r]: no scratch.
#include "common.h"
#include "launch_args.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {

constexpr int kBeamThreads = 256;
constexpr int kBeamPartNK = 18;   // keys per thread in the part kernel: 16 + 1 ragged, padded to even
constexpr int kBeamMergeNK = 32;  // ... in the merge kernel: 8192 candidates / 256 threads

// control words (int32) of a beam call, shared with ops/beam_search.py BeamState
enum BeamCtl { kCtlStep = 0, kCtlSteps = 1, kCtlRows = 2, kCtlStop = 3, kCtlFinished = 4, kCtlSlots = 5, kCtlWords = 8 };

__device__ __forceinline__ uint32_t bm_order_key(float f) {  // (sampling.hip order_key)
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float bm_key_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// The K largest of the workgroup's 256 x NK keys (unique, 0 = none) -> out[0..K), best first, 0 where
// the keys run out. maxima: [256], surv: [16 * NK], out: [16] in LDS. Every thread calls it.
template <int NK>
__device__ __forceinline__ void select_top(const uint64_t (&key)[NK], int K, uint64_t* maxima, uint64_t* surv,
                                           uint64_t* out) {
  const int t = threadIdx.x;
  uint64_t mine = 0;
#pragma unroll
  for (int i = 0; i < NK; ++i) mine = key[i] > mine ? key[i] : mine;
  maxima[t] = mine;
  if (t < 16) out[t] = 0;
  __syncthreads();
  int rank = 0;
  for (int j = 0; j < kBeamThreads; j += 2) {  // broadcast reads, 16 B each
    const uint64_t a = maxima[j], b = maxima[j + 1];
    rank += (a > mine || (a == mine && j < t)) ? 1 : 0;
    rank += (b > mine || (b == mine && j + 1 < t)) ? 1 : 0;
  }
  // ranks are a permutation, so exactly one thread holds the maximum of rank K - 1: the threshold
  uint64_t* tau_slot = surv + 16 * NK;  // one word behind the table
  if (rank == K - 1) *tau_slot = mine;
  __syncthreads();
  const uint64_t tau = *tau_slot;
  if (rank < K) {
#pragma unroll
    for (int i = 0; i < NK; ++i) surv[rank * NK + i] = (key[i] >= tau && key[i] != 0) ? key[i] : 0;
  }
  __syncthreads();
  const int ns = K * NK;
  for (int s = t; s < ns; s += kBeamThreads) {
    const uint64_t k = surv[s];
    if (k == 0) continue;
    int r = 0;
    for (int j = 0; j < ns; j += 2) r += (surv[j] > k ? 1 : 0) + (surv[j + 1] > k ? 1 : 0);
    if (r < K) out[r] = k;
  }
  __syncthreads();
}

__device__ __forceinline__ int bm_width(int W) { return min(max(W, 1), kBeamMaxW); }

// ws per row (floats): m [P], s [P], keys uint64 [P, 16]
template <typename T>
__global__ void __launch_bounds__(kBeamThreads) beam_part_kernel(const T* __restrict__ logits, int64_t row_stride, int V,
                                                                 int P, int W, const int* __restrict__ ctl,
                                                                 float* __restrict__ ws, int64_t ws_row) {
  __shared__ float fred[2][4];
  __shared__ __attribute__((aligned(16))) uint64_t maxima[kBeamThreads];
  __shared__ __attribute__((aligned(16))) uint64_t surv[16 * kBeamPartNK + 2];
  __shared__ uint64_t outk[16];
  const int part = blockIdx.x, row = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (ctl[kCtlStep] >= ctl[kCtlSteps] || row >= ctl[kCtlRows]) return;  // (uniform)
  const int base = part * kBeamPartN;
  const int len = min(kBeamPartN, V - base);  // >= 1: the grid has ceil(V / 4096) parts
  const T* pp = logits + (size_t)row * row_stride + base;
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
    const int j = t + kBeamThreads * c;
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

  uint64_t key[kBeamPartNK];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t idx = (uint32_t)(base + head + 8 * (t + kBeamThreads * c) + e);
      key[8 * c + e] = ok[c] ? (((uint64_t)bm_order_key(v[c][e]) << 32) | (uint32_t)~idx) : 0;
    }
  key[16] = t < rag ? (((uint64_t)bm_order_key(r) << 32) | (uint32_t)~(uint32_t)(base + ri)) : 0;
  key[17] = 0;
  const int K = 2 * bm_width(W);
  select_top<kBeamPartNK>(key, K, maxima, surv, outk);
  uint64_t* keys = reinterpret_cast<uint64_t*>(wr + 2 * (size_t)P) + (size_t)part * 16;
  if (t < 16) keys[t] = t < K ? outk[t] : 0;
}

struct BeamIO {
  int* ctl;            // [kCtlWords]
  float* cum;          // [kBeamMaxW]
  const float* inv_norm;  // [steps + 1]: inv_norm[t] for t generated tokens
  int64_t* idx;        // [W] the next step's input tokens
  int* parent;         // [W]
  int* hist;           // [steps, W, 2] (token, parent)
  float* fin_f;        // [W, 2] (normalised score, s)
  int* fin_i;          // [W, 4] (step t, parent, walk rank, token)
  int64_t* adv_a;      // position / cache length / burst step counters (+1 each), or nullptr
  int64_t* adv_b;
  int64_t* adv_c;
};

__global__ void __launch_bounds__(kBeamThreads) beam_merge_kernel(int V, int P, int W, const float* __restrict__ ws,
                                                                  int64_t ws_row, BeamIO io) {
  __shared__ float lse[kBeamMaxW];
  __shared__ __attribute__((aligned(16))) uint64_t maxima[kBeamThreads];
  __shared__ __attribute__((aligned(16))) uint64_t surv[16 * kBeamMergeNK + 2];
  __shared__ uint64_t outk[16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int step = io.ctl[kCtlStep], steps = io.ctl[kCtlSteps];
  if (step < 0 || step >= steps) return;  // (uniform) a step behind the last writes nothing
  W = bm_width(W);
  const int rows = min(max(io.ctl[kCtlRows], 1), W), K = 2 * W;
  const int stop = io.ctl[kCtlStop];
  for (int row = w; row < rows; row += 4) {  // one wave per row, one lane per part (P <= 64)
    const float* wr = ws + (size_t)row * ws_row;
    const bool has = lane < P;
    const float mp = has ? wr[lane] : -INFINITY;
    const float sp = has ? wr[P + lane] : 0.f;
    const float m = wave_max(mp);
    const float sum = wave_sum(has ? sp * expf(mp - m) : 0.f);
    if (lane == 0) lse[row] = m + logf(sum);
  }
  __syncthreads();
  const int per_row = P * K, n = rows * per_row;  // <= 8 * 64 * 16 = 8192
  uint64_t key[kBeamMergeNK];
#pragma unroll
  for (int i = 0; i < kBeamMergeNK; ++i) {
    const int j = t + kBeamThreads * i;
    key[i] = 0;
    if (j < n) {
      const int row = j / per_row, rem = j - row * per_row, part = rem / K, slot = rem - part * K;
      const uint64_t pk = reinterpret_cast<const uint64_t*>(ws + (size_t)row * ws_row + 2 * (size_t)P)[part * 16 + slot];
      if (pk != 0) {
        const float x = bm_key_value((uint32_t)(pk >> 32));
        const uint32_t v = ~(uint32_t)pk;
        const float s = io.cum[row] + (x - lse[row]);
        key[i] = ((uint64_t)bm_order_key(s) << 32) | ((uint32_t)(7 - row) << 29) | (0x1fffffffu - v);
      }
    }
  }
  select_top<kBeamMergeNK>(key, K, maxima, surv, outk);
  if (t != 0) return;
  // the walk, in the definition's order: a stop candidate joins the finished list, any other one is the
  // next live beam while slots are free
  const int tt = step + 1;  // generated tokens after this step
  const float norm = io.inv_norm[tt];
  int live = 0, nf = min(max(io.ctl[kCtlFinished], 0), W);
  int* hist = io.hist + (size_t)step * W * 2;
  for (int r = 0; r < K; ++r) {
    const uint64_t k = outk[r];
    if (k == 0) break;
    const float s = bm_key_value((uint32_t)(k >> 32));
    const uint32_t lo = (uint32_t)k;
    const int b = 7 - (int)(lo >> 29), v = (int)(0x1fffffffu - (lo & 0x1fffffffu));
    if (v == stop) {
      const float score = s * norm;
      int pos = nf;
      while (pos > 0 && io.fin_f[2 * (pos - 1)] < score) --pos;  // an equal score keeps the earlier entry in front
      if (pos < W) {
        for (int j = min(nf, W - 1); j > pos; --j) {
          io.fin_f[2 * j] = io.fin_f[2 * (j - 1)];
          io.fin_f[2 * j + 1] = io.fin_f[2 * (j - 1) + 1];
          for (int e = 0; e < 4; ++e) io.fin_i[4 * j + e] = io.fin_i[4 * (j - 1) + e];
        }
        io.fin_f[2 * pos] = score;
        io.fin_f[2 * pos + 1] = s;
        io.fin_i[4 * pos] = tt;
        io.fin_i[4 * pos + 1] = b;
        io.fin_i[4 * pos + 2] = r;
        io.fin_i[4 * pos + 3] = v;
        nf = min(nf + 1, W);
      }
    } else if (live < W) {
      io.idx[live] = v;
      io.parent[live] = b;
      io.cum[live] = s;  // (every thread read cum in front of select_top's barriers)
      hist[2 * live] = v;
      hist[2 * live + 1] = b;
      ++live;
    }
  }
  PZ_DEVICE_CHECK(live == W);
  io.ctl[kCtlFinished] = nf;
  io.ctl[kCtlStep] = tt;
  io.ctl[kCtlRows] = W;
  if (io.adv_a) {  // a decode step's: its K/V went into one more suffix slot
    ++io.ctl[kCtlSlots];
    ++*io.adv_a;
    ++*io.adv_b;
    ++*io.adv_c;
  }
}

// table: int64 [L + 1, 6]: per layer (K base, V base, Hkv, D, capacity in slots, first workgroup), then one
// row (W, workgroups, L, 0, 0, 0); rows of a cache are [W, Hkv, cap, D] bf16, contiguous.
constexpr int kReorderPieceBytes = kBeamThreads * 16;

template <int W>
__global__ void __launch_bounds__(kBeamThreads) beam_reorder_kernel(const int64_t* __restrict__ table, int L,
                                                                    const int* __restrict__ parent,
                                                                    const int* __restrict__ n_dev) {
  const int t = threadIdx.x;
  int par[W];
  bool identity = true, valid = true;
#pragma unroll
  for (int r = 0; r < W; ++r) {
    par[r] = parent[r];
    identity = identity && par[r] == r;
    valid = valid && par[r] >= 0 && par[r] < W;
  }
  PZ_DEVICE_CHECK(valid);
  if (identity || !valid) return;  // (uniform)
  int l = 0;
  while (l + 1 < L && (int64_t)blockIdx.x >= table[6 * (l + 1) + 5]) ++l;
  const int64_t* e = table + 6 * l;
  const int Hkv = (int)e[2], D = (int)e[3], cap = (int)e[4];
  const int64_t plane = (int64_t)cap * D * 2;  // bytes of one (row, head): a multiple of 16
  const int pieces = (int)((plane + kReorderPieceBytes - 1) / kReorderPieceBytes);
  int rel = (int)((int64_t)blockIdx.x - e[5]);
  const int piece = rel % pieces;
  rel /= pieces;
  const int head = rel % Hkv, which = rel / Hkv;  // which: 0 = K, 1 = V
  if (which > 1) return;
  const int n = min(max(*n_dev, 0), cap);
  const int64_t used = (int64_t)n * D * 2;  // bytes of a plane in use (<= plane)
  const int64_t off = (int64_t)piece * kReorderPieceBytes + 16 * t;  // this thread's byte offset inside the plane
  if (off >= used) return;  // behind the last slot: the whole workgroup when its piece is, else this thread
  char* base = reinterpret_cast<char*>(e[which]) + (int64_t)head * plane + off;
  const int64_t row_bytes = (int64_t)Hkv * plane;
  float4_t val[W];  // (a native vector type: the array stays in registers)
#pragma unroll
  for (int r = 0; r < W; ++r) val[r] = *reinterpret_cast<const float4_t*>(base + par[r] * row_bytes);
#pragma unroll
  for (int r = 0; r < W; ++r)
    if (par[r] != r) *reinterpret_cast<float4_t*>(base + r * row_bytes) = val[r];
}

// The int8 form, for TurboQuant suffix caches: the same design over planes described in bytes. table: int64
// [E + 1, 6], per entry (first base, second base, Hkv, bytes per slot, capacity in slots, first workgroup): a layer
// is two entries, its int8 K / V caches [W, Hkv, cap, D] (slot bytes D, a multiple of 16: moved in 16-B units) and
// its fp32 K / V scale planes [W, Hkv, cap] (slot bytes 4: moved in 4-B units, since n scales end on no 16-B
// boundary and nothing at or behind slot n may be written). A workgroup owns 256 units of one plane for all W rows.
template <int W, class U>
__device__ __forceinline__ void reorder_units(char* base, int64_t row_bytes, const int (&par)[W]) {
  U val[W];  // (a native type: the array stays in registers)
#pragma unroll
  for (int r = 0; r < W; ++r) val[r] = *reinterpret_cast<const U*>(base + par[r] * row_bytes);
#pragma unroll
  for (int r = 0; r < W; ++r)
    if (par[r] != r) *reinterpret_cast<U*>(base + r * row_bytes) = val[r];
}

template <int W>
__global__ void __launch_bounds__(kBeamThreads) beam_reorder_bytes_kernel(const int64_t* __restrict__ table, int E,
                                                                          const int* __restrict__ parent,
                                                                          const int* __restrict__ n_dev) {
  const int t = threadIdx.x;
  int par[W];
  bool identity = true, valid = true;
#pragma unroll
  for (int r = 0; r < W; ++r) {
    par[r] = parent[r];
    identity = identity && par[r] == r;
    valid = valid && par[r] >= 0 && par[r] < W;
  }
  PZ_DEVICE_CHECK(valid);
  if (identity || !valid) return;  // (uniform)
  int l = 0;
  while (l + 1 < E && (int64_t)blockIdx.x >= table[6 * (l + 1) + 5]) ++l;
  const int64_t* e = table + 6 * l;
  const int Hkv = (int)e[2], sb = (int)e[3], cap = (int)e[4];
  const int unit = sb % 16 == 0 ? 16 : 4;  // (uniform)
  const int64_t plane = (int64_t)cap * sb;  // bytes of one (row, head)
  const int pieces = (int)((plane + kBeamThreads * unit - 1) / (kBeamThreads * unit));
  int rel = (int)((int64_t)blockIdx.x - e[5]);
  const int piece = rel % pieces;
  rel /= pieces;
  const int head = rel % Hkv, which = rel / Hkv;  // which: the entry's first or second base
  if (which > 1) return;
  const int n = min(max(*n_dev, 0), cap);
  const int64_t used = (int64_t)n * sb;  // bytes of a plane in use: a multiple of the unit
  const int64_t off = ((int64_t)piece * kBeamThreads + t) * unit;
  if (off >= used) return;  // behind the last slot: the whole workgroup when its piece is, else this thread
  char* base = reinterpret_cast<char*>(e[which]) + (int64_t)head * plane + off;
  const int64_t row_bytes = (int64_t)Hkv * plane;
  if (unit == 16) reorder_units<W, float4_t>(base, row_bytes, par);
  else reorder_units<W, float>(base, row_bytes, par);
}

template <int W>
static void launch_reorder(int64_t w, unsigned grid, hipStream_t stream, const int64_t* table, int L, const int* par,
                           const int* n, bool bytes = false) {
  if constexpr (W <= kBeamMaxW) {
    if (w != W) launch_reorder<W + 1>(w, grid, stream, table, L, par, n, bytes);
    else if (bytes) hipLaunchKernelGGL(beam_reorder_bytes_kernel<W>, dim3(grid), dim3(kBeamThreads), 0, stream, table, L, par, n);
    else hipLaunchKernelGGL(beam_reorder_kernel<W>, dim3(grid), dim3(kBeamThreads), 0, stream, table, L, par, n);
  }
}

}  // namespace penroz

using namespace penroz;

// (parts per row, workspace floats per row) (host only)
std::tuple<int64_t, int64_t> beam_step_plan(int64_t V, int64_t W) {
  const BeamPlan p = plan_beam_step(V, W);
  TORCH_CHECK(p.parts > 0, "beam_step_plan: 2 <= W <= ", kBeamMaxW, " and 2 W <= V <= ", (int64_t)kBeamMaxParts * kBeamPartN,
              ", got W = ", W, ", V = ", V);
  return {p.parts, p.ws_floats};
}

static int* beam_i32(const char* who, const char* what, const torch::Tensor& t, int64_t at_least) {
  TORCH_CHECK(t.defined() && t.is_cuda() && t.scalar_type() == torch::kInt32 && t.is_contiguous() && t.numel() >= at_least,
              who, ": int32 contiguous device ", what, " of at least ", at_least);
  return t.data_ptr<int>();
}

// One beam step on logits [rows >= R_in, V] (bf16 / fp16 / fp32, unit column stride, any row stride). ctl int32
// [8] (step, steps T, R_in, stop token or -1, finished, suffix slots, -, -), cum fp32 [8], inv_norm fp32 [> T],
// idx int64 [W], parent int32 [W], hist int32 [T, W, 2], fin_f fp32 [W, 2], fin_i int32 [W, 4], workspace fp32
// [W * beam_step_plan(V, W)[1]]. pos_t / len_t / step_t (int64 [1], all or none): advanced by one, with ctl's
// suffix slot count. steps_cap: the T that hist and inv_norm were sized for (ctl's T is at most that).
void beam_step(torch::Tensor logits, torch::Tensor ctl, torch::Tensor cum, torch::Tensor inv_norm, torch::Tensor idx,
               torch::Tensor parent, torch::Tensor hist, torch::Tensor fin_f, torch::Tensor fin_i,
               torch::Tensor workspace, int64_t W, int64_t steps_cap, c10::optional<torch::Tensor> pos_t,
               c10::optional<torch::Tensor> len_t, c10::optional<torch::Tensor> step_t) {
  const char* who = "beam_step";
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.size(0) >= 1 && logits.size(0) <= kBeamMaxW &&
                  logits.stride(1) == 1 && logits.stride(0) >= logits.size(1),
              who, ": device logits [1..", kBeamMaxW, " rows, V], unit column stride");
  const int64_t rows = logits.size(0), V = logits.size(1);
  const BeamPlan p = plan_beam_step(V, W);
  TORCH_CHECK(p.parts > 0, who, ": 2 <= W <= ", kBeamMaxW, " and 2 W <= V <= ", (int64_t)kBeamMaxParts * kBeamPartN,
              ", got W = ", W, ", V = ", V);
  TORCH_CHECK(steps_cap >= 1, who, ": steps_cap >= 1");
  la_one_device(who, logits, {ctl, cum, inv_norm, idx, parent, hist, fin_f, fin_i, workspace, pos_t, len_t, step_t});
  BeamIO io{};
  io.ctl = beam_i32(who, "ctl", ctl, kCtlWords);
  io.cum = const_cast<float*>(la_f32_vec(who, "cum", cum, kBeamMaxW, true));
  io.inv_norm = la_f32_vec(who, "inv_norm", inv_norm, steps_cap + 1, true);
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt64 && idx.is_contiguous() && idx.numel() == W, who,
              ": idx must be contiguous int64 [W = ", W, "]");
  io.idx = idx.data_ptr<int64_t>();
  io.parent = beam_i32(who, "parent", parent, W);
  io.hist = beam_i32(who, "hist", hist, steps_cap * W * 2);
  io.fin_f = const_cast<float*>(la_f32_vec(who, "fin_f", fin_f, 2 * W, true));
  io.fin_i = beam_i32(who, "fin_i", fin_i, 4 * W);
  TORCH_CHECK(workspace.scalar_type() == torch::kFloat32 && workspace.is_contiguous() &&
                  workspace.numel() >= rows * p.ws_floats && la_aligned(workspace, 8),
              who, ": workspace must be contiguous 8-B aligned fp32 of at least ", rows * p.ws_floats);
  const int given = (int)la_defined(pos_t) + (int)la_defined(len_t) + (int)la_defined(step_t);
  TORCH_CHECK(given == 0 || given == 3, who, ": pos_t, len_t and step_t come together");
  if (given) {
    io.adv_a = la_i64_scalar(who, "pos_t", *pos_t);
    io.adv_b = la_i64_scalar(who, "len_t", *len_t);
    io.adv_c = la_i64_scalar(who, "step_t", *step_t);
  }
  auto stream = at::hip::getCurrentHIPStream();
  la_by_elem(who, logits.scalar_type(), [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(beam_part_kernel<T>, dim3(p.parts, (unsigned)rows), dim3(kBeamThreads), 0, stream,
                       reinterpret_cast<const T*>(logits.data_ptr()), (int64_t)logits.stride(0), (int)V, p.parts, (int)W,
                       io.ctl, workspace.data_ptr<float>(), p.ws_floats);
  });
  hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(kBeamThreads), 0, stream, (int)V, p.parts, (int)W,
                     workspace.data_ptr<float>(), p.ws_floats, io);
}

// The device table of beam_reorder for these suffix caches (each [W, Hkv, cap, D] bf16, contiguous, 16-B
// aligned; K and V of a layer alike): (table int64 [L + 1, 6] on the HOST, workgroups). beam_reorder takes the
// host table (it reads W, the grid and L from its last row) and a device copy of it.
// With k_scales / v_scales (per layer fp32 [W, Hkv, cap], contiguous) the caches are int8 (D % 16 == 0) and the
// table is the byte form's: two entries per layer, [2 L + 1, 6], its last row flagged.
std::tuple<torch::Tensor, int64_t> beam_reorder_table(std::vector<torch::Tensor> ks, std::vector<torch::Tensor> vs,
                                                      c10::optional<std::vector<torch::Tensor>> k_scales,
                                                      c10::optional<std::vector<torch::Tensor>> v_scales) {
  const char* who = "beam_reorder_table";
  TORCH_CHECK(!ks.empty() && ks.size() == vs.size(), who, ": one K and one V cache per layer");
  const bool q8 = k_scales.has_value() || v_scales.has_value();
  TORCH_CHECK(!q8 || (k_scales.has_value() && v_scales.has_value() && k_scales->size() == ks.size() &&
                      v_scales->size() == ks.size()),
              who, ": one K and one V scale plane per layer, or none");
  const int64_t L = (int64_t)ks.size(), W = ks[0].size(0), E = q8 ? 2 * L : L;
  const auto kind = q8 ? torch::kInt8 : torch::kBFloat16;
  auto host = torch::zeros({E + 1, 6}, torch::dtype(torch::kInt64));
  int64_t* h = host.data_ptr<int64_t>();
  int64_t wgs = 0;
  for (int64_t l = 0; l < L; ++l) {
    const torch::Tensor &k = ks[l], &v = vs[l];
    TORCH_CHECK(k.is_cuda() && k.scalar_type() == kind && k.dim() == 4 && k.is_contiguous() &&
                    la_aligned(k, 16) && k.size(0) == W && k.size(3) % (q8 ? 16 : 8) == 0 && v.is_cuda() && v.device() == k.device() &&
                    v.scalar_type() == kind && v.is_contiguous() && la_aligned(v, 16) && v.sizes() == k.sizes() &&
                    k.device() == ks[0].device(),
                who, ": layer ", l, ": ", q8 ? "int8" : "bf16", " contiguous 16-B aligned [W, Hkv, cap, D % ", q8 ? 16 : 8,
                " == 0] K and V on one device");
    int64_t* e = h + 6 * (q8 ? 2 * l : l);
    e[0] = reinterpret_cast<int64_t>(k.data_ptr());
    e[1] = reinterpret_cast<int64_t>(v.data_ptr());
    e[2] = k.size(1);
    e[3] = k.size(3);
    e[4] = k.size(2);
    e[5] = wgs;
    wgs += (q8 ? plan_beam_reorder_bytes(k.size(1), k.size(2), k.size(3)) : plan_beam_reorder(k.size(1), k.size(2), k.size(3))).workgroups;
    if (q8) {
      const torch::Tensor &sk = (*k_scales)[l], &sv = (*v_scales)[l];
      la_one_device(who, k, {sk, sv});
      e[6] = reinterpret_cast<int64_t>(la_f32_shape(who, "K scales", sk, {W, k.size(1), k.size(2)}));
      e[7] = reinterpret_cast<int64_t>(la_f32_shape(who, "V scales", sv, {W, k.size(1), k.size(2)}));
      e[8] = k.size(1);
      e[9] = 4;
      e[10] = k.size(2);
      e[11] = wgs;
      wgs += plan_beam_reorder_bytes(k.size(1), k.size(2), 4).workgroups;
    }
  }
  TORCH_CHECK(W >= 2 && W <= kBeamMaxW && wgs >= 1 && wgs < (int64_t)1 << 31, who, ": 2 <= W <= ", kBeamMaxW);
  h[6 * E] = W;
  h[6 * E + 1] = wgs;
  h[6 * E + 2] = E;
  h[6 * E + 3] = q8 ? 1 : 0;
  return {host, wgs};
}

// Row r of every cache of the table <- row parent[r], slots [0, n_t[0]); parent int32 [W], n_t int32 [1], both
// on the device table's device. The caches the table was built from must be alive.
void beam_reorder(torch::Tensor host_table, torch::Tensor table, torch::Tensor parent, torch::Tensor n_t) {
  const char* who = "beam_reorder";
  TORCH_CHECK(!host_table.is_cuda() && host_table.scalar_type() == torch::kInt64 && host_table.is_contiguous() &&
                  host_table.dim() == 2 && host_table.size(0) >= 2 && host_table.size(1) == 6,
              who, ": host table from beam_reorder_table");
  const int64_t* h = host_table.data_ptr<int64_t>() + 6 * (host_table.size(0) - 1);
  const int64_t W = h[0], workgroups = h[1], L = h[2];
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kInt64 && table.is_contiguous() &&
                  table.sizes() == host_table.sizes() && L == host_table.size(0) - 1,
              who, ": the device copy of the host table");
  TORCH_CHECK(W >= 2 && W <= kBeamMaxW && workgroups >= 1 && workgroups < (int64_t)1 << 31, who, ": 2 <= W <= ", kBeamMaxW);
  la_one_device(who, table, {parent, n_t});
  const int* par = beam_i32(who, "parent", parent, W);
  const int* n = beam_i32(who, "n_t", n_t, 1);
  launch_reorder<2>(W, (unsigned)workgroups, at::hip::getCurrentHIPStream(), table.data_ptr<int64_t>(), (int)L, par, n, h[3] != 0);
}

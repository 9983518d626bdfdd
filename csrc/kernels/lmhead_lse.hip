// Prompt scoring for MI355X: the lm_head GEMM x = h[N][C] · W[V][C]ᵀ (+ bias[V]) fused with the
// reductions a log-probability needs, so that no logit is ever written (bf16 operands, fp32
// accumulate, fp32 out). Per row i the launch produces
//   token_logprob[i] = x[i, target_i] − logsumexp(x[i, :]),
//   top_token[i]     = argmax_v x[i, v] (the lowest id among equal maxima),
//   top_logprob[i]   = max_v x[i, v] − logsumexp(x[i, :]),
// from the fp32 accumulators themselves: the logits are NOT rounded to bf16 first, unlike the module
// path (nn.Linear under autocast), and the target logit carries the same rounding as the sum it is
// compared with (ops/prompt_logprobs.py holds the definition and the fp64 reference).
//
// Work split. One 256-thread workgroup (4 waves) owns a row tile of 128·RB rows (RB = 1, 2) and one
// of S contiguous ranges of the vocabulary, which it sweeps in column tiles of 128; the row tile
// and S come from plan_lmhead_lse (host_plan.h), two workgroups per CU (72 KiB of LDS each at
// RB = 2), so that one workgroup's epilogue VALU runs under the other's MFMAs. Workgroups of one
// vocabulary range sit on one XCD (they share that range of W in its L2). W is read once per row
// tile; h (N·C·2 bytes, L2-resident) is re-streamed per column tile.
//
// Main loop. v_mfma_f32_32x32x16_bf16 with W as the A operand and h as the B operand: a lane's 16
// accumulator registers of a 32 × 32 block are 16 vocabulary columns (8(r>>2) + 4(lane>>5) + (r&3))
// of ONE row (lane & 31), so every per-row reduction is lane-local until the end of the sweep. A
// wave owns 32·RB rows × all 128 columns of the tile (RB × 4 blocks). Both operands arrive by
// LDS-DMA (global_load_lds_dwordx4, scalar base + per-lane offset) as stages of [rows][32 k] (64-B
// rows) in a 3-stage ring, two stages in flight, one counted vmcnt and one barrier per k-step; the
// ring runs on into the next column tile. The 16-B chunk c of tile row r sits at c ^ f(r),
// f(r) = ((r>>1 ^ r>>3) & 1) | ((r>>2 & 1) << 1), applied to the DMA source address: the
// ds_read_b128 of 16 consecutive rows at one logical chunk touches 16 distinct 16-B bank slots of
// 256 B, and that of 8 consecutive rows 8 distinct slots of 128 B. Rows past N and columns past V
// are clamped loads (row N − 1, column V − 1): never stored, masked in the epilogue.
//
// Epilogue per column tile, on the accumulators: bias, columns >= V to −inf (weight exactly 0, never
// the maximum), the lane's tile maximum, the online (m, s = Σ exp(x − m)) with s rescaled only when
// m moves, the best (value, lowest id) rescanned only when the tile maximum beats it, and the
// target logit captured by comparing column ids only in lanes whose target lies in this tile.
//
// After the sweep the two half-waves of a row are combined (lower columns first) and the partial
// (m, s, best, best id, x_target or −inf) goes to [S][N] buffers; a merge kernel, one wave per
// row, folds the S partials in a fixed order (one thread per row took 330 µs over 393 splits). No
// atomics, no workgroup waits for another: a grid larger than the machine runs in rounds. The result
// is bitwise reproducible, and a row's result does not depend on which rows share its tile: every
// output element of an MFMA is its own fixed chain over k, and all reductions of a row run in a
// fixed order over its own values. The same row scored within another N — in the 128-row or the
// 256-row form — gives the same bits as long as S is the same.
//
// Top-n form (top_n in 1..20, ops/prompt_logprobs.py's top_n): the same sweep also keeps, per row, the n
// best (logit, lowest id first) columns of the range in an LDS list behind the ring, selected in the tile
// epilogue on the accumulators (see lmhead_lse_kernel's TN), and the merge kernel folds the S lists of a
// row to ids [N, n] and logprobs [N, n]. It runs the 128-row tile at every N (68.5 KiB of LDS, two
// workgroups per CU), its three plain outputs are bitwise those of the plain launch at the same S, its
// entry 0 is (top_token, top_logprob) bitwise, and the guarantees above hold for the lists as well. With
// top_n = 0 the launcher starts exactly the kernels of before (the TN = 0 / TOPN = false instantiations).
#include "attn_common.h"
#include "host_plan.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {
namespace {

constexpr int LL_BN = kLmheadColTile, LL_BK = kLmheadKStep, LL_NBUF = 3;
constexpr int LL_W_TILE = LL_BN * LL_BK * 2;  // 8 KiB: one stage of W
static_assert(LL_BN == 128 && LL_BK == 32, "the lane maps below are written for 128-column tiles of 32 k");

template <int N_>
__device__ __forceinline__ void ll_vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory");
}

// physical 16-B chunk = logical chunk ^ ll_swz(tile row)
__device__ __forceinline__ int ll_swz(int r) { return (((r >> 1) ^ (r >> 3)) & 1) | (((r >> 2) & 1) << 1); }

__device__ __forceinline__ uint4 ll_read16(const char* base, unsigned off) {
  return *reinterpret_cast<const uint4*>(base + off);
}

// exp(d) for d <= 0 (−inf gives 0)
__device__ __forceinline__ float ll_exp(float d) { return __builtin_amdgcn_exp2f(d * kLog2e); }

// Top-n keys: (the logit's bits mapped so that unsigned order is float order, ~column id) in one 64-bit
// word — one total order, larger = better, the lowest id first among equal logits (−0 counts as +0, as a
// float compare does). 0 is the empty slot: below every real key (−inf maps to 0x007fffff).
using ll_key_t = unsigned long long;
__device__ __forceinline__ ll_key_t ll_key(float x, int col) {
  unsigned u = __float_as_uint(x == 0.f ? 0.f : x);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((ll_key_t)u << 32) | (unsigned)~col;
}
__device__ __forceinline__ float ll_key_value(ll_key_t k) {
  const unsigned u = (unsigned)(k >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ void ll_wave_fence() {  // LDS written by one half-wave, read by the other
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// partials: pf [4][S][N] fp32 (m, s, best, x_target), pid [S][N] int32 (best id)
//
// TN > 0 (the top-n form, RB = 1): the launch also keeps each row's topn <= TN best keys of this vocabulary
// range. Behind the ring sit the lists, [TN][128 rows] keys (consecutive rows in consecutive 8-B slots: no
// bank conflict) sorted best first, and their fill counts [128]; a row's list belongs to its wave alone
// (lanes l and l + 32), so no barrier guards it. A lane carries its row's count, n-th key (0 until the list
// is full) and that key's logit tv. Per column tile a lane whose tile maximum is below tv is done: none of
// its 64 columns can enter; a wave with no other lane skips the rest. Otherwise the wave walks its 64
// accumulator registers (a rolled loop, the register picked by a scalar index) with one compare x >= tv
// each. Where a lane passes, the two half-waves take turns (the lower columns first): reload count and n-th
// key (the other half may just have moved them), build the key and compare it exactly, and insert a key
// that beats the n-th by shifting the worse keys down one slot, a divergent loop over LDS; then every
// lane of the wave reloads its row's threshold, so tv is never stale. Which keys
// a list holds after a tile does not depend on the order they were offered in (keys are distinct, and the
// n best of a set is one set), so the result is that of the definition whatever the divergence does. Past
// the first tiles a row sees about n / t insertions in its t-th tile. The partial lists go to
// plist [S][N][topn], empty slots 0. The −inf columns >= V of the ragged last tile are offered like any
// other: every real column beats them (a higher logit, or −inf with a lower id), so they only ever sit in
// slots that would otherwise be empty, and the merge kernel drops them by their id.
template <int RB, bool BIAS, int TN = 0>
__global__ void __launch_bounds__(256, 2) lmhead_lse_kernel(const bf16* __restrict__ H, const bf16* __restrict__ W,
                                                            const float* __restrict__ bias,
                                                            const int64_t* __restrict__ targets, float* __restrict__ pf,
                                                            int* __restrict__ pid, int N, int V, int C, int ldh, int ldw,
                                                            int tiles_m, int splits, int tiles_per,
                                                            ll_key_t* __restrict__ plist, int topn) {
  static_assert(TN == 0 || RB == 1, "the top-n lists are laid out for the 128-row tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BM = 128 * RB;
  constexpr int H_TILE = BM * LL_BK * 2;
  constexpr int STAGE = H_TILE + LL_W_TILE;
  constexpr int HP = 2 * RB;     // h pieces (16 rows × 64 B) per wave and stage
  constexpr int G = HP + 2;      // LDS-DMA instructions per wave and stage
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5, l32 = lane & 31;

  // workgroups of one XCD (blockIdx & 7) take consecutive work items; the row tile runs fastest
  const int GX = gridDim.x >> 3;  // the grid is a multiple of 8 (host)
  const int item = (blockIdx.x & 7) * GX + (blockIdx.x >> 3);
  if (item >= tiles_m * splits) return;
  const int tm = item % tiles_m, sp = item / tiles_m;
  const int m0 = tm * BM;
  const int ct0 = sp * tiles_per, ct1 = min(ct0 + tiles_per, (V + LL_BN - 1) / LL_BN);
  const int KS = C / LL_BK;

  // LDS-DMA lane maps: lane -> row (lane >> 2) of a 16-row piece, physical chunk (lane & 3)
  unsigned hoff[HP], woff[2];
#pragma unroll
  for (int i = 0; i < HP; ++i) {
    const int row = 16 * (HP * w + i) + (lane >> 2);
    const int c = (lane & 3) ^ ll_swz(row);
    hoff[i] = (unsigned)min(m0 + row, N - 1) * (unsigned)ldh * 2u + (unsigned)c * 16u;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = 16 * (2 * w + i) + (lane >> 2);
    woff[i] = (unsigned)row * (unsigned)ldw * 2u + (unsigned)(((lane & 3) ^ ll_swz(row)) * 16);
  }
  const unsigned lds_base = (unsigned)(size_t)(lds_void_t*)smem;

  int d_ct = ct0, d_k = 0;  // DMA stream state (scalar)
  auto dma = [&](int stage) {
    const unsigned lh = __builtin_amdgcn_readfirstlane(lds_base + stage * STAGE + HP * w * 1024);
    const unsigned lw = __builtin_amdgcn_readfirstlane(lds_base + stage * STAGE + H_TILE + 2 * w * 1024);
    const int n0 = d_ct * LL_BN;
    const char* sh = reinterpret_cast<const char*>(H + d_k);
    const char* sw = reinterpret_cast<const char*>(W + (size_t)n0 * ldw + d_k);
#pragma unroll
    for (int i = 0; i < HP; ++i) glds16_s(sh, hoff[i], lh + i * 1024);
    if (n0 + LL_BN <= V) {
#pragma unroll
      for (int i = 0; i < 2; ++i) glds16_s(sw, woff[i], lw + i * 1024);
    } else {  // the ragged last column tile: rows past V re-read row V - 1 (masked in the epilogue)
      const int nmax = V - 1 - n0;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = 16 * (2 * w + i) + (lane >> 2);
        const unsigned o = woff[i] - (unsigned)(row - min(row, nmax)) * (unsigned)ldw * 2u;
        glds16_s(sw, o, lw + i * 1024);
      }
    }
    // advance; the stream stops at the last tile's last k-step: later issues re-load it (nobody
    // reads those stages), which keeps every wave's vmcnt arithmetic uniform
    if (d_k + LL_BK < C) {
      d_k += LL_BK;
    } else if (d_ct + 1 < ct1) {
      d_k = 0;
      ++d_ct;
    }
  };

  // fragment reads: lane -> tile row (lane & 31) of a 32-row block, logical chunk 2 kk + (lane >> 5)
  const unsigned fl0 = (unsigned)(l32 * 64 + ((half ^ ll_swz(l32)) << 4));
  const unsigned fh = fl0 + (unsigned)(32 * RB * w) * 64u;
  const unsigned fw = fl0 + (unsigned)H_TILE;

  // per-row running state: this lane's columns of row m0 + 32 (RB w + i) + (lane & 31)
  float rm[RB], rs[RB], rbest[RB], rxt[RB];
  int rid[RB], rtgt[RB];
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    rm[i] = -INFINITY, rs[i] = 0.f, rbest[i] = -INFINITY, rxt[i] = -INFINITY, rid[i] = 0x7fffffff;
    const int64_t t = targets[min(m0 + 32 * (RB * w + i) + l32, N - 1)];
    PZ_DEVICE_CHECK(t >= 0 && t < V);
    rtgt[i] = (int)t;
    asm volatile("" : "+v"(rtgt[i]));  // the load is waited for here, not inside the counted loop
  }

  // top-n state of this lane's row (tile row lrow): fill count, n-th key (0: not full), its logit
  ll_key_t* const lst = reinterpret_cast<ll_key_t*>(smem + LL_NBUF * STAGE);  // [TN][BM]
  int* const lcnt = reinterpret_cast<int*>(lst + TN * BM);                     // [BM]
  const int lrow = 32 * w + l32;
  int tcnt = 0;
  ll_key_t thr = 0;
  float tv = -INFINITY;
  auto top_reload = [&]() {
    tcnt = lcnt[lrow];
    thr = tcnt == topn ? lst[(topn - 1) * BM + lrow] : 0;
    tv = tcnt == topn ? ll_key_value(thr) : -INFINITY;
  };
  if constexpr (TN > 0) {
    if (half == 0) lcnt[lrow] = 0;
    ll_wave_fence();
  }

  // the accumulators of a column tile start from its bias (or 0): column of acc[i][j][r] =
  // n0 + 4 (lane >> 5) + 32 j + 8 (r >> 2) + (r & 3). The bias is the launcher's fp32 copy, padded with
  // zeros to whole column tiles and one tile more (the init after a range's last tile reads on)
  f32x16 acc[RB][4];
  auto acc_init = [&](int n0) {
    const float* bp = bias + n0 + 4 * half;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float4_t b = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BIAS) b = *reinterpret_cast<const float4_t*>(bp + 32 * j + 8 * q);
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] = b[e];
      }
  };
  acc_init(ct0 * LL_BN);

  // prologue: stages 0, 1 in flight, wait for stage 0
  dma(0);
  dma(1);
  ll_vm_wait<G>();
  __builtin_amdgcn_s_barrier();

  int cur = 0;  // ring position of the stage being read
  for (int ct = ct0; ct < ct1; ++ct) {
    const int n0 = ct * LL_BN;
    for (int ks = 0; ks < KS; ++ks) {
      dma(cur >= 1 ? cur - 1 : LL_NBUF - 1);  // (cur + 2) % 3: the stage read in the step before
      const char* stg = smem + cur * STAGE;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        uint4 wf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wf[j] = ll_read16(stg, (fw + j * 2048) ^ (kk << 5));
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          const uint4 hf = ll_read16(stg, (fh + i * 2048) ^ (kk << 5));
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = mfma32(wf[j], hf, acc[i][j]);
        }
      }
      if (ks == KS - 1) {
        // ---- epilogue: column of acc[i][j][r] = cb + 32 j + 8 (r >> 2) + (r & 3)
        const bool edge = n0 + LL_BN > V;
        const int cb = n0 + 4 * half;
#pragma unroll
        for (int i = 0; i < RB; ++i) {
          float cm = -INFINITY;
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const int col = cb + 32 * j + 8 * (r >> 2) + (r & 3);
              float x = acc[i][j][r];
              if (edge) x = col < V ? x : -INFINITY;
              acc[i][j][r] = x;
              cm = fmaxf(cm, x);
            }
          if (cm > rm[i]) {  // the sum is rescaled only when the maximum moves (m = −inf: s is 0 and stays 0)
            rs[i] *= ll_exp(rm[i] - cm);
            rm[i] = cm;
          }
          const float ms = rm[i] == -INFINITY ? 0.f : rm[i];  // a lane whose columns were all >= V so far
          float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) t4[r & 3] += ll_exp(acc[i][j][r] - ms);
          rs[i] += (t4[0] + t4[1]) + (t4[2] + t4[3]);
          if (cm > rbest[i]) {  // tiles ascend, so a later equal maximum never replaces an earlier one
            rbest[i] = cm;
            int id = 0;
#pragma unroll
            for (int j = 3; j >= 0; --j)
#pragma unroll
              for (int r = 15; r >= 0; --r)
                if (acc[i][j][r] == cm) id = cb + 32 * j + 8 * (r >> 2) + (r & 3);  // descending: the lowest stays
            rid[i] = id;
          }
          const int tl = rtgt[i] - cb;
          if (tl >= 0 && tl < LL_BN) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
              for (int r = 0; r < 16; ++r)
                if (tl == 32 * j + 8 * (r >> 2) + (r & 3)) rxt[i] = acc[i][j][r];
          }
          if constexpr (TN > 0) {
            const bool want = cm >= tv && m0 + lrow < N;  // (a clamped row keeps no list)
            if (__ballot(want)) {
#pragma unroll
              for (int j = 0; j < 4; ++j)
#pragma unroll 1
                for (int r = 0; r < 16; ++r) {  // rolled: one insertion body per block, the register picked by r
                  const float x = acc[i][j][r];
                  const bool pass = want && x >= tv;  // (a column >= V of the ragged tile is −inf and may enter: the merge drops it)
                  if (__ballot(pass)) {
#pragma unroll 1
                    for (int turn = 0; turn < 2; ++turn) {
                      if (pass && half == turn) {
                        top_reload();
                        const ll_key_t k = ll_key(x, cb + 32 * j + 8 * (r >> 2) + (r & 3));
                        if (k > thr) {
                          int s = min(tcnt, topn - 1);  // the slot that opens: a full list drops its n-th key
                          while (s > 0) {
                            const ll_key_t p = lst[(s - 1) * BM + lrow];
                            if (p > k) break;
                            lst[s * BM + lrow] = p;
                            --s;
                          }
                          lst[s * BM + lrow] = k;
                          lcnt[lrow] = min(tcnt + 1, topn);
                        }
                      }
                      ll_wave_fence();
                    }
                    top_reload();
                  }
                }
            }
          }
        }
        acc_init(n0 + LL_BN);
      }
      ll_vm_wait<G>();
      __builtin_amdgcn_s_barrier();
      cur = cur + 1 < LL_NBUF ? cur + 1 : 0;
    }
  }
  ll_vm_wait<0>();

  // the two half-waves of a row, lower columns first
  const size_t SN = (size_t)splits * N;
#pragma unroll
  for (int i = 0; i < RB; ++i) {
    const float om = __shfl_xor(rm[i], 32), os = __shfl_xor(rs[i], 32), ob = __shfl_xor(rbest[i], 32);
    const float ox = __shfl_xor(rxt[i], 32);
    const int oi = __shfl_xor(rid[i], 32);
    const int row = m0 + 32 * (RB * w + i) + l32;
    if (half == 0 && row < N) {
      const float M = fmaxf(rm[i], om);  // finite: the two halves cover every column of every tile
      const float s = rs[i] * ll_exp(rm[i] - M) + os * ll_exp(om - M);
      const bool take = ob > rbest[i] || (ob == rbest[i] && oi < rid[i]);
      const size_t o = (size_t)sp * N + row;
      pf[o] = M;
      pf[SN + o] = s;
      pf[2 * SN + o] = take ? ob : rbest[i];
      pf[3 * SN + o] = fmaxf(rxt[i], ox);
      pid[o] = take ? oi : rid[i];
    }
  }
  if constexpr (TN > 0) {  // the row's list, its two lanes taking alternate slots
    top_reload();
    if (m0 + lrow < N) {
      ll_key_t* out = plist + ((size_t)sp * N + m0 + lrow) * topn;
      for (int s = half; s < topn; s += 2) out[s] = s < tcnt ? lst[s * BM + lrow] : 0;
    }
  }
}

// one wave per row folds the S partials: lane l takes splits l, l + 64, ... in ascending order, then the 64
// lanes combine in the fixed order of wave_max / wave_sum (common.h) — the result depends on S alone
//
// TOPN: the wave also folds the row's S · topn partial keys to its topn best, kept sorted across the lanes
// (lane j holds the j-th best; the wave keeps 64, the first topn count). Lane l loads candidate 64 b + l
// of batch b; the few that beat the current topn-th key are taken in lane order, each inserted with one
// ballot (its rank = the lanes holding a better key) and one shift by a lane. Keys are distinct, so the
// result is the topn best of the set in the keys' order, whatever the partials' order was.
template <bool TOPN>
__global__ void __launch_bounds__(256) lmhead_lse_merge_kernel(const float* __restrict__ pf, const int* __restrict__ pid,
                                                               int N, int S, float* __restrict__ token_lp,
                                                               int64_t* __restrict__ top_id, float* __restrict__ top_lp,
                                                               float* __restrict__ x_t, float* __restrict__ lse_out,
                                                               const ll_key_t* __restrict__ plist, int topn, int V,
                                                               int64_t* __restrict__ n_id, float* __restrict__ n_lp) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;  // (a whole wave)
  const size_t SN = (size_t)S * N;
  float m = -INFINITY, best = -INFINITY, xt = -INFINITY;
  int id = 0x7fffffff;
  for (int k = lane; k < S; k += 64) {
    const size_t o = (size_t)k * N + row;
    m = fmaxf(m, pf[o]);
    const float b = pf[2 * SN + o];
    const int bi = pid[o];
    if (b > best || (b == best && bi < id)) best = b, id = bi;
    xt = fmaxf(xt, pf[3 * SN + o]);
  }
  const float M = wave_max(m);
  float s = 0.f;
  for (int k = lane; k < S; k += 64) {
    const size_t o = (size_t)k * N + row;
    s += pf[SN + o] * expf(pf[o] - M);
  }
  s = wave_sum(s);
  const float B = wave_max(best);
  id = best == B ? id : 0x7fffffff;  // the lowest id among the lanes that hold the maximum
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) id = min(id, __shfl_xor(id, off));
  xt = wave_max(xt);
  if (lane == 0) {
    const float lse = M + logf(s);
    token_lp[row] = xt - lse;
    top_id[row] = id;
    top_lp[row] = B - lse;
    x_t[row] = xt;
    lse_out[row] = lse;
  }
  if constexpr (TOPN) {
    const float lse = M + logf(s);  // (M and s are the same in every lane)
    ll_key_t mine = 0;
    unsigned long long nth = 0;  // lane topn - 1's key (wave-uniform)
    const int total = S * topn;
    constexpr int PF = 8;  // batches loaded together: S · topn / 64 dependent round trips otherwise (123 at 393 x 20)
    for (int c0 = 0; c0 < total; c0 += 64 * PF) {
      ll_key_t keys[PF];
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const int c = c0 + 64 * u + lane;
        keys[u] = c < total ? plist[((size_t)(c / topn) * N + row) * topn + c % topn] : 0;
      }
#pragma unroll
      for (int u = 0; u < PF; ++u) {
        const ll_key_t key = ~(unsigned)keys[u] < (unsigned)V ? keys[u] : 0;  // 0: a masked column of the ragged tile, an empty slot
        unsigned long long todo = __ballot(key > nth);
        while (todo) {
          const int src = __builtin_ctzll(todo);
          todo &= todo - 1;
          const ll_key_t k = ((ll_key_t)(unsigned)__builtin_amdgcn_readlane((int)(key >> 32), src) << 32) |
                             (unsigned)__builtin_amdgcn_readlane((int)key, src);
          if (k <= nth) continue;  // (nth rose since the ballot)
          const int rank = __popcll(__ballot(mine > k));
          const ll_key_t up = ((ll_key_t)(unsigned)__shfl_up((int)(mine >> 32), 1) << 32) | (unsigned)__shfl_up((int)mine, 1);
          mine = lane < rank ? mine : lane == rank ? k : up;
          nth = ((ll_key_t)(unsigned)__builtin_amdgcn_readlane((int)(mine >> 32), topn - 1) << 32) |
                (unsigned)__builtin_amdgcn_readlane((int)mine, topn - 1);
        }
      }
    }
    if (lane < topn) {  // entries past min(topn, V) stay empty: −1 / −inf
      n_id[(size_t)row * topn + lane] = mine ? (int64_t)(unsigned)~(unsigned)mine : -1;
      n_lp[(size_t)row * topn + lane] = mine ? ll_key_value(mine) - lse : -INFINITY;
    }
  }
}

}  // namespace
}  // namespace penroz

using namespace penroz;

std::tuple<int64_t, int64_t, int64_t> lmhead_lse_plan(int64_t N, int64_t V, int64_t C, int64_t splits, int64_t top_n) {
  const LmheadPlan p = plan_lmhead_lse(N, V, C, (int)std::max<int64_t>(0, std::min<int64_t>(splits, kLmheadMaxSplits)), top_n > 0);
  return {p.row_tile, p.splits, p.grid};
}

// h [N, C] bf16, w [V, C] bf16, bias [V] (any float type) or none, targets int64 [N] in [0, V)
// -> (token_logprob fp32 [N], top_token int64 [N], top_logprob fp32 [N], x_target fp32 [N], lse fp32 [N]).
// splits > 0 forces the number of vocabulary ranges (clamped to the column tiles): a row's bits depend on S,
// so a caller that compares rows across N pins it. The last two results are what the tests hold to the
// reference exactly (the target logit) and diagnostics; the merge kernel writes them on every call (2 N
// floats that lmhead_lse, the public triple, drops).
// top_n in 1..20: the top-n form (128-row tiles at every N), which appends (top_n_ids int64 [N, top_n],
// top_n_logprobs fp32 [N, top_n]): per row the min(top_n, V) most likely tokens, best first, the lowest id
// first among equal logits, then −1 / −inf. 0: exactly the launches of before.
std::vector<torch::Tensor> lmhead_lse_raw(torch::Tensor h, torch::Tensor w, c10::optional<torch::Tensor> bias,
                                          torch::Tensor targets, int64_t splits, int64_t top_n) {
  TORCH_CHECK(top_n >= 0 && top_n <= kLmheadTopCap, "lmhead_lse: top_n must be in [0, ", kLmheadTopCap, "], got ", top_n);
  TORCH_CHECK(h.is_cuda() && w.is_cuda() && targets.is_cuda(), "lmhead_lse: CUDA tensors");
  TORCH_CHECK(h.scalar_type() == torch::kBFloat16 && w.scalar_type() == torch::kBFloat16,
              "lmhead_lse: bf16 h and W only (fp16 / fp32 take ops.prompt_logprobs' torch path)");
  TORCH_CHECK(h.dim() == 2 && w.dim() == 2 && h.stride(1) == 1 && w.stride(1) == 1 && h.size(1) == w.size(1),
              "lmhead_lse: h [N, C] and W [V, C] with unit column stride");
  const int64_t N = h.size(0), C = h.size(1), V = w.size(0);
  TORCH_CHECK(targets.scalar_type() == torch::kInt64 && targets.dim() == 1 && targets.numel() == N,
              "lmhead_lse: targets int64 [N]");
  const LmheadPlan p = plan_lmhead_lse(N, V, C, (int)std::max<int64_t>(0, std::min<int64_t>(splits, kLmheadMaxSplits)), top_n > 0);
  TORCH_CHECK(p.row_tile != 0, "lmhead_lse: needs N >= 1, V >= 1 and C a multiple of ", kLmheadKStep, " in [",
              kLmheadKStep, ", ", kLmheadMaxC, "], got N = ", N, ", V = ", V, ", C = ", C);
  const int64_t ldh = N > 1 ? h.stride(0) : C, ldw = V > 1 ? w.stride(0) : C;
  TORCH_CHECK(ldh % 8 == 0 && ldw % 8 == 0 && ldh >= C && ldw >= C && reinterpret_cast<uintptr_t>(h.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0, "lmhead_lse: 16-B aligned rows");
  TORCH_CHECK(N * ldh * 2 < (1ll << 32) && (int64_t)kLmheadColTile * ldw * 2 < (1ll << 32),
              "lmhead_lse: h, and a column tile of W, must span < 4 GiB");
  auto fopt = h.options().dtype(torch::kFloat32);
  torch::Tensor bf;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->is_cuda() && bias->dim() == 1 && bias->numel() == V, "lmhead_lse: bias [V]");
    // fp32, zero-padded to whole column tiles and one more: the kernel reads it with unclamped 16-B loads
    bf = torch::zeros({((V + kLmheadColTile - 1) / kLmheadColTile + 1) * kLmheadColTile}, fopt);
    bf.narrow(0, 0, V).copy_(*bias);
  }
  auto tg = targets.contiguous();
  auto pf = torch::empty({4, p.splits, N}, fopt);
  auto pid = torch::empty({p.splits, N}, h.options().dtype(torch::kInt32));
  auto token_lp = torch::empty({N}, fopt), top_lp = torch::empty({N}, fopt), x_t = torch::empty({N}, fopt);
  auto lse = torch::empty({N}, fopt);
  auto top_id = torch::empty({N}, h.options().dtype(torch::kInt64));
  const int n = (int)top_n;
  torch::Tensor plist, n_id, n_lp;  // the partial lists [S, N, n] (64-bit keys) and the two top-n results
  if (n > 0) {
    plist = torch::empty({p.splits, N, n}, h.options().dtype(torch::kInt64));
    n_id = torch::empty({N, n}, h.options().dtype(torch::kInt64));
    n_lp = torch::empty({N, n}, fopt);
  }
  auto stream = at::hip::getCurrentHIPStream();
  const int tiles_m = (int)((N + p.row_tile - 1) / p.row_tile);
  const int lds1 = LL_NBUF * (128 * LL_BK * 2 + LL_W_TILE), lds2 = LL_NBUF * (256 * LL_BK * 2 + LL_W_TILE);
  const int ldsn = lds1 + 128 * (kLmheadTopCap * 8 + 4);  // the 128-row ring, the rows' lists and their counts: 68.5 KiB
  static bool attr_set = false;  // the 256-row ring (72 KiB) is beyond the 64 KiB a kernel gets unasked
  if (!attr_set) {
    auto allow = [](auto kern, int lds) {
      TORCH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      lds) == hipSuccess, "lmhead_lse: cannot reserve ", lds, " bytes of LDS");
    };
    allow(lmhead_lse_kernel<1, false>, lds1);
    allow(lmhead_lse_kernel<1, true>, lds1);
    allow(lmhead_lse_kernel<2, false>, lds2);
    allow(lmhead_lse_kernel<2, true>, lds2);
    allow(lmhead_lse_kernel<1, false, kLmheadTopCap>, ldsn);
    allow(lmhead_lse_kernel<1, true, kLmheadTopCap>, ldsn);
    attr_set = true;
  }
  auto launch = [&](auto kern, int lds) {
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(256), lds, stream, reinterpret_cast<const bf16*>(h.data_ptr()),
                       reinterpret_cast<const bf16*>(w.data_ptr()), bf.defined() ? bf.data_ptr<float>() : nullptr,
                       tg.data_ptr<int64_t>(), pf.data_ptr<float>(), pid.data_ptr<int>(), (int)N, (int)V, (int)C, (int)ldh,
                       (int)ldw, tiles_m, p.splits, p.tiles_per,
                       n > 0 ? reinterpret_cast<ll_key_t*>(plist.data_ptr<int64_t>()) : nullptr, n);
    TORCH_CHECK(hipGetLastError() == hipSuccess, "lmhead_lse: the kernel launch failed");
  };
  if (n > 0) {
    if (bf.defined()) launch(lmhead_lse_kernel<1, true, kLmheadTopCap>, ldsn);
    else launch(lmhead_lse_kernel<1, false, kLmheadTopCap>, ldsn);
  } else if (p.row_tile == 128) {
    if (bf.defined()) launch(lmhead_lse_kernel<1, true>, lds1);
    else launch(lmhead_lse_kernel<1, false>, lds1);
  } else {
    if (bf.defined()) launch(lmhead_lse_kernel<2, true>, lds2);
    else launch(lmhead_lse_kernel<2, false>, lds2);
  }
  auto merge = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, pf.data_ptr<float>(), pid.data_ptr<int>(),
                       (int)N, p.splits, token_lp.data_ptr<float>(), top_id.data_ptr<int64_t>(), top_lp.data_ptr<float>(),
                       x_t.data_ptr<float>(), lse.data_ptr<float>(),
                       n > 0 ? reinterpret_cast<const ll_key_t*>(plist.data_ptr<int64_t>()) : nullptr, n, (int)V,
                       n > 0 ? n_id.data_ptr<int64_t>() : nullptr, n > 0 ? n_lp.data_ptr<float>() : nullptr);
    TORCH_CHECK(hipGetLastError() == hipSuccess, "lmhead_lse: the merge kernel's launch failed");
  };
  if (n > 0) merge(lmhead_lse_merge_kernel<true>);
  else merge(lmhead_lse_merge_kernel<false>);
  if (n > 0) return {token_lp, top_id, top_lp, x_t, lse, n_id, n_lp};
  return {token_lp, top_id, top_lp, x_t, lse};
}

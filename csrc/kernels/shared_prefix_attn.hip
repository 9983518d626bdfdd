// Shared-prefix decode attention: one decode step of R rows that are R samples of ONE prompt. The prompt's
// K/V ("prefix", [1, Hkv, capP, D]) is stored once; every row keeps only the tokens it generated itself
// ("suffix", [R, Hkv, capS, D]). Row r's keys are the prefix keys followed by its own suffix keys, so
// decode_attn.hip on a replicated cache would read the prefix R times per step. Here every prefix key is
// read once per KV head and query tile, and the scores of all rows against it are one matrix product.
//
// Launch 1, one grid of 256-thread workgroups of two kinds; both write unnormalised fp32 partials
// (o[D], m, l) per (row, head) into a workspace [S + 1, R, H, ·]:
//   prefix workgroup = (KV head, query tile, key range s of S). The query rows of a KV head are the packed
//     pairs (row r, group head g), index r·G + g, BM = 32 / 64 / 128 of them per tile, 32 per wave (pad rows
//     load a clamped row and are never stored; waves without rows only stage). Range s is
//     [s·per, min(P, (s + 1)·per)) with per = ceil(ceil(P / 64) / S)·64 from the DEVICE-side prefix length, so
//     one captured graph balances every P over the S workgroups; a range that starts beyond P writes a
//     weight-0 partial (m at its finite floor, l = 0). K / V tiles of 64 keys (32 at D = 256) arrive by
//     LDS-DMA into the two-stage XOR-swizzled ring of prefill_attn.hip, dealt over all four waves;
//     Sᵀ = K·Qᵀ and Oᵀ += Vᵀ·Pᵀ run on v_mfma_f32_32x32x16_bf16 with that kernel's fragment maps, the
//     online softmax in exp2 with the rescale decided per row. No causal mask (every prefix key precedes
//     every query); keys at or beyond the range end are masked, which only the last tile of P meets.
//   suffix workgroup = (row, KV head): writes the row's new K / V (raw 16-B pieces of the QKV row) into
//     suffix slot len − 1 − P (len: one for all rows, or every row its own — rows whose remainders behind the
//     prefix differ in length), then attends the row's len − P suffix keys as decode_attn.hip does — one key
//     per thread, chunks of up to 256 keys, V through LDS — for the G heads of the group: partial number S.
// Launch 2 folds the S + 1 partials of every (row, head) in index order and writes bf16.
// No atomics, no arrival counters, no waiting between workgroups: bitwise reproducible, and a row's bits
// depend on its own q, the prefix, its suffix, P and S only — not on R or on the other rows' values.
// The prefill form (shared_prefix_prefill_kernel, below) serves Tq query positions per row with the same partials
// and the same merge.
#include "attn_common.h"
#include "launch_args.h"
#include "shared_prefix_common.h"
#include <torch/extension.h>
#include <utility>
#include <vector>
#include <ATen/hip/HIPContext.h>

namespace penroz {
namespace {

constexpr int sp_suffix_keys(int D) { return D * 2 * 256 <= 32768 ? 256 : 32768 / (D * 2); }  // keys per chunk
constexpr int sp_suffix_lds(int D) { return 32768 + kSpGroup * D * 4 + kSpGroup * sp_suffix_keys(D) * 4 + 80 * 4; }
constexpr int sp_prefix_lds(int D, int NWQ) {
  return 4 * prefill_keys(D) * 128 * (D / 64) + (D >= 256 ? 32 * NWQ * 128 * (D / 64) : 0) + 16;
}

// ---- suffix workgroup: row b, KV head g ------------------------------------------------------------
template <int D>
__device__ __forceinline__ void sp_suffix(char* smem, const bf16* __restrict__ q, const bf16* __restrict__ k_new,
                                          const bf16* __restrict__ v_new, bf16* __restrict__ ksuf,
                                          bf16* __restrict__ vsuf, float* __restrict__ ws_o, float* __restrict__ ws_ml,
                                          int b, int g, int R, int H, int Hkv, int G, int capS, int n_suf, float c,
                                          int64_t q_rs, int64_t kv_rs, int S) {
  constexpr int GMAX = kSpGroup;
  constexpr int RB = D * 2;                    // cache row bytes
  constexpr int KC = sp_suffix_keys(D);        // keys per chunk (V chunk <= 32 KB of LDS)
  constexpr int TPK = 256 / KC;                // threads per key in the score phase
  constexpr int CR = RB / 16, CPT = CR / TPK;  // 16-B pieces per row, and per thread
  constexpr int SW = 7;                        // LDS row swizzle mask (pieces)
  constexpr int NP2 = D / 2, NG = 256 / NP2;   // P·V: column pairs × key groups
  constexpr int QPT = GMAX * D / 256;
  static_assert(CPT == 8 && NG * NP2 == 256 && NG * GMAX * D * 4 <= 32768, "suffix tiling");
  char* vbuf = smem;  // V chunk, later the P·V partials
  float* qs = reinterpret_cast<float*>(smem + 32768);  // [GMAX][D]
  float* pl = qs + GMAX * D;                            // [GMAX][KC]
  float* red_m = pl + GMAX * KC;                        // [4][GMAX]
  float* red_l = red_m + 4 * GMAX;                      // [4][GMAX]
  float* fin = red_l + 4 * GMAX;                        // [GMAX][2]

  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  float qv[QPT];
#pragma unroll
  for (int r = 0; r < QPT; ++r) {
    const int i = t + 256 * r;
    qv[r] = i < G * D ? bf2f(q[(size_t)b * q_rs + (size_t)(g * G + i / D) * D + i % D]) : 0.f;
  }
  const int k1 = n_suf;  // keys 0 .. n_suf − 1; the last one is this step's
  const size_t head_base = ((size_t)b * Hkv + g) * capS;
  const size_t new_off = (size_t)b * kv_rs + (size_t)g * D;
  const int kk = t / TPK, part = t % TPK;
  const int kg = t / NP2, d0 = 2 * (t % NP2);
  sp_u32x4 kr[CPT], vr[CPT];
  auto load_chunk = [&](int c0) {
    const int key = c0 + kk;
    const size_t row = head_base + (key < k1 ? key : c0);
    const bool fresh = key == k1 - 1;  // pointer select, no branch
    const char* ksrc = reinterpret_cast<const char*>(fresh ? k_new + new_off : ksuf + row * D) + part * CPT * 16;
    const char* vsrc = reinterpret_cast<const char*>(fresh ? v_new + new_off : vsuf + row * D) + part * CPT * 16;
#pragma unroll
    for (int x = 0; x < CPT; ++x) kr[x] = *reinterpret_cast<const sp_u32x4*>(ksrc + 16 * x);
#pragma unroll
    for (int x = 0; x < CPT; ++x) vr[x] = *reinterpret_cast<const sp_u32x4*>(vsrc + 16 * x);
  };
  load_chunk(0);
#pragma unroll
  for (int r = 0; r < QPT; ++r) {
    const int i = t + 256 * r;
    if (i < G * D) qs[i] = qv[r] * c;  // scores come out in log2 units
  }
  __syncthreads();

  float M[GMAX], L[GMAX], o[GMAX][2], s[GMAX];
#pragma unroll
  for (int i = 0; i < GMAX; ++i) {
    M[i] = kSpFloor;
    L[i] = 0.f;
    o[i][0] = o[i][1] = 0.f;
  }
  for (int c0 = 0; c0 < k1; c0 += KC) {
    const bool valid = c0 + kk < k1;
    if (c0 + kk == k1 - 1) {  // this step's K / V row into its slot, the bits the QKV row holds
      const size_t row = head_base + (k1 - 1);
#pragma unroll
      for (int x = 0; x < CPT; ++x) {
        *reinterpret_cast<sp_u32x4*>(reinterpret_cast<char*>(ksuf + row * D) + part * CPT * 16 + 16 * x) = kr[x];
        *reinterpret_cast<sp_u32x4*>(reinterpret_cast<char*>(vsuf + row * D) + part * CPT * 16 + 16 * x) = vr[x];
      }
    }
#pragma unroll
    for (int x = 0; x < CPT; ++x) {
      const int pc = part * CPT + x;
      *reinterpret_cast<sp_u32x4*>(vbuf + kk * RB + ((pc ^ (kk & SW)) << 4)) = vr[x];
    }
#pragma unroll
    for (int i = 0; i < GMAX; ++i) {
      if (i >= G) break;
      float a = 0.f;
#pragma unroll
      for (int x = 0; x < CPT; ++x) {
        const uint32_t w4[4] = {kr[x].x, kr[x].y, kr[x].z, kr[x].w};
        const float* qp = qs + i * D + (part * CPT + x) * 8;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a += qp[2 * e] * __uint_as_float(w4[e] << 16);
          a += qp[2 * e + 1] * __uint_as_float(w4[e] & 0xffff0000u);
        }
      }
#pragma unroll
      for (int x = 1; x < TPK; x <<= 1) a += __shfl_xor(a, x, 64);
      s[i] = valid ? a : -INFINITY;
      const float wm = wave_max(s[i]);
      if (lane == 0) red_m[wid * GMAX + i] = wm;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < GMAX; ++i) {
      if (i >= G) break;
      const float cm = fmaxf(fmaxf(red_m[i], red_m[GMAX + i]), fmaxf(red_m[2 * GMAX + i], red_m[3 * GMAX + i]));
      const float mn = fmaxf(M[i], cm);  // finite: every chunk holds a valid key
      const float alpha = fexp2(M[i] - mn);
      const float p = valid ? fexp2(s[i] - mn) : 0.f;
      if (part == 0) pl[i * KC + kk] = p;
      const float wsum = wave_sum(part == 0 ? p : 0.f);
      if (lane == 0) red_l[wid * GMAX + i] = wsum;
      M[i] = mn;
      s[i] = alpha;
    }
    if (c0 + KC < k1) load_chunk(c0 + KC);  // prefetch: lands while this chunk's P·V runs
    __syncthreads();
    const int nv = min(KC, k1 - c0);
#pragma unroll
    for (int i = 0; i < GMAX; ++i) {
      if (i >= G) break;
      L[i] = L[i] * s[i] + (red_l[i] + red_l[GMAX + i]) + (red_l[2 * GMAX + i] + red_l[3 * GMAX + i]);
      o[i][0] *= s[i];
      o[i][1] *= s[i];
    }
    const int bo = d0 * 2;
#pragma unroll 8
    for (int j = kg; j < nv; j += NG) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(vbuf + j * RB + ((((bo >> 4) ^ (j & SW))) << 4) + (bo & 15));
      const float v0 = __uint_as_float(w << 16), v1 = __uint_as_float(w & 0xffff0000u);
#pragma unroll
      for (int i = 0; i < GMAX; ++i) {
        if (i >= G) break;
        const float pw = pl[i * KC + j];
        o[i][0] += pw * v0;
        o[i][1] += pw * v1;
      }
    }
    __syncthreads();
  }
  // merge the NG key groups (partials reuse the V buffer), then partial number S
  float* ro = reinterpret_cast<float*>(vbuf);
#pragma unroll
  for (int i = 0; i < GMAX; ++i) {
    if (i >= G) break;
    *reinterpret_cast<float2*>(ro + (kg * GMAX + i) * D + d0) = make_float2(o[i][0], o[i][1]);
    if (t == 0) {
      fin[2 * i] = M[i];
      fin[2 * i + 1] = L[i];
    }
  }
  __syncthreads();
  for (int idx = t; idx < G * D; idx += 256) {
    const int i = idx / D, d = idx % D;
    float O = 0.f;
#pragma unroll
    for (int x = 0; x < NG; ++x) O += ro[(x * GMAX + i) * D + d];
    const size_t r = ((size_t)S * R + b) * H + g * G + i;
    ws_o[r * D + d] = O;
    if (d == 0) {
      ws_ml[2 * r] = fin[2 * i];
      ws_ml[2 * r + 1] = fin[2 * i + 1];
    }
  }
}

// ---- launch 1 --------------------------------------------------------------------------------------
// NWQ: waves of a prefix workgroup that own query rows (tile height BM = 32·NWQ); all four waves stage.
template <int D, int NWQ>
__global__ void __launch_bounds__(256)
    shared_prefix_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k_new, const bf16* __restrict__ v_new,
                         const bf16* __restrict__ kp, const bf16* __restrict__ vp, bf16* __restrict__ ksuf,
                         bf16* __restrict__ vsuf, const int64_t* __restrict__ prefix_t,
                         const int64_t* __restrict__ len_t, int len_stride, float* __restrict__ ws_o,
                         float* __restrict__ ws_ml, int R, int Hkv, int gs, int capP, int capS, int S, int nqt, float scale,
                         int64_t q_rs, int64_t kv_rs) {
  constexpr int NP = D / 64, NS = D / 16, ND = D / 32, BM = 32 * NWQ, NW = 4;
  constexpr bool QLDS = D >= 256;  // as in prefill_attn.hip: the tile's query rows sit in LDS, 32-key tiles
  constexpr int BN = prefill_keys(D), NH = BN / 32;
  constexpr int TILE = BN * 128 * NP;
  constexpr int PLDS = sp_prefix_lds(D, NWQ), SLDS = sp_suffix_lds(D);
  __shared__ __attribute__((aligned(16))) char smem[PLDS > SLDS ? PLDS : SLDS];

  const int G = 1 << gs, H = Hkv << gs;
  const int P = (int)min<int64_t>(max<int64_t>(prefix_t[0], 0), (int64_t)capP);
  const float c = scale * kLog2e;
  const int nprefix = Hkv * nqt * S;
  if ((int)blockIdx.x >= nprefix) {
    const int item = blockIdx.x - nprefix, b = item / Hkv, g = item % Hkv;
    // the row's own keys, this step's included; a length outside the suffix cache never leaves it. len_stride 1:
    // every row its own length (rows whose remainders differ, ops/shared_prefix.py); 0: one for all
    const int n_suf = (int)min<int64_t>(max<int64_t>(len_t[(size_t)b * len_stride] - P, 1), (int64_t)capS);
    sp_suffix<D>(smem, q, k_new, v_new, ksuf, vsuf, ws_o, ws_ml, b, g, R, H, Hkv, G, capS, n_suf, c, q_rs, kv_rs, S);
    return;
  }
  const char* Qs = smem + 4 * TILE;
  const int sp = blockIdx.x % S, qt = (blockIdx.x / S) % nqt, hk = blockIdx.x / (S * nqt);
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id(), hh = lane >> 5;

  // this lane's query row: packed index r·G + g of the KV head
  const int pr = qt * BM + 32 * w + (lane & 31);
  const int row = pr >> gs, head = (hk << gs) + (pr & (G - 1));
  const bool valid = w < NWQ && row < R;
  const bool wact = w < NWQ && ((qt * BM + 32 * w) >> gs) < R;  // wave-uniform: the wave owns real rows
  // this workgroup's keys [k0, k1): the bounds come from the device-side length
  const int per = ((((P + 63) >> 6) + S - 1) / S) << 6;
  const int k0 = sp * per, k1 = min(P, k0 + per);
  const int ntk = k1 > k0 ? (k1 - k0 + BN - 1) / BN : 0;

  uint4 qf[QLDS ? 1 : NS];
  if constexpr (QLDS) {
    if (w < NWQ) {
      const unsigned qdst = __builtin_amdgcn_readfirstlane(lds_addr_of(Qs)) + 32 * w * 128;
      const int rr = lane >> 3;
#pragma unroll
      for (int r8 = 0; r8 < 4; ++r8) {
        const int rq = qt * BM + 32 * w + 8 * r8 + rr;
        const bf16* src = q + (size_t)min(rq >> gs, R - 1) * q_rs + (size_t)((hk << gs) + (rq & (G - 1))) * D;
        const int lc = (lane & 7) ^ sp_swz(8 * (r8 & 1) + rr);
#pragma unroll
        for (int p = 0; p < NP; ++p) glds16(src + 64 * p + 8 * lc, qdst + (p * BM + 8 * r8) * 128);
      }
    }
  } else {
    const bf16* qrow = q + (size_t)(valid ? row : 0) * q_rs + (size_t)head * D;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = valid ? *reinterpret_cast<const uint4*>(qrow + 16 * s + 8 * hh) : zero4();
#pragma unroll
    for (int s = 0; s < NS; ++s) launder(qf[s]);
  }
  auto qfrag = [&](int s) -> uint4 {
    if constexpr (QLDS) return row_frag(Qs + (s >> 2) * BM * 128, 32 * w, s & 3, lane);
    else return qf[s];
  };

  f32x16 o[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[j][i] = 0.f;
  float m = kSpFloor, l = 0.f;

  // LDS-DMA of tile j's K and V: 2·NP·BN/8 pieces (8 rows × 128 B) dealt over the four waves; rows at or
  // beyond P load row P − 1 (finite data under P = 0 weights; nothing beyond the cache is read)
  const bf16* kb = kp + (size_t)hk * capP * D;
  const bf16* vb = vp + (size_t)hk * capP * D;
  auto dma = [&](int j) {
    const unsigned stage = __builtin_amdgcn_readfirstlane(lds_addr_of(smem + (j & 1) * 2 * TILE));
    const int ln = opaque_lane_id(), rr = ln >> 3;
#pragma unroll
    for (int t = 0; t < 2 * NP * (BN / 8) / NW; ++t) {
      const int idx = t * NW + w;  // wave-uniform: matrix, panel, 8-row slab
      const int r8 = idx % (BN / 8), p = (idx / (BN / 8)) % NP, mtx = idx / (BN / 8 * NP);
      const int lc = (ln & 7) ^ sp_swz(8 * (r8 & 1) + rr);
      const int krow = max(min(k0 + j * BN + 8 * r8 + rr, P - 1), 0);
      glds16_s(mtx ? vb : kb, (unsigned)(krow * D + 64 * p + 8 * lc) * 2u, stage + mtx * TILE + (p * BN + 8 * r8) * 128);
    }
  };
  if (ntk > 0) dma(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the first tile's DMA, and the Q image's
  __syncthreads();

  for (int j = 0; j < ntk; ++j) {
    if (j + 1 < ntk) dma(j + 1);  // its stage was released by the previous iteration's barrier
    const char* Kt = smem + (j & 1) * 2 * TILE;
    const char* Vt = Kt + TILE;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {  // the tile's 32-key halves, one online-softmax step each
      const int kh0 = k0 + j * BN + 32 * hf;
      if (wact && kh0 < k1) {  // wave-uniform
        f32x16 st;
#pragma unroll
        for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          st = mfma32(row_frag(Kt + (s >> 2) * BN * 128, 32 * hf, s & 3, lane), qfrag(s), st);
          if constexpr (D >= 256)
            if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // keep few LDS fragments in flight
        }
        auto softmax = [&](auto mask_tag) {
          constexpr bool MASK = decltype(mask_tag)::value;
          float tmax = -INFINITY;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            float s = st[i];
            if constexpr (MASK) s = kh0 + acc_row(i, lane) >= k1 ? -INFINITY : s;
            st[i] = s;
            tmax = fmaxf(tmax, s);
          }
          tmax = halves_max(tmax) * c;  // finite: the half holds key kh0 < k1
          const float mnew = tmax > m + kRescaleThr ? tmax : m;
          if (!__all(mnew == m)) {
            const float alpha = mnew == m ? 1.f : fexp2(m - mnew);
            l *= alpha;
#pragma unroll
            for (int jd = 0; jd < ND; ++jd)
#pragma unroll
              for (int i = 0; i < 16; ++i) o[jd][i] *= alpha;
          }
          m = mnew;
          const float negm = -m;
          float lsum = 0.f;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float p = fexp2(fmaf(st[i], c, negm));
            lsum += p;
            st[i] = p;
          }
          l += lsum;
        };
        if (kh0 + 32 > k1) softmax(std::true_type{});  // the range's last, partial half
        else softmax(std::false_type{});
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
          const uint4 pf = acc_frag(st, ss);
#pragma unroll
          for (int jd = 0; jd < ND; ++jd) {
            o[jd] = mfma32(tr_frag(Vt + (jd >> 1) * BN * 128, 32 * hf + 16 * ss, 32 * (jd & 1), lane), pf, o[jd]);
            if constexpr (D >= 256)
              if (jd & 1) __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  l = halves_sum(l);
  if (valid) {  // partial number sp of (row, head): weight 0 (m at the floor, l = 0) when the range is empty
    const size_t r = ((size_t)sp * R + row) * H + head;
    float* orow = ws_o + r * D;
#pragma unroll
    for (int jd = 0; jd < ND; ++jd)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *reinterpret_cast<float4_t*>(orow + 32 * jd + 8 * g4 + 4 * hh) =
            float4_t{o[jd][4 * g4], o[jd][4 * g4 + 1], o[jd][4 * g4 + 2], o[jd][4 * g4 + 3]};
    if (hh == 0) {
      ws_ml[2 * r] = m;
      ws_ml[2 * r + 1] = l;
    }
  }
}

// ---- the prefill form: Tq query positions per row ---------------------------------------------------
// R rows that share the prefix and differ behind it (ops/shared_prefix.py, ``share_prefix``): q [R, Tq, H, D] are
// the rows' remainders, query t of row r sees the P prefix keys and row r's own suffix slots 0..t, which are
// this call's new K / V. No prefix key needs a mask, so for the prefix every (row, position, group head) is one
// more packed query row, index (r·Tq + t)·G + g, and one staged prefix tile serves up to 128 of them drawn from
// all rows at once. One launch of 256-thread workgroups of three kinds:
//   prefix workgroup = (KV head, tile of BM packed rows, key range s of S), ranges as in the decode form;
//   suffix workgroup = (row, KV head, tile of BM packed (t, g) rows of that row), heaviest tiles first: causal
//     over the row's new keys 0..t, staged straight from the call's K / V rows (so it waits for no copy), key
//     tiles above the tile's last position never staged, steps above a wave's diagonal skipped, the mask
//     applied only in steps that cross it;
//   copy workgroup: the call's K / V rows, 16-B pieces, into suffix slots 0..Tq − 1 (the bits the QKV rows hold).
// Prefix and suffix workgroups run ONE tile body (sp_tile): 32·NWQ query rows against keys [k0, kend) of one K / V
// matrix, key i visible to a lane's row while i <= klast — the range's last key for a prefix workgroup, the row's
// own position for a suffix one. They write the unnormalised partials s (prefix) and S (suffix) of
// (row, position, head); shared_prefix_merge_kernel folds the S + 1 in index order. A row's bits depend on its
// own query, the prefix, its own keys 0..t, P and S: masked keys enter P·V with weight exactly 0, the rescale
// is decided per row, and nothing crosses rows.
template <int D, int NWQ, class QSrc>
__device__ __forceinline__ void sp_tile(char* smem, QSrc qsrc, bool valid, bool wact, int klast, int kminw, int kmaxw,
                                        const bf16* __restrict__ kb, const bf16* __restrict__ vb, int kstride, int k0,
                                        int kend, float c, float* __restrict__ orow, float* __restrict__ mlrow) {
  constexpr int NP = D / 64, NS = D / 16, ND = D / 32, BM = 32 * NWQ, NW = 4;
  constexpr bool QLDS = D >= 256;
  constexpr int BN = prefill_keys(D), NH = BN / 32;
  constexpr int TILE = BN * 128 * NP;
  const char* Qs = smem + 4 * TILE;
  const int lane = threadIdx.x & 63, w = wave_id(), hh = lane >> 5;
  const int ntk = kend > k0 ? (kend - k0 + BN - 1) / BN : 0;

  uint4 qf[QLDS ? 1 : NS];
  if constexpr (QLDS) {
    if (w < NWQ) {  // the wave's 32 rows by LDS-DMA (rows beyond the last: a clamped row, never stored)
      const unsigned qdst = __builtin_amdgcn_readfirstlane(lds_addr_of(Qs)) + 32 * w * 128;
      const int rr = lane >> 3;
#pragma unroll
      for (int r8 = 0; r8 < 4; ++r8) {
        const bf16* src = qsrc(32 * w + 8 * r8 + rr);
        const int lc = (lane & 7) ^ sp_swz(8 * (r8 & 1) + rr);
#pragma unroll
        for (int p = 0; p < NP; ++p) glds16(src + 64 * p + 8 * lc, qdst + (p * BM + 8 * r8) * 128);
      }
    }
  } else {
    const bf16* qrow = qsrc(32 * w + (lane & 31));
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = valid ? *reinterpret_cast<const uint4*>(qrow + 16 * s + 8 * hh) : zero4();
#pragma unroll
    for (int s = 0; s < NS; ++s) launder(qf[s]);
  }
  auto qfrag = [&](int s) -> uint4 {
    if constexpr (QLDS) return row_frag(Qs + (s >> 2) * BM * 128, 32 * w, s & 3, lane);
    else return qf[s];
  };

  f32x16 o[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[j][i] = 0.f;
  float m = kSpFloor, l = 0.f;

  // LDS-DMA of tile j's K and V over the four waves; rows at or beyond kend load row kend − 1 (finite data under
  // P = 0 weights: a NaN in an unused slot contributes nothing, and nothing beyond the keys in use is read)
  auto dma = [&](int j) {
    const unsigned stage = __builtin_amdgcn_readfirstlane(lds_addr_of(smem + (j & 1) * 2 * TILE));
    const int ln = opaque_lane_id(), rr = ln >> 3;
#pragma unroll
    for (int t = 0; t < 2 * NP * (BN / 8) / NW; ++t) {
      const int idx = t * NW + w;  // wave-uniform: matrix, panel, 8-row slab
      const int r8 = idx % (BN / 8), p = (idx / (BN / 8)) % NP, mtx = idx / (BN / 8 * NP);
      const int lc = (ln & 7) ^ sp_swz(8 * (r8 & 1) + rr);
      const int krow = max(min(k0 + j * BN + 8 * r8 + rr, kend - 1), 0);
      glds16_s(mtx ? vb : kb, (unsigned)(krow * kstride + 64 * p + 8 * lc) * 2u, stage + mtx * TILE + (p * BN + 8 * r8) * 128);
    }
  };
  if (ntk > 0) dma(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the first tile's DMA, and the Q image's
  __syncthreads();

  for (int j = 0; j < ntk; ++j) {
    if (j + 1 < ntk) dma(j + 1);  // its stage was released by the previous iteration's barrier
    const char* Kt = smem + (j & 1) * 2 * TILE;
    const char* Vt = Kt + TILE;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {
      const int kh0 = k0 + j * BN + 32 * hf;
      if (wact && kh0 <= kmaxw) {  // wave-uniform: some row of the wave sees a key of this half
        f32x16 st;
#pragma unroll
        for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          st = mfma32(row_frag(Kt + (s >> 2) * BN * 128, 32 * hf, s & 3, lane), qfrag(s), st);
          if constexpr (D >= 256)
            if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        auto softmax = [&](auto mask_tag) {
          constexpr bool MASK = decltype(mask_tag)::value;
          float tmax = -INFINITY;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            float s = st[i];
            if constexpr (MASK) s = kh0 + acc_row(i, lane) > klast ? -INFINITY : s;
            st[i] = s;
            tmax = fmaxf(tmax, s);
          }
          tmax = halves_max(tmax) * c;  // −inf for a row that sees no key of this half: its m stays, its p are 0
          const float mnew = tmax > m + kRescaleThr ? tmax : m;
          if (!__all(mnew == m)) {
            const float alpha = mnew == m ? 1.f : fexp2(m - mnew);
            l *= alpha;
#pragma unroll
            for (int jd = 0; jd < ND; ++jd)
#pragma unroll
              for (int i = 0; i < 16; ++i) o[jd][i] *= alpha;
          }
          m = mnew;
          const float negm = -m;
          float lsum = 0.f;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float p = fexp2(fmaf(st[i], c, negm));
            lsum += p;
            st[i] = p;
          }
          l += lsum;
        };
        if (kh0 + 31 > kminw) softmax(std::true_type{});  // the half crosses some row's last key
        else softmax(std::false_type{});
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
          const uint4 pf = acc_frag(st, ss);
#pragma unroll
          for (int jd = 0; jd < ND; ++jd) {
            o[jd] = mfma32(tr_frag(Vt + (jd >> 1) * BN * 128, 32 * hf + 16 * ss, 32 * (jd & 1), lane), pf, o[jd]);
            if constexpr (D >= 256)
              if (jd & 1) __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  l = halves_sum(l);
  if (valid) {  // weight 0 (m at the floor, l = 0) when the range is empty
#pragma unroll
    for (int jd = 0; jd < ND; ++jd)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
        *reinterpret_cast<float4_t*>(orow + 32 * jd + 8 * g4 + 4 * hh) =
            float4_t{o[jd][4 * g4], o[jd][4 * g4 + 1], o[jd][4 * g4 + 2], o[jd][4 * g4 + 3]};
    if (hh == 0) {
      mlrow[0] = m;
      mlrow[1] = l;
    }
  }
}

// nqt: prefix query tiles per KV head; nst: suffix query tiles per (row, KV head); ncopy: copy workgroups
template <int D, int NWQ>
__global__ void __launch_bounds__(256)
    shared_prefix_prefill_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k_new, const bf16* __restrict__ v_new,
                                 const bf16* __restrict__ kp, const bf16* __restrict__ vp, bf16* __restrict__ ksuf,
                                 bf16* __restrict__ vsuf, const int64_t* __restrict__ prefix_t, float* __restrict__ ws_o,
                                 float* __restrict__ ws_ml, int R, int Tq, int Hkv, int gs, int capP, int capS, int S, int nqt,
                                 int nst, float scale, int64_t q_rs, int64_t kv_rs) {
  constexpr int BM = 32 * NWQ;
  __shared__ __attribute__((aligned(16))) char smem[sp_prefix_lds(D, NWQ)];
  const int G = 1 << gs, H = Hkv << gs, NR = R * Tq;  // NR: (row, position) pairs
  const int P = (int)min<int64_t>(max<int64_t>(prefix_t[0], 0), (int64_t)capP);
  const float c = scale * kLog2e;
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
  const int nprefix = Hkv * nqt * S, nsuffix = R * Hkv * nst;
  const int tr = 32 * w + (lane & 31);  // this lane's row of the tile
  int blk = blockIdx.x;

  if (blk < nprefix) {
    const int sp = blk % S, qt = (blk / S) % nqt, hk = blk / (S * nqt);
    const int pr = qt * BM + tr, pos = pr >> gs, head = (hk << gs) + (pr & (G - 1));
    const bool valid = w < NWQ && pos < NR;
    const bool wact = w < NWQ && ((qt * BM + 32 * w) >> gs) < NR;
    const int per = ((((P + 63) >> 6) + S - 1) / S) << 6;
    const int k0 = sp * per, k1 = min(P, k0 + per);
    auto qsrc = [&](int row) {
      const int x = qt * BM + row;
      return q + (size_t)min(x >> gs, NR - 1) * q_rs + (size_t)((hk << gs) + (x & (G - 1))) * D;
    };
    const size_t r = ((size_t)sp * NR + (valid ? pos : 0)) * H + head;
    sp_tile<D, NWQ>(smem, qsrc, valid, wact, k1 - 1, k1 - 1, k1 - 1, kp + (size_t)hk * capP * D, vp + (size_t)hk * capP * D,
                    D, k0, k1, c, ws_o + r * D, ws_ml + 2 * r);
    return;
  }
  blk -= nprefix;
  if (blk < nsuffix) {
    const int PT = BM >> gs;  // positions per tile
    const int qt = nst - 1 - blk / (R * Hkv), b = (blk % (R * Hkv)) / Hkv, hk = blk % Hkv;  // heaviest tiles first
    const int pl = qt * PT + (tr >> gs), head = (hk << gs) + (tr & (G - 1));
    const bool valid = w < NWQ && pl < Tq;
    const int pw0 = qt * PT + ((32 * w) >> gs);
    const bool wact = w < NWQ && pw0 < Tq;
    const int kend = min((qt + 1) * PT, Tq);  // keys this tile's rows can see
    auto qsrc = [&](int row) {
      return q + ((size_t)b * Tq + min(qt * PT + (row >> gs), Tq - 1)) * q_rs + (size_t)((hk << gs) + (row & (G - 1))) * D;
    };
    const size_t off = (size_t)b * Tq * kv_rs + (size_t)hk * D;  // row b's new keys: slot t is K / V row b·Tq + t
    const size_t r = ((size_t)S * NR + (size_t)b * Tq + (valid ? pl : 0)) * H + head;
    sp_tile<D, NWQ>(smem, qsrc, valid, wact, pl, pw0, min(pw0 + (32 >> gs), Tq) - 1, k_new + off, v_new + off, (int)kv_rs, 0,
                    kend, c, ws_o + r * D, ws_ml + 2 * r);
    return;
  }
  blk -= nsuffix;
  constexpr int CR = D / 8;  // 16-B pieces per K / V head row
  const int64_t npieces = (int64_t)NR * Hkv * CR;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int64_t i = ((int64_t)blk * 4 + x) * 256 + tid;
    if (i < npieces) {
      const int pc = (int)(i % CR), hk = (int)((i / CR) % Hkv);
      const int64_t rt = i / (CR * Hkv);
      const size_t src = (size_t)rt * kv_rs + (size_t)hk * D + 8 * pc;
      const size_t dst = (((size_t)(rt / Tq) * Hkv + hk) * capS + (size_t)(rt % Tq)) * D + 8 * pc;
      *reinterpret_cast<sp_u32x4*>(ksuf + dst) = *reinterpret_cast<const sp_u32x4*>(k_new + src);
      *reinterpret_cast<sp_u32x4*>(vsuf + dst) = *reinterpret_cast<const sp_u32x4*>(v_new + src);
    }
  }
}

}  // namespace
}  // namespace penroz

using namespace penroz;

// The launch plan (host_plan.h), for ops/attention.py, the decoder, tests and logs: (admitted, query-tile rows,
// query tiles per KV head, key ranges S, workgroups of launch 1, LDS bytes, fp32 workspace floats)
std::tuple<bool, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t> shared_prefix_plan(int64_t R, int64_t H, int64_t Hkv,
                                                                                         int64_t D, int64_t capP,
                                                                                         int64_t splits) {
  const SharedPrefixPlan p = plan_shared_prefix(R, H, Hkv, D, capP, (int)splits);
  return {p.ok, p.tile_rows, p.tiles, p.splits, p.grid, p.lds_bytes, p.ws_floats};
}

// The prefix workgroups' key ranges at prefix length P (host_plan.h shared_prefix_range), for tests: [first, second) per s
std::vector<std::pair<int64_t, int64_t>> shared_prefix_ranges(int64_t P, int64_t S) {
  std::vector<std::pair<int64_t, int64_t>> r;
  for (int s = 0; s < (int)S; ++s) r.push_back(shared_prefix_range(P, (int)S, s));
  return r;
}

// q [R, H, D], k_new / v_new [R, Hkv, D]: bf16 views into the step's fused QKV rows (one row stride each);
// kp / vp [1, Hkv, capP, D] and ks / vs [R, Hkv, capS, D]: bf16 caches; prefix_t: device int64 [1], the prefix
// length; len_t: device int64 [1], the total length after this step, or [R], every row's own. Writes slot
// len − 1 − prefix of ks / vs (per row, its own).
// splits > 0 forces S (tests, A/B). -> [R, H·D] bf16
torch::Tensor shared_prefix_attn(torch::Tensor q, torch::Tensor k_new, torch::Tensor v_new, torch::Tensor kp,
                                 torch::Tensor vp, torch::Tensor ks, torch::Tensor vs, torch::Tensor prefix_t,
                                 torch::Tensor len_t, double scale, int64_t splits) {
  const char* who = "shared_prefix_attn";
  la_one_device(who, q, {k_new, v_new, kp, vp, ks, vs, prefix_t, len_t});
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 && q.dim() == 3 && q.stride(2) == 1 && q.stride(1) == q.size(2) &&
                  q.stride(0) % 8 == 0 && la_aligned(q, 16),
              who, ": bf16 q [R, H, D] with packed heads, rows 16-B aligned");
  const int64_t R = q.size(0), H = q.size(1), D = q.size(2);
  TORCH_CHECK(kp.scalar_type() == torch::kBFloat16 && kp.dim() == 4 && kp.is_contiguous() && vp.is_contiguous() &&
                  vp.scalar_type() == torch::kBFloat16 && kp.sizes() == vp.sizes() && kp.size(0) == 1 && kp.size(3) == D &&
                  la_aligned(kp, 16) && la_aligned(vp, 16),
              who, ": contiguous bf16 prefix caches [1, Hkv, capP, D]");
  const int64_t Hkv = kp.size(1), capP = kp.size(2);
  TORCH_CHECK(ks.scalar_type() == torch::kBFloat16 && ks.dim() == 4 && ks.is_contiguous() && vs.is_contiguous() &&
                  vs.scalar_type() == torch::kBFloat16 && ks.sizes() == vs.sizes() && ks.size(0) == R && ks.size(1) == Hkv &&
                  ks.size(3) == D && ks.size(2) >= 1 && la_aligned(ks, 16) && la_aligned(vs, 16),
              who, ": contiguous bf16 suffix caches [R, Hkv, capS, D]");
  const int64_t capS = ks.size(2);
  for (const auto* t : {&k_new, &v_new})
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16 && t->dim() == 3 && t->size(0) == R && t->size(1) == Hkv &&
                    t->size(2) == D && t->stride(2) == 1 && t->stride(1) == D && la_aligned(*t, 16),
                who, ": bf16 k_new / v_new [R, Hkv, D] with packed heads, rows 16-B aligned");
  TORCH_CHECK(k_new.stride(0) == v_new.stride(0) && k_new.stride(0) % 8 == 0, who, ": k_new / v_new row stride");
  const int64_t* pt = la_i64_scalar(who, "prefix_t", prefix_t);
  const I64Rows lt = la_i64_rows(who, "len_t", len_t, R);
  const SharedPrefixPlan p = plan_shared_prefix(R, H, Hkv, D, capP, (int)splits);
  TORCH_CHECK(p.ok, who, ": 2-64 rows, head_dim 64 / 128 / 256, H / Hkv in {1, 2, 4, 8} (the replicated call takes the rest)");
  TORCH_CHECK(capP * D < (int64_t(1) << 30) && capS * D * R * Hkv < (int64_t(1) << 40), who, ": cache too large");
  auto ws = torch::empty({p.ws_floats}, q.options().dtype(torch::kFloat32));
  auto out = torch::empty({R, H * D}, q.options());
  const int64_t rows = R * H;
  float* ws_o = ws.data_ptr<float>();
  float* ws_ml = ws_o + (int64_t)(p.splits + 1) * rows * D;
  int gs = 0;
  while ((Hkv << gs) < H) ++gs;
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto d, auto nw) {
    constexpr int DD = decltype(d)::value, NWQ = decltype(nw)::value;
    hipLaunchKernelGGL((shared_prefix_kernel<DD, NWQ>), dim3((unsigned)p.grid), dim3(256), 0, stream,
                       reinterpret_cast<const bf16*>(q.data_ptr()), reinterpret_cast<const bf16*>(k_new.data_ptr()),
                       reinterpret_cast<const bf16*>(v_new.data_ptr()), reinterpret_cast<const bf16*>(kp.data_ptr()),
                       reinterpret_cast<const bf16*>(vp.data_ptr()), reinterpret_cast<bf16*>(ks.data_ptr()),
                       reinterpret_cast<bf16*>(vs.data_ptr()), pt, lt.p, lt.stride, ws_o, ws_ml, (int)R, (int)Hkv, gs,
                       (int)capP, (int)capS, p.splits, p.tiles, (float)scale, (int64_t)q.stride(0), (int64_t)k_new.stride(0));
  };
  const bool ok = dispatch_exact(launch, PrefillDims{}, (int)D, PrefillWaves{}, p.tile_rows / 32);
  TORCH_CHECK(ok, who, ": no kernel for the planned tile");
  hipLaunchKernelGGL(shared_prefix_merge_kernel, dim3((unsigned)((rows * (D / 4) + 255) / 256)), dim3(256), 0, stream, ws_o,
                     ws_ml, reinterpret_cast<bf16*>(out.data_ptr()), (int)rows, (int)D, p.splits + 1);
  return out;
}

// The prefill form's launch plan (host_plan.h): (admitted, tile rows, prefix query tiles per KV head, suffix query
// tiles per (row, KV head), key ranges S, workgroups of launch 1, LDS bytes, fp32 workspace floats)
std::tuple<bool, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t> shared_prefix_prefill_plan(
    int64_t R, int64_t Tq, int64_t H, int64_t Hkv, int64_t D, int64_t capP, int64_t capS, int64_t splits) {
  const SharedPrefixPrefillPlan p = plan_shared_prefix_prefill(R, Tq, H, Hkv, D, capP, capS, (int)splits);
  return {p.ok, p.tile_rows, p.tiles, p.suffix_tiles, p.splits, p.grid, p.lds_bytes, p.ws_floats};
}

// q [R, Tq, H, D], k_new / v_new [R, Tq, Hkv, D]: bf16 views into the call's fused QKV rows (uniform row strides);
// kp / vp [1, Hkv, capP, D] and ks / vs [R, Hkv, capS, D]: bf16 caches; prefix_t: device int64 [1], the prefix
// length. Query t of row r attends the prefix keys and row r's new keys 0..t; the new K / V are written into
// suffix slots 0..Tq − 1. splits > 0 forces S (tests, A/B). -> [R, Tq, H·D] bf16
torch::Tensor shared_prefix_prefill_attn(torch::Tensor q, torch::Tensor k_new, torch::Tensor v_new, torch::Tensor kp,
                                         torch::Tensor vp, torch::Tensor ks, torch::Tensor vs, torch::Tensor prefix_t,
                                         double scale, int64_t splits) {
  const char* who = "shared_prefix_prefill_attn";
  la_one_device(who, q, {k_new, v_new, kp, vp, ks, vs, prefix_t});
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 && q.dim() == 4 && q.stride(3) == 1 && q.stride(2) == q.size(3) &&
                  (q.size(1) == 1 || q.stride(0) == q.size(1) * q.stride(1)) && la_aligned(q, 16),
              who, ": bf16 q [R, Tq, H, D] with packed heads and a uniform row stride, rows 16-B aligned");
  const int64_t R = q.size(0), Tq = q.size(1), H = q.size(2), D = q.size(3);
  const int64_t q_rs = Tq == 1 ? q.stride(0) : q.stride(1);
  TORCH_CHECK(q_rs % 8 == 0 && q_rs >= H * D, who, ": q row stride");
  TORCH_CHECK(kp.scalar_type() == torch::kBFloat16 && kp.dim() == 4 && kp.is_contiguous() && vp.is_contiguous() &&
                  vp.scalar_type() == torch::kBFloat16 && kp.sizes() == vp.sizes() && kp.size(0) == 1 && kp.size(3) == D &&
                  la_aligned(kp, 16) && la_aligned(vp, 16),
              who, ": contiguous bf16 prefix caches [1, Hkv, capP, D]");
  const int64_t Hkv = kp.size(1), capP = kp.size(2);
  TORCH_CHECK(ks.scalar_type() == torch::kBFloat16 && ks.dim() == 4 && ks.is_contiguous() && vs.is_contiguous() &&
                  vs.scalar_type() == torch::kBFloat16 && ks.sizes() == vs.sizes() && ks.size(0) == R && ks.size(1) == Hkv &&
                  ks.size(3) == D && ks.size(2) >= Tq && la_aligned(ks, 16) && la_aligned(vs, 16),
              who, ": contiguous bf16 suffix caches [R, Hkv, capS >= Tq, D]");
  const int64_t capS = ks.size(2);
  for (const auto* t : {&k_new, &v_new})
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16 && t->dim() == 4 && t->size(0) == R && t->size(1) == Tq &&
                    t->size(2) == Hkv && t->size(3) == D && t->stride(3) == 1 && t->stride(2) == D &&
                    (Tq == 1 || t->stride(0) == Tq * t->stride(1)) && la_aligned(*t, 16),
                who, ": bf16 k_new / v_new [R, Tq, Hkv, D] with packed heads and a uniform row stride, rows 16-B aligned");
  const int64_t kv_rs = Tq == 1 ? k_new.stride(0) : k_new.stride(1);
  TORCH_CHECK(kv_rs == (Tq == 1 ? v_new.stride(0) : v_new.stride(1)) && kv_rs % 8 == 0 && kv_rs >= Hkv * D, who,
              ": k_new / v_new row stride");
  const int64_t* pt = la_i64_scalar(who, "prefix_t", prefix_t);
  const SharedPrefixPrefillPlan p = plan_shared_prefix_prefill(R, Tq, H, Hkv, D, capP, capS, (int)splits);
  TORCH_CHECK(p.ok, who, ": 2-64 rows, 1 to capS positions, head_dim 64 / 128 / 256, H / Hkv in {1, 2, 4, 8}");
  // the tile loads address K / V rows with 32-bit byte offsets from a per-head or per-row base
  TORCH_CHECK(capP * D < (int64_t(1) << 30) && Tq * kv_rs < (int64_t(1) << 30) && capS * D * R * Hkv < (int64_t(1) << 40),
              who, ": cache or QKV rows too large");
  auto ws = torch::empty({p.ws_floats}, q.options().dtype(torch::kFloat32));
  auto out = torch::empty({R, Tq, H * D}, q.options());
  const int64_t rows = R * Tq * H;
  float* ws_o = ws.data_ptr<float>();
  float* ws_ml = ws_o + (int64_t)(p.splits + 1) * rows * D;
  int gs = 0;
  while ((Hkv << gs) < H) ++gs;
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto d, auto nw) {
    constexpr int DD = decltype(d)::value, NWQ = decltype(nw)::value;
    hipLaunchKernelGGL((shared_prefix_prefill_kernel<DD, NWQ>), dim3((unsigned)p.grid), dim3(256), 0, stream,
                       reinterpret_cast<const bf16*>(q.data_ptr()), reinterpret_cast<const bf16*>(k_new.data_ptr()),
                       reinterpret_cast<const bf16*>(v_new.data_ptr()), reinterpret_cast<const bf16*>(kp.data_ptr()),
                       reinterpret_cast<const bf16*>(vp.data_ptr()), reinterpret_cast<bf16*>(ks.data_ptr()),
                       reinterpret_cast<bf16*>(vs.data_ptr()), pt, ws_o, ws_ml, (int)R, (int)Tq, (int)Hkv, gs, (int)capP,
                       (int)capS, p.splits, p.tiles, p.suffix_tiles, (float)scale, q_rs, kv_rs);
  };
  const bool ok = dispatch_exact(launch, PrefillDims{}, (int)D, PrefillWaves{}, p.tile_rows / 32);
  TORCH_CHECK(ok, who, ": no kernel for the planned tile");
  hipLaunchKernelGGL(shared_prefix_merge_kernel, dim3((unsigned)((rows * (D / 4) + 255) / 256)), dim3(256), 0, stream, ws_o,
                     ws_ml, reinterpret_cast<bf16*>(out.data_ptr()), (int)rows, (int)D, p.splits + 1);
  return out;
}

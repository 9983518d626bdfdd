// Shared-prefix attention over the int8 "TurboQuant" KV cache: the decode form and the prefill form of
// shared_prefix_attn.hip for caches int8 [·, Hkv, cap, D] with one fp32 scale per (row, KV head, token)
// [·, Hkv, cap]. The split of the work, the fp32 partials (o[D], m, l) per (row, head) in [S + 1, R, H, ·] and
// launch 2 (shared_prefix_common.h) are the bf16 kernels'; what changes is how a K / V tile reaches LDS and where
// the scales enter.
//
// Prefix workgroups (KV head, query tile of 32 / 64 / 128 packed rows, key range s of S from the DEVICE-side prefix
// length). An int8 tile cannot come by LDS-DMA into a bf16 image, so every thread loads 16 values (16 B) per lane
// load into registers — K of tile j + 1 under tile j's score MFMAs, V of tile j + 1 under its softmax and P·V
// MFMAs — widens them to bf16 (exact: |x| <= 128 has 8 significant bits) and writes them into the other stage of
// the two-stage XOR-swizzled ring, the image the bf16 kernel's fragment reads expect. The tile's K and V scales are
// staged per ring stage; the K scale multiplies the score column after the MFMA and before the maximum, the V
// scale the P column before P is rounded to bf16, and the denominator sums the unscaled P (prefill_attn.hip's
// int8 path). Keys at or beyond the range end load the range's last row and its scales (finite data under
// P = 0 weights); a range that starts beyond P loads nothing and writes the weight-0 partial.
//
// Suffix workgroups, decode form (row, KV head): the step's new K and V rows are quantised in the kernel —
// absmax over D by a shuffle reduction over the threads that hold the row's pieces, scale = absmax / 127 (1 when
// 0), round to nearest even, clamp: bit for bit kv_quantize and decode_attn.hip's fused append — stored with
// their scales into suffix slot len − 1 − P, and take part in the step as those int8 values times the scale, as
// every other key does (decode_attn.hip's fused int8 append does the same). The row's len − P suffix keys are
// attended one key per thread group from the int8 suffix cache, V through LDS as int8.
//
// Prefill form (share_prefix remainder pass): the causal suffix workgroups stage the call's bf16 K / V rows and
// quantise them on the way into LDS — the same rule, absmax over the lanes that hold a row — so every new key and
// value is seen as the cache will hold it, without waiting for the copy workgroups, which store the int8 rows and
// scales into suffix slots 0..Tq − 1. The result is attention over the cache as stored: what write-then-attend on
// the plain int8 cache computes.
//
// No atomics, no waiting between workgroups, bitwise reproducible; a row's bits depend on its own query, the
// prefix, its own suffix, P and S only.
#include "attn_common.h"
#include "launch_args.h"
#include "shared_prefix_common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {
namespace {

// 4 int8 -> 4 bf16 (exact)
__device__ __forceinline__ void spq_widen(uint32_t w, uint32_t& lo, uint32_t& hi) {
  lo = pack_bf16x2((float)(int8_t)(w & 0xff), (float)(int8_t)((w >> 8) & 0xff));
  hi = pack_bf16x2((float)(int8_t)((w >> 16) & 0xff), (float)(int8_t)(w >> 24));
}

// ---- the quantiser: kv_quantize's rule on bf16 pieces held in registers -----------------------------
__device__ __forceinline__ float spq_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float spq_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
__device__ __forceinline__ float spq_absmax8(sp_u32x4 u, float m) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) m = fmaxf(fmaxf(m, fabsf(spq_lo(w[e]))), fabsf(spq_hi(w[e])));
  return m;
}
__device__ __forceinline__ float spq_scale(float absmax) {
  const float sc = absmax / 127.f;
  return sc == 0.f ? 1.f : sc;
}
__device__ __forceinline__ float spq_q(float x, float sc) { return fminf(fmaxf(rintf(x / sc), -128.f), 127.f); }
__device__ __forceinline__ uint32_t spq_byte(float x) { return (uint32_t)(uint8_t)(int8_t)x; }
// 16 bf16 (two pieces) -> 16 int8 (one piece)
__device__ __forceinline__ sp_u32x4 spq_pack16(sp_u32x4 a, sp_u32x4 b, float sc) {
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
    o[e] = spq_byte(spq_q(spq_lo(w[2 * e]), sc)) | (spq_byte(spq_q(spq_hi(w[2 * e]), sc)) << 8) |
           (spq_byte(spq_q(spq_lo(w[2 * e + 1]), sc)) << 16) | (spq_byte(spq_q(spq_hi(w[2 * e + 1]), sc)) << 24);
  return sp_u32x4{o[0], o[1], o[2], o[3]};
}
// 8 bf16 -> the 8 quantised values as bf16 (what widening the stored int8 gives)
__device__ __forceinline__ uint4 spq_quant8_bf16(sp_u32x4 a, float sc) {
  return uint4{pack_bf16x2(spq_q(spq_lo(a.x), sc), spq_q(spq_hi(a.x), sc)), pack_bf16x2(spq_q(spq_lo(a.y), sc), spq_q(spq_hi(a.y), sc)),
               pack_bf16x2(spq_q(spq_lo(a.z), sc), spq_q(spq_hi(a.z), sc)), pack_bf16x2(spq_q(spq_lo(a.w), sc), spq_q(spq_hi(a.w), sc))};
}

// ---- the tile body: 32·NWQ query rows against keys [k0, kend) of one K / V matrix --------------------
// Key i is visible to a lane's row while i <= klast (shared_prefix_attn.hip sp_tile). FRESH false: kb / vb are int8
// cache rows of D bytes with scales ks / vs per key; FRESH true: kb / vb are bf16 rows kstride elements apart (the
// call's own K / V), quantised per row while they are staged.
template <int D, int NWQ, bool FRESH, class QSrc>
__device__ __forceinline__ void spq_tile(char* smem, QSrc qsrc, bool valid, bool wact, int klast, int kminw, int kmaxw,
                                         const void* __restrict__ kb, const void* __restrict__ vb,
                                         const float* __restrict__ ks, const float* __restrict__ vs, int kstride, int k0,
                                         int kend, float c, float* __restrict__ orow, float* __restrict__ mlrow) {
  constexpr int NP = D / 64, NS = D / 16, ND = D / 32, BM = 32 * NWQ, NT = 256;
  constexpr bool QLDS = D >= 256;
  constexpr int BN = prefill_keys(D), NH = BN / 32;
  constexpr int TILE = BN * 128 * NP;
  constexpr int QTILE = QLDS ? BM * 128 * NP : 0;
  constexpr int CPR = D / 16;            // 16-value chunks per key row
  constexpr int NL = BN * CPR / NT;      // chunks per thread, tile and matrix
  constexpr int NRG = FRESH ? 2 * NL : NL;
  static_assert(NL >= 1 && BN * CPR % NT == 0, "tile staging");
  const char* Qs = smem + 4 * TILE;
  float* sc = reinterpret_cast<float*>(smem + 4 * TILE + QTILE);  // [stage][K scales BN | V scales BN]
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id(), hh = lane >> 5;
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

  // tile j of one matrix into registers: thread = chunk (row, ch) of 16 values; rows at or beyond kend load row
  // kend − 1 (nothing beyond the keys in use is read)
  auto load = [&](const void* base, int j, sp_u32x4 (&rg)[NRG]) {
    const int ot = 64 * w + opaque_lane_id();  // addresses recomputed per call, not kept in registers
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      const int idx = t * NT + ot, row = idx / CPR, ch = idx % CPR;
      const int krow = max(min(k0 + j * BN + row, kend - 1), 0);
      if constexpr (FRESH) {
        const char* p = reinterpret_cast<const char*>(base) + (size_t)(unsigned)(krow * kstride + 16 * ch) * 2;
        rg[2 * t] = *reinterpret_cast<const sp_u32x4*>(p);
        rg[2 * t + 1] = *reinterpret_cast<const sp_u32x4*>(p + 16);
      } else {
        rg[t] = *reinterpret_cast<const sp_u32x4*>(reinterpret_cast<const char*>(base) + (unsigned)(krow * D + 16 * ch));
      }
    }
  };
  // ... and from registers into the swizzled bf16 image; FRESH: the row's scale into scd[row]
  auto store = [&](char* tile, const sp_u32x4 (&rg)[NRG], float* scd) {
    const int ot = 64 * w + opaque_lane_id();
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      const int idx = t * NT + ot, row = idx / CPR, ch = idx % CPR;
      uint4 a, bq;
      if constexpr (FRESH) {
        float mx = spq_absmax8(rg[2 * t + 1], spq_absmax8(rg[2 * t], 0.f));
#pragma unroll
        for (int x = 1; x < CPR; x <<= 1) mx = fmaxf(mx, __shfl_xor(mx, x, 64));  // the CPR lanes that hold the row
        const float s = spq_scale(mx);
        if (ch == 0) scd[row] = s;
        a = spq_quant8_bf16(rg[2 * t], s);
        bq = spq_quant8_bf16(rg[2 * t + 1], s);
      } else {
        spq_widen(rg[t].x, a.x, a.y);
        spq_widen(rg[t].y, a.z, a.w);
        spq_widen(rg[t].z, bq.x, bq.y);
        spq_widen(rg[t].w, bq.z, bq.w);
      }
      char* pn = tile + (ch >> 2) * BN * 128;
      *reinterpret_cast<uint4*>(pn + tile_off(row, 2 * (ch & 3))) = a;
      *reinterpret_cast<uint4*>(pn + tile_off(row, 2 * (ch & 3) + 1)) = bq;
    }
  };
  auto scales = [&](int j) {  // the cache's: keys at or beyond kend take key kend − 1's (finite)
    if constexpr (!FRESH) {
      if (tid < 2 * BN) {
        const int key = max(min(k0 + j * BN + (tid & (BN - 1)), kend - 1), 0);
        sc[(j & 1) * 2 * BN + tid] = (tid < BN ? ks : vs)[key];
      }
    }
  };

  sp_u32x4 rg[NRG];
  if (ntk > 0) {
    load(kb, 0, rg);
    store(smem, rg, sc);
    load(vb, 0, rg);
    store(smem + TILE, rg, sc + BN);
    scales(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the Q image's DMA
  __syncthreads();

  for (int j = 0; j < ntk; ++j) {
    const bool next = j + 1 < ntk;
    char* nstage = smem + ((j + 1) & 1) * 2 * TILE;  // released by the previous iteration's barrier
    float* nsc = sc + ((j + 1) & 1) * 2 * BN;
    if (next) load(kb, j + 1, rg);
    const char* Kt = smem + (j & 1) * 2 * TILE;
    const char* Vt = Kt + TILE;
    const float* sct = sc + (j & 1) * 2 * BN;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {  // the tile's 32-key halves, one online-softmax step each
      const int kh0 = k0 + j * BN + 32 * hf;
      const bool act = wact && kh0 <= kmaxw;  // wave-uniform: some row of the wave sees a key of this half
      f32x16 st;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = 0.f;
      if (act) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          st = mfma32(row_frag(Kt + (s >> 2) * BN * 128, 32 * hf, s & 3, lane), qfrag(s), st);
          if constexpr (D >= 256)
            if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // keep few LDS fragments in flight
        }
      }
      if (hf == 0 && next) {  // K of tile j + 1 landed under the score MFMAs; its V loads fly under the rest
        store(nstage, rg, nsc);
        load(vb, j + 1, rg);
      }
      if (act) {
        auto softmax = [&](auto mask_tag) {
          constexpr bool MASK = decltype(mask_tag)::value;
          float tmax = -INFINITY;
#pragma unroll
          for (int i4 = 0; i4 < 4; ++i4) {
            const float4_t ksc = *reinterpret_cast<const float4_t*>(sct + 32 * hf + 8 * i4 + 4 * hh);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int i = 4 * i4 + k;
              float s = st[i] * ksc[k];
              if constexpr (MASK) s = kh0 + acc_row(i, lane) > klast ? -INFINITY : s;
              st[i] = s;
              tmax = fmaxf(tmax, s);
            }
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
          for (int i4 = 0; i4 < 4; ++i4) {
            const float4_t vsc = *reinterpret_cast<const float4_t*>(sct + BN + 32 * hf + 8 * i4 + 4 * hh);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float p = fexp2(fmaf(st[4 * i4 + k], c, negm));
              lsum += p;  // the denominator sums the unscaled P
              st[4 * i4 + k] = p * vsc[k];
            }
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
    if (next) {
      store(nstage + TILE, rg, nsc + BN);
      scales(j + 1);
    }
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

// ---- decode form, suffix workgroup: row b, KV head g ---------------------------------------------------
// Thread (kk, part) holds key kk's 64 int8 values part·64 .. of a chunk of KC keys; TPK = 256 / KC threads a key.
template <int D>
__device__ __forceinline__ void spq_suffix(char* smem, const bf16* __restrict__ q, const bf16* __restrict__ k_new,
                                           const bf16* __restrict__ v_new, int8_t* __restrict__ ksuf,
                                           int8_t* __restrict__ vsuf, float* __restrict__ kss, float* __restrict__ vss,
                                           float* __restrict__ ws_o, float* __restrict__ ws_ml, int b, int g, int R, int H,
                                           int Hkv, int G, int capS, int n_suf, float c, int64_t q_rs, int64_t kv_rs, int S) {
  constexpr int GMAX = kSpGroup;
  constexpr int RB = D;                        // cache row bytes
  constexpr int KC = sp_q8_suffix_keys(D);     // keys per chunk (V chunk = 16 KB of LDS)
  constexpr int TPK = 256 / KC;                // threads per key
  constexpr int CR = RB / 16, CPT = CR / TPK;  // 16-B pieces per row, and per thread
  constexpr int SW = CR - 1 < 7 ? CR - 1 : 7;  // LDS row swizzle mask (pieces)
  constexpr int NP2 = D / 2, NG = 256 / NP2;   // P·V: column pairs × key groups
  constexpr int QPT = GMAX * D / 256;
  static_assert(CPT == 4 && KC * RB == 16384 && NG * NP2 == 256 && NG * GMAX * D * 4 <= 16384, "suffix tiling");
  char* vbuf = smem;  // V chunk (int8), later the P·V partials
  float* qs = reinterpret_cast<float*>(smem + 16384);  // [GMAX][D]
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
  const int kk = t / TPK, part = t % TPK;
  const int kg = t / NP2, d0 = 2 * (t % NP2);

  // this step's K and V rows, quantised: every thread takes its part's 64 values (the same row for every key
  // slot, so the reduction runs on all lanes), the absmax over D comes from the TPK lanes of its key
  sp_u32x4 fk[CPT], fv[CPT];
  float fks, fvs;
  auto quant = [&](const bf16* src, sp_u32x4 (&out)[CPT], float& s) {
    sp_u32x4 raw[2 * CPT];
#pragma unroll
    for (int x = 0; x < 2 * CPT; ++x) raw[x] = *reinterpret_cast<const sp_u32x4*>(src + 8 * x);
    float mx = 0.f;
#pragma unroll
    for (int x = 0; x < 2 * CPT; ++x) mx = spq_absmax8(raw[x], mx);
#pragma unroll
    for (int x = 1; x < TPK; x <<= 1) mx = fmaxf(mx, __shfl_xor(mx, x, 64));
    s = spq_scale(mx);
#pragma unroll
    for (int x = 0; x < CPT; ++x) out[x] = spq_pack16(raw[2 * x], raw[2 * x + 1], s);
  };
  const size_t new_off = (size_t)b * kv_rs + (size_t)g * D + (size_t)part * CPT * 16;
  quant(k_new + new_off, fk, fks);
  quant(v_new + new_off, fv, fvs);

  sp_u32x4 kr[CPT], vr[CPT];
  float ksc = 1.f, vsc = 1.f;
  auto load_chunk = [&](int c0) {
    const int key = c0 + kk;
    const size_t row = head_base + (key < k1 ? key : c0);
    const int8_t* ksrc = ksuf + row * D + part * CPT * 16;
    const int8_t* vsrc = vsuf + row * D + part * CPT * 16;
#pragma unroll
    for (int x = 0; x < CPT; ++x) kr[x] = *reinterpret_cast<const sp_u32x4*>(ksrc + 16 * x);
#pragma unroll
    for (int x = 0; x < CPT; ++x) vr[x] = *reinterpret_cast<const sp_u32x4*>(vsrc + 16 * x);
    ksc = kss[row];
    vsc = vss[row];
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
    if (c0 + kk == k1 - 1) {  // this step's row: into its slot, and into the step as what the slot now holds
      const size_t row = head_base + (k1 - 1);
#pragma unroll
      for (int x = 0; x < CPT; ++x) {
        kr[x] = fk[x];
        vr[x] = fv[x];
        *reinterpret_cast<sp_u32x4*>(ksuf + row * D + (part * CPT + x) * 16) = fk[x];
        *reinterpret_cast<sp_u32x4*>(vsuf + row * D + (part * CPT + x) * 16) = fv[x];
      }
      ksc = fks;
      vsc = fvs;
      if (part == 0) {
        kss[row] = fks;
        vss[row] = fvs;
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
        const float* qp = qs + i * D + (part * CPT + x) * 16;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a += qp[4 * e] * (float)(int8_t)(w4[e] & 0xff);
          a += qp[4 * e + 1] * (float)(int8_t)((w4[e] >> 8) & 0xff);
          a += qp[4 * e + 2] * (float)(int8_t)((w4[e] >> 16) & 0xff);
          a += qp[4 * e + 3] * (float)(int8_t)(w4[e] >> 24);
        }
      }
#pragma unroll
      for (int x = 1; x < TPK; x <<= 1) a += __shfl_xor(a, x, 64);
      s[i] = valid ? a * ksc : -INFINITY;
      const float wm = wave_max(s[i]);
      if (lane == 0) red_m[wid * GMAX + i] = wm;
    }
    const float vsc_c = vsc;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < GMAX; ++i) {
      if (i >= G) break;
      const float cm = fmaxf(fmaxf(red_m[i], red_m[GMAX + i]), fmaxf(red_m[2 * GMAX + i], red_m[3 * GMAX + i]));
      const float mn = fmaxf(M[i], cm);  // finite: every chunk holds a valid key
      const float alpha = fexp2(M[i] - mn);
      const float p = valid ? fexp2(s[i] - mn) : 0.f;
      if (part == 0) pl[i * KC + kk] = valid ? p * vsc_c : 0.f;  // the V scale folded into the weight
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
#pragma unroll 8
    for (int j = kg; j < nv; j += NG) {
      const uint32_t wv = *reinterpret_cast<const uint16_t*>(vbuf + j * RB + ((((d0 >> 4) ^ (j & SW))) << 4) + (d0 & 15));
      const float v0 = (float)(int8_t)(wv & 0xff), v1 = (float)(int8_t)(wv >> 8);
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

// The operands of both forms: the step's bf16 rows, the int8 prefix and suffix caches with their scales
struct SpQ8Args {
  const bf16 *q, *k_new, *v_new;
  const int8_t *kp, *vp;
  const float *kps, *vps;
  int8_t *ks, *vs;
  float *kss, *vss;
  const int64_t* prefix_t;
  float *ws_o, *ws_ml;
  int R, Hkv, gs, capP, capS, S, nqt;
  float scale;
  int64_t q_rs, kv_rs;
};

// ---- decode form, launch 1 ------------------------------------------------------------------------------
template <int D, int NWQ>
__global__ void __launch_bounds__(256) shared_prefix_q8_kernel(const SpQ8Args a, const int64_t* __restrict__ len_t, int len_stride) {
  constexpr int BM = 32 * NWQ;
  constexpr int PLDS = sp_q8_prefix_lds(D, BM), SLDS = sp_q8_suffix_lds(D);
  __shared__ __attribute__((aligned(16))) char smem[PLDS > SLDS ? PLDS : SLDS];
  const int R = a.R, Hkv = a.Hkv, gs = a.gs, S = a.S, nqt = a.nqt;
  const int G = 1 << gs, H = Hkv << gs;
  const int P = (int)min<int64_t>(max<int64_t>(a.prefix_t[0], 0), (int64_t)a.capP);
  const float c = a.scale * kLog2e;
  const int nprefix = Hkv * nqt * S;
  if ((int)blockIdx.x >= nprefix) {
    const int item = blockIdx.x - nprefix, b = item / Hkv, g = item % Hkv;
    // the row's own keys, this step's included; a length outside the suffix cache never leaves it
    const int n_suf = (int)min<int64_t>(max<int64_t>(len_t[(size_t)b * len_stride] - P, 1), (int64_t)a.capS);
    spq_suffix<D>(smem, a.q, a.k_new, a.v_new, a.ks, a.vs, a.kss, a.vss, a.ws_o, a.ws_ml, b, g, R, H, Hkv, G, a.capS, n_suf, c,
                  a.q_rs, a.kv_rs, S);
    return;
  }
  const int sp = blockIdx.x % S, qt = (blockIdx.x / S) % nqt, hk = blockIdx.x / (S * nqt);
  const int lane = threadIdx.x & 63, w = wave_id();
  const int pr = qt * BM + 32 * w + (lane & 31);  // this lane's query row: packed index r·G + g of the KV head
  const int row = pr >> gs, head = (hk << gs) + (pr & (G - 1));
  const bool valid = w < NWQ && row < R;
  const bool wact = w < NWQ && ((qt * BM + 32 * w) >> gs) < R;  // wave-uniform: the wave owns real rows
  const int per = ((((P + 63) >> 6) + S - 1) / S) << 6;  // this workgroup's keys [k0, k1), from the device-side length
  const int k0 = sp * per, k1 = min(P, k0 + per);
  auto qsrc = [&](int tr) {
    const int x = qt * BM + tr;
    return a.q + (size_t)min(x >> gs, R - 1) * a.q_rs + (size_t)((hk << gs) + (x & (G - 1))) * D;
  };
  const size_t r = ((size_t)sp * R + (valid ? row : 0)) * H + head;
  spq_tile<D, NWQ, false>(smem, qsrc, valid, wact, k1 - 1, k1 - 1, k1 - 1, a.kp + (size_t)hk * a.capP * D,
                          a.vp + (size_t)hk * a.capP * D, a.kps + (size_t)hk * a.capP, a.vps + (size_t)hk * a.capP, D, k0, k1, c,
                          a.ws_o + r * D, a.ws_ml + 2 * r);
}

// ---- prefill form, launch 1: prefix, causal suffix and copy workgroups (shared_prefix_attn.hip) ----------
template <int D, int NWQ>
__global__ void __launch_bounds__(256) shared_prefix_prefill_q8_kernel(const SpQ8Args a, int Tq, int nst) {
  constexpr int BM = 32 * NWQ;
  __shared__ __attribute__((aligned(16))) char smem[sp_q8_prefix_lds(D, BM)];
  const int R = a.R, Hkv = a.Hkv, gs = a.gs, S = a.S, nqt = a.nqt;
  const int G = 1 << gs, H = Hkv << gs, NR = R * Tq;  // NR: (row, position) pairs
  const int P = (int)min<int64_t>(max<int64_t>(a.prefix_t[0], 0), (int64_t)a.capP);
  const float c = a.scale * kLog2e;
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
      return a.q + (size_t)min(x >> gs, NR - 1) * a.q_rs + (size_t)((hk << gs) + (x & (G - 1))) * D;
    };
    const size_t r = ((size_t)sp * NR + (valid ? pos : 0)) * H + head;
    spq_tile<D, NWQ, false>(smem, qsrc, valid, wact, k1 - 1, k1 - 1, k1 - 1, a.kp + (size_t)hk * a.capP * D,
                            a.vp + (size_t)hk * a.capP * D, a.kps + (size_t)hk * a.capP, a.vps + (size_t)hk * a.capP, D, k0, k1,
                            c, a.ws_o + r * D, a.ws_ml + 2 * r);
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
      return a.q + ((size_t)b * Tq + min(qt * PT + (row >> gs), Tq - 1)) * a.q_rs + (size_t)((hk << gs) + (row & (G - 1))) * D;
    };
    const size_t off = (size_t)b * Tq * a.kv_rs + (size_t)hk * D;  // row b's new keys: slot t is K / V row b·Tq + t
    const size_t r = ((size_t)S * NR + (size_t)b * Tq + (valid ? pl : 0)) * H + head;
    spq_tile<D, NWQ, true>(smem, qsrc, valid, wact, pl, pw0, min(pw0 + (32 >> gs), Tq) - 1, a.k_new + off, a.v_new + off, nullptr,
                           nullptr, (int)a.kv_rs, 0, kend, c, a.ws_o + r * D, a.ws_ml + 2 * r);
    return;
  }
  blk -= nsuffix;
  // copy workgroups: thread = one 16-value chunk of a K and a V head row; the row's absmax over its CR lanes
  constexpr int CR = D / 16;
  const int64_t nchunks = (int64_t)NR * Hkv * CR;  // a multiple of CR, as 256 is: a row's lanes are all in or all out
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int64_t i0 = ((int64_t)blk * 4 + x) * 256 + tid, i = min(i0, nchunks - 1);
    const int pc = (int)(i % CR), hk = (int)((i / CR) % Hkv);
    const int64_t rt = i / (CR * Hkv);
    const size_t src = (size_t)rt * a.kv_rs + (size_t)hk * D + 16 * pc;
    const size_t slot = ((size_t)(rt / Tq) * Hkv + hk) * a.capS + (size_t)(rt % Tq);
    auto one = [&](const bf16* from, int8_t* to, float* scales) {
      const sp_u32x4 lo = *reinterpret_cast<const sp_u32x4*>(from + src), hi = *reinterpret_cast<const sp_u32x4*>(from + src + 8);
      float mx = spq_absmax8(hi, spq_absmax8(lo, 0.f));
#pragma unroll
      for (int y = 1; y < CR; y <<= 1) mx = fmaxf(mx, __shfl_xor(mx, y, 64));
      const float s = spq_scale(mx);
      if (i0 < nchunks) {
        *reinterpret_cast<sp_u32x4*>(to + slot * D + 16 * pc) = spq_pack16(lo, hi, s);
        if (pc == 0) scales[slot] = s;
      }
    };
    one(a.k_new, a.ks, a.kss);
    one(a.v_new, a.vs, a.vss);
  }
}

// ---- host: the operands both forms share ---------------------------------------------------------------
// kp / vp int8 [1, Hkv, capP, D] with kps / vps fp32 [1, Hkv, capP]; ks / vs int8 [R, Hkv, capS, D] with kss / vss
// fp32 [R, Hkv, capS]
void spq_check_caches(const char* who, int64_t R, int64_t D, const torch::Tensor& kp, const torch::Tensor& vp,
                      const torch::Tensor& kps, const torch::Tensor& vps, const torch::Tensor& ks, const torch::Tensor& vs,
                      const torch::Tensor& kss, const torch::Tensor& vss, int64_t min_capS) {
  TORCH_CHECK(kp.scalar_type() == torch::kInt8 && kp.dim() == 4 && kp.is_contiguous() && vp.is_contiguous() &&
                  vp.scalar_type() == torch::kInt8 && kp.sizes() == vp.sizes() && kp.size(0) == 1 && kp.size(3) == D &&
                  la_aligned(kp, 16) && la_aligned(vp, 16),
              who, ": contiguous int8 prefix caches [1, Hkv, capP, D]");
  const int64_t Hkv = kp.size(1), capP = kp.size(2);
  la_f32_shape(who, "prefix K scales", kps, {1, Hkv, capP});
  la_f32_shape(who, "prefix V scales", vps, {1, Hkv, capP});
  TORCH_CHECK(ks.scalar_type() == torch::kInt8 && ks.dim() == 4 && ks.is_contiguous() && vs.is_contiguous() &&
                  vs.scalar_type() == torch::kInt8 && ks.sizes() == vs.sizes() && ks.size(0) == R && ks.size(1) == Hkv &&
                  ks.size(3) == D && ks.size(2) >= min_capS && la_aligned(ks, 16) && la_aligned(vs, 16),
              who, ": contiguous int8 suffix caches [R, Hkv, capS >= ", min_capS, ", D]");
  la_f32_shape(who, "suffix K scales", kss, {R, Hkv, ks.size(2)});
  la_f32_shape(who, "suffix V scales", vss, {R, Hkv, ks.size(2)});
}

SpQ8Args spq_args(const torch::Tensor& q, const torch::Tensor& k_new, const torch::Tensor& v_new, const torch::Tensor& kp,
                  const torch::Tensor& vp, const torch::Tensor& kps, const torch::Tensor& vps, const torch::Tensor& ks,
                  const torch::Tensor& vs, const torch::Tensor& kss, const torch::Tensor& vss, const int64_t* pt, float* ws_o,
                  float* ws_ml, int64_t R, int64_t H, int splits, int tiles, double scale, int64_t q_rs, int64_t kv_rs) {
  const int64_t Hkv = kp.size(1);
  int gs = 0;
  while ((Hkv << gs) < H) ++gs;
  return {reinterpret_cast<const bf16*>(q.data_ptr()), reinterpret_cast<const bf16*>(k_new.data_ptr()),
          reinterpret_cast<const bf16*>(v_new.data_ptr()), kp.data_ptr<int8_t>(), vp.data_ptr<int8_t>(), kps.data_ptr<float>(),
          vps.data_ptr<float>(), ks.data_ptr<int8_t>(), vs.data_ptr<int8_t>(), kss.data_ptr<float>(), vss.data_ptr<float>(), pt,
          ws_o, ws_ml, (int)R, (int)Hkv, gs, (int)kp.size(2), (int)ks.size(2), splits, tiles, (float)scale, q_rs, kv_rs};
}

}  // namespace
}  // namespace penroz

using namespace penroz;

// The int8 decode form's launch plan (host_plan.h), laid out as shared_prefix_plan's
std::tuple<bool, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t> shared_prefix_q8_plan(int64_t R, int64_t H, int64_t Hkv,
                                                                                            int64_t D, int64_t capP,
                                                                                            int64_t splits) {
  const SharedPrefixPlan p = plan_shared_prefix_q8(R, H, Hkv, D, capP, (int)splits);
  return {p.ok, p.tile_rows, p.tiles, p.splits, p.grid, p.lds_bytes, p.ws_floats};
}

// shared_prefix_attn over int8 caches. q [R, H, D], k_new / v_new [R, Hkv, D]: bf16 views into the step's fused QKV
// rows; kp / vp int8 [1, Hkv, capP, D] with scales kps / vps fp32 [1, Hkv, capP]; ks / vs int8 [R, Hkv, capS, D]
// with scales kss / vss fp32 [R, Hkv, capS]; prefix_t, len_t as in shared_prefix_attn. Quantises the new rows into
// slot len − 1 − prefix of ks / vs / kss / vss (per row, its own). -> [R, H·D] bf16
torch::Tensor shared_prefix_attn_q8(torch::Tensor q, torch::Tensor k_new, torch::Tensor v_new, torch::Tensor kp,
                                    torch::Tensor vp, torch::Tensor kps, torch::Tensor vps, torch::Tensor ks, torch::Tensor vs,
                                    torch::Tensor kss, torch::Tensor vss, torch::Tensor prefix_t, torch::Tensor len_t,
                                    double scale, int64_t splits) {
  const char* who = "shared_prefix_attn_q8";
  la_one_device(who, q, {k_new, v_new, kp, vp, kps, vps, ks, vs, kss, vss, prefix_t, len_t});
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 && q.dim() == 3 && q.stride(2) == 1 && q.stride(1) == q.size(2) &&
                  q.stride(0) % 8 == 0 && la_aligned(q, 16),
              who, ": bf16 q [R, H, D] with packed heads, rows 16-B aligned");
  const int64_t R = q.size(0), H = q.size(1), D = q.size(2);
  spq_check_caches(who, R, D, kp, vp, kps, vps, ks, vs, kss, vss, 1);
  const int64_t Hkv = kp.size(1), capP = kp.size(2), capS = ks.size(2);
  for (const auto* t : {&k_new, &v_new})
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16 && t->dim() == 3 && t->size(0) == R && t->size(1) == Hkv &&
                    t->size(2) == D && t->stride(2) == 1 && t->stride(1) == D && la_aligned(*t, 16),
                who, ": bf16 k_new / v_new [R, Hkv, D] with packed heads, rows 16-B aligned");
  TORCH_CHECK(k_new.stride(0) == v_new.stride(0) && k_new.stride(0) % 8 == 0, who, ": k_new / v_new row stride");
  const int64_t* pt = la_i64_scalar(who, "prefix_t", prefix_t);
  const I64Rows lt = la_i64_rows(who, "len_t", len_t, R);
  const SharedPrefixPlan p = plan_shared_prefix_q8(R, H, Hkv, D, capP, (int)splits);
  TORCH_CHECK(p.ok, who, ": 2-64 rows, head_dim 64 / 128 / 256, H / Hkv in {1, 2, 4, 8} (the replicated call takes the rest)");
  TORCH_CHECK(capP * D < (int64_t(1) << 30) && capS * D * R * Hkv < (int64_t(1) << 40), who, ": cache too large");
  auto ws = torch::empty({p.ws_floats}, q.options().dtype(torch::kFloat32));
  auto out = torch::empty({R, H * D}, q.options());
  const int64_t rows = R * H;
  float* ws_o = ws.data_ptr<float>();
  float* ws_ml = ws_o + (int64_t)(p.splits + 1) * rows * D;
  const SpQ8Args a = spq_args(q, k_new, v_new, kp, vp, kps, vps, ks, vs, kss, vss, pt, ws_o, ws_ml, R, H, p.splits, p.tiles,
                              scale, q.stride(0), k_new.stride(0));
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto d, auto nw) {
    constexpr int DD = decltype(d)::value, NWQ = decltype(nw)::value;
    hipLaunchKernelGGL((shared_prefix_q8_kernel<DD, NWQ>), dim3((unsigned)p.grid), dim3(256), 0, stream, a, lt.p, lt.stride);
  };
  const bool ok = dispatch_exact(launch, PrefillDims{}, (int)D, PrefillWaves{}, p.tile_rows / 32);
  TORCH_CHECK(ok, who, ": no kernel for the planned tile");
  hipLaunchKernelGGL(shared_prefix_merge_kernel, dim3((unsigned)((rows * (D / 4) + 255) / 256)), dim3(256), 0, stream, ws_o,
                     ws_ml, reinterpret_cast<bf16*>(out.data_ptr()), (int)rows, (int)D, p.splits + 1);
  return out;
}

// The int8 prefill form's launch plan (host_plan.h), laid out as shared_prefix_prefill_plan's
std::tuple<bool, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t> shared_prefix_prefill_q8_plan(
    int64_t R, int64_t Tq, int64_t H, int64_t Hkv, int64_t D, int64_t capP, int64_t capS, int64_t splits) {
  const SharedPrefixPrefillPlan p = plan_shared_prefix_prefill_q8(R, Tq, H, Hkv, D, capP, capS, (int)splits);
  return {p.ok, p.tile_rows, p.tiles, p.suffix_tiles, p.splits, p.grid, p.lds_bytes, p.ws_floats};
}

// shared_prefix_prefill_attn over int8 caches: q [R, Tq, H, D], k_new / v_new [R, Tq, Hkv, D] bf16 views into the
// call's fused QKV rows; the caches and scales as in shared_prefix_attn_q8. Query t of row r attends the prefix
// keys and row r's new keys 0..t as the cache stores them; the new K / V are quantised into suffix slots
// 0..Tq − 1. -> [R, Tq, H·D] bf16
torch::Tensor shared_prefix_prefill_attn_q8(torch::Tensor q, torch::Tensor k_new, torch::Tensor v_new, torch::Tensor kp,
                                            torch::Tensor vp, torch::Tensor kps, torch::Tensor vps, torch::Tensor ks,
                                            torch::Tensor vs, torch::Tensor kss, torch::Tensor vss, torch::Tensor prefix_t,
                                            double scale, int64_t splits) {
  const char* who = "shared_prefix_prefill_attn_q8";
  la_one_device(who, q, {k_new, v_new, kp, vp, kps, vps, ks, vs, kss, vss, prefix_t});
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 && q.dim() == 4 && q.stride(3) == 1 && q.stride(2) == q.size(3) &&
                  (q.size(1) == 1 || q.stride(0) == q.size(1) * q.stride(1)) && la_aligned(q, 16),
              who, ": bf16 q [R, Tq, H, D] with packed heads and a uniform row stride, rows 16-B aligned");
  const int64_t R = q.size(0), Tq = q.size(1), H = q.size(2), D = q.size(3);
  const int64_t q_rs = Tq == 1 ? q.stride(0) : q.stride(1);
  TORCH_CHECK(q_rs % 8 == 0 && q_rs >= H * D, who, ": q row stride");
  spq_check_caches(who, R, D, kp, vp, kps, vps, ks, vs, kss, vss, Tq);
  const int64_t Hkv = kp.size(1), capP = kp.size(2), capS = ks.size(2);
  for (const auto* t : {&k_new, &v_new})
    TORCH_CHECK(t->scalar_type() == torch::kBFloat16 && t->dim() == 4 && t->size(0) == R && t->size(1) == Tq &&
                    t->size(2) == Hkv && t->size(3) == D && t->stride(3) == 1 && t->stride(2) == D &&
                    (Tq == 1 || t->stride(0) == Tq * t->stride(1)) && la_aligned(*t, 16),
                who, ": bf16 k_new / v_new [R, Tq, Hkv, D] with packed heads and a uniform row stride, rows 16-B aligned");
  const int64_t kv_rs = Tq == 1 ? k_new.stride(0) : k_new.stride(1);
  TORCH_CHECK(kv_rs == (Tq == 1 ? v_new.stride(0) : v_new.stride(1)) && kv_rs % 8 == 0 && kv_rs >= Hkv * D, who,
              ": k_new / v_new row stride");
  const int64_t* pt = la_i64_scalar(who, "prefix_t", prefix_t);
  const SharedPrefixPrefillPlan p = plan_shared_prefix_prefill_q8(R, Tq, H, Hkv, D, capP, capS, (int)splits);
  TORCH_CHECK(p.ok, who, ": 2-64 rows, 1 to capS positions, head_dim 64 / 128 / 256, H / Hkv in {1, 2, 4, 8}");
  // the tile loads address K / V rows with 32-bit offsets from a per-head or per-row base
  TORCH_CHECK(capP * D < (int64_t(1) << 30) && Tq * kv_rs < (int64_t(1) << 30) && capS * D * R * Hkv < (int64_t(1) << 40),
              who, ": cache or QKV rows too large");
  auto ws = torch::empty({p.ws_floats}, q.options().dtype(torch::kFloat32));
  auto out = torch::empty({R, Tq, H * D}, q.options());
  const int64_t rows = R * Tq * H;
  float* ws_o = ws.data_ptr<float>();
  float* ws_ml = ws_o + (int64_t)(p.splits + 1) * rows * D;
  const SpQ8Args a = spq_args(q, k_new, v_new, kp, vp, kps, vps, ks, vs, kss, vss, pt, ws_o, ws_ml, R, H, p.splits, p.tiles,
                              scale, q_rs, kv_rs);
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto d, auto nw) {
    constexpr int DD = decltype(d)::value, NWQ = decltype(nw)::value;
    hipLaunchKernelGGL((shared_prefix_prefill_q8_kernel<DD, NWQ>), dim3((unsigned)p.grid), dim3(256), 0, stream, a, (int)Tq,
                       p.suffix_tiles);
  };
  const bool ok = dispatch_exact(launch, PrefillDims{}, (int)D, PrefillWaves{}, p.tile_rows / 32);
  TORCH_CHECK(ok, who, ": no kernel for the planned tile");
  hipLaunchKernelGGL(shared_prefix_merge_kernel, dim3((unsigned)((rows * (D / 4) + 255) / 256)), dim3(256), 0, stream, ws_o,
                     ws_ml, reinterpret_cast<bf16*>(out.data_ptr()), (int)rows, (int)D, p.splits + 1);
  return out;
}

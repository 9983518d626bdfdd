// Prefill attention over the KV cache: forward-only causal flash attention for MANY query rows
// (a prompt, a window-full re-prefill, a later chunk of a prompt) whose keys and values are read
// from the cache [B, Hkv, cap, D] — bf16, or int8 with per-token fp32 scales (TurboQuant).
// Query i sits at position q_offset + i and sees cache slots 0 … q_offset + i; slots at or beyond
// S = q_offset + Tq are never used. decode_attn.hip serves the same definition one query position
// per workgroup on the VALU; this kernel serves it with v_mfma_f32_32x32x16_bf16.
//
// Work split. One workgroup = one (batch, KV head, query tile); NW = 1 / 2 / 4 waves of 32 tile rows
// each. The G = H / Hkv query heads of the KV head are packed into the tile's rows — row r is
// (position r / G, head r % G) — so one staged K/V tile serves the whole group (Gemma-3 1B: G = 4 on
// one KV head; its cache is read once, not four times). A wave owns its 32 rows over the whole head
// dim: the Oᵀ accumulator (D/2 registers) and, at D = 64 / 128, the Q fragments (D/4) stay in registers.
// At D = 256 the 64 Q registers beside 128 of Oᵀ spilled to scratch, so there the tile's query rows sit
// in LDS and the K / V tiles are 32 keys instead of 64 (128 KB with four waves; one workgroup per CU,
// each wave with the 512-register file of a SIMD to itself). The plan (host_plan.h) takes the widest
// tile that still gives every CU a workgroup; tiles launch heaviest (largest positions) first.
//
// Per staged tile, one step per 32 keys: Sᵀ = K·Qᵀ (the key on the accumulator row, one query row per
// lane, so the softmax never leaves the lane but for one exchange between the lane halves), online
// softmax with the deferred rescale of the flash kernels — decided per ROW here, not per wave, so a
// row's result does not depend on its neighbours — then Oᵀ += Vᵀ·Pᵀ with V read transposed from LDS
// (ds_read_b64_tr_b16). Steps wholly above the wave's diagonal are skipped, the mask is applied only
// in steps that cross it, and the key loop ends at the tile's last position.
//
// Staging: a two-stage ring of K and V tiles in the paneled, XOR-swizzled image of attn_common.h
// (D/64 panels of 64 or 32 rows × 128 B). bf16 caches arrive by LDS-DMA, tile j + 1 in flight under tile
// j's MFMAs. int8 caches are loaded 16 values per lane load into registers — K of tile j + 1 under
// the score MFMAs of tile j, V under softmax and P·V — widened to bf16 (exact) and written to the
// other stage; the key's scale multiplies its score column after the MFMA, the value's scale its P
// column before P is rounded to bf16, and the softmax denominator sums the unscaled P.
// Rows at or beyond S are clamped to row S - 1 on load (finite data under P = 0; their int8 scales
// read as 0), so a NaN in an unused slot contributes nothing and nothing beyond cap is read.
// No split of the key range, no atomics: an output row depends on its q row, its keys and its
// position only, whatever Tq, B, the tile width or the grid.
#include "attn_common.h"
#include "launch_args.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {
namespace {

typedef uint32_t pf_u32x4 __attribute__((ext_vector_type(4)));  // raw 16-B piece kept in registers

__device__ __forceinline__ int pf_swz(int r) { return (((r >> 1) & 1) << 2) | ((r >> 2) & 3); }

// 4 int8 -> 4 bf16 (exact: |x| <= 128 has 8 significant bits)
__device__ __forceinline__ void pf_widen(uint32_t w, uint32_t& lo, uint32_t& hi) {
  lo = pack_bf16x2((float)(int8_t)(w & 0xff), (float)(int8_t)((w >> 8) & 0xff));
  hi = pack_bf16x2((float)(int8_t)((w >> 16) & 0xff), (float)(int8_t)(w >> 24));
}

template <int D, int NW, bool Q8>
__global__ void __launch_bounds__(64 * NW)
    prefill_attn_kernel(const bf16* __restrict__ q, const void* __restrict__ kcv, const void* __restrict__ vcv,
                        const float* __restrict__ ks, const float* __restrict__ vs, bf16* __restrict__ out, int Tq,
                        int Hkv, int gs, int cap, int S, int q_offset, float scale, int64_t q_rs, int nbh) {
  constexpr int NP = D / 64, NS = D / 16, ND = D / 32, NT = 64 * NW, BM = 32 * NW;
  // D = 256: Q fragments (64 registers) beside the 128 of Oᵀ went to scratch, so the tile's query rows sit
  // in LDS (read as B fragments per step) and the K / V tiles are 32 keys to make room for them
  constexpr bool QLDS = D >= 256;
  constexpr int BN = prefill_keys(D), NH = BN / 32;
  constexpr int TILE = BN * 128 * NP;           // one K or V tile: NP panels of BN rows × 128 B
  constexpr int QTILE = QLDS ? BM * 128 * NP : 0;
  constexpr int CPR = D / 16;                   // int8: 16-B chunks per cache row,
  constexpr int NL = Q8 ? BN * CPR / NT : 1;    // and lane loads per tile and matrix
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE + QTILE + (Q8 ? 4 * BN * 4 : 16)];
  const char* Qs = smem + 4 * TILE;
  float* sc = reinterpret_cast<float*>(smem + 4 * TILE + QTILE);  // int8: [stage][K scales BN | V scales BN]

  const int G = 1 << gs, H = Hkv << gs, PT = BM >> gs;  // positions per tile
  const int ntile = gridDim.x / nbh;
  const int qt = ntile - 1 - (int)blockIdx.x / nbh, bh = blockIdx.x % nbh;  // heaviest tiles first
  const int b = bh / Hkv, hk = bh % Hkv;
  const int tid = threadIdx.x, lane = tid & 63, w = wave_id(), hh = lane >> 5;

  // this lane's query row, and the positions of the wave's 32 rows
  const int r = 32 * w + (lane & 31);
  const int pl = qt * PT + (r >> gs), head = (hk << gs) + (r & (G - 1));
  const bool valid = pl < Tq;
  const int qpos = q_offset + pl;
  const int pw0 = qt * PT + ((32 * w) >> gs);
  const bool wact = pw0 < Tq;                                       // wave-uniform
  const int qminw = q_offset + pw0, qmaxw = q_offset + min(pw0 + (32 >> gs), Tq) - 1;
  const int kend = q_offset + min((qt + 1) * PT, Tq);               // keys this tile's rows can see
  const int ntk = (kend + BN - 1) / BN;
  const float c = scale * kLog2e;

  uint4 qf[QLDS ? 1 : NS];  // B fragment s of Qᵀ: element j = Q[row][16s + 8hh + j]
  if constexpr (QLDS) {
    // the wave's own 32 rows by LDS-DMA into the paneled image (rows beyond Tq: clamped, never stored);
    // published by the wait and barrier that publish the first K / V tile
    const unsigned qdst = __builtin_amdgcn_readfirstlane(lds_addr_of(Qs)) + 32 * w * 128;
    const int rr = lane >> 3;
#pragma unroll
    for (int r8 = 0; r8 < 4; ++r8) {
      const int rq = 32 * w + 8 * r8 + rr;
      const bf16* src = q + ((size_t)b * Tq + min(qt * PT + (rq >> gs), Tq - 1)) * q_rs + (size_t)((hk << gs) + (rq & (G - 1))) * D;
      const int lc = (lane & 7) ^ pf_swz(8 * (r8 & 1) + rr);
#pragma unroll
      for (int p = 0; p < NP; ++p) glds16(src + 64 * p + 8 * lc, qdst + (p * BM + 8 * r8) * 128);
    }
  } else {
    const bf16* qrow = q + ((size_t)b * Tq + (valid ? pl : 0)) * q_rs + (size_t)head * D;
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
  float m = -1e30f, l = 0.f;

  // ---- bf16 staging: LDS-DMA of tile j's K and V, 2·NP·BN/8 pieces (8 rows × 128 B) dealt over the waves
  const bf16* kb16 = reinterpret_cast<const bf16*>(kcv) + (size_t)bh * cap * D;
  const bf16* vb16 = reinterpret_cast<const bf16*>(vcv) + (size_t)bh * cap * D;
  auto dma = [&](int j) {
    const unsigned stage = __builtin_amdgcn_readfirstlane(lds_addr_of(smem + (j & 1) * 2 * TILE));
    const int ln = opaque_lane_id(), rr = ln >> 3;  // per-piece addresses are recomputed, not kept in registers
#pragma unroll
    for (int t = 0; t < 2 * NP * (BN / 8) / NW; ++t) {
      const int idx = t * NW + w;  // wave-uniform: matrix, panel, 8-row slab
      const int r8 = idx % (BN / 8), p = (idx / (BN / 8)) % NP, mtx = idx / (BN / 8 * NP);
      const int lc = (ln & 7) ^ pf_swz(8 * (r8 & 1) + rr);
      const int row = min(j * BN + 8 * r8 + rr, S - 1);
      glds16_s(mtx ? vb16 : kb16, (unsigned)(row * D + 64 * p + 8 * lc) * 2u, stage + mtx * TILE + (p * BN + 8 * r8) * 128);
    }
  };

  // ---- int8 staging: NL 16-B lane loads per matrix into registers, widened into the LDS image later
  const int8_t* kb8 = reinterpret_cast<const int8_t*>(kcv) + (size_t)bh * cap * D;
  const int8_t* vb8 = reinterpret_cast<const int8_t*>(vcv) + (size_t)bh * cap * D;
  auto q8_load = [&](const int8_t* base, int j, pf_u32x4 (&rg)[NL]) {
    const int ot = 64 * w + opaque_lane_id();  // addresses recomputed per call, not kept in registers
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      const int idx = t * NT + ot, row = idx / CPR, ch = idx % CPR;
      rg[t] = *reinterpret_cast<const pf_u32x4*>(base + (unsigned)(min(j * BN + row, S - 1) * D + 16 * ch));
    }
  };
  auto q8_store = [&](char* tile, const pf_u32x4 (&rg)[NL]) {
    const int ot = 64 * w + opaque_lane_id();
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      const int idx = t * NT + ot, row = idx / CPR, ch = idx % CPR;
      uint4 a, bq;
      pf_widen(rg[t].x, a.x, a.y);
      pf_widen(rg[t].y, a.z, a.w);
      pf_widen(rg[t].z, bq.x, bq.y);
      pf_widen(rg[t].w, bq.z, bq.w);
      char* pn = tile + (ch >> 2) * BN * 128;
      *reinterpret_cast<uint4*>(pn + tile_off(row, 2 * (ch & 3))) = a;
      *reinterpret_cast<uint4*>(pn + tile_off(row, 2 * (ch & 3) + 1)) = bq;
    }
  };
  auto q8_scales = [&](int j) {  // slots at or beyond S: scale 0
    const float* ksr = ks + (size_t)bh * cap;
    const float* vsr = vs + (size_t)bh * cap;
    for (int i = tid; i < 2 * BN; i += NT) {
      const int key = j * BN + (i & (BN - 1));
      sc[(j & 1) * 2 * BN + i] = key < S ? (i < BN ? ksr : vsr)[key] : 0.f;
    }
  };

  pf_u32x4 rg[NL];
  if constexpr (Q8) {
    q8_load(kb8, 0, rg);
    q8_store(smem, rg);
    q8_load(vb8, 0, rg);
    q8_store(smem + TILE, rg);
    q8_scales(0);
  } else {
    dma(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the first tile's DMA, and the Q image's
  __syncthreads();

  for (int j = 0; j < ntk; ++j) {
    const bool next = j + 1 < ntk;
    char* nstage = smem + ((j + 1) & 1) * 2 * TILE;  // released by the previous iteration's barrier
    if constexpr (Q8) {
      if (next) q8_load(kb8, j + 1, rg);
    } else {
      if (next) dma(j + 1);
    }
    const char* Kt = smem + (j & 1) * 2 * TILE;
    const char* Vt = Kt + TILE;
    const float* sct = sc + (j & 1) * 2 * BN;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {  // the tile's 32-key halves, one online-softmax step each
      const int k0 = j * BN + 32 * hf;
      const bool act = wact && k0 <= qmaxw;  // wave-uniform: not wholly above the wave's diagonal
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
      if constexpr (Q8) {
        if (hf == 0 && next) {  // K of tile j + 1 landed under the score MFMAs; V loads fly under the rest
          q8_store(nstage, rg);
          q8_load(vb8, j + 1, rg);
        }
      }
      if (act) {
        auto softmax = [&](auto mask_tag) {
          constexpr bool MASK = decltype(mask_tag)::value;
          float tmax = -INFINITY;
#pragma unroll
          for (int i4 = 0; i4 < 4; ++i4) {
            float4_t ksc = {1.f, 1.f, 1.f, 1.f};
            if constexpr (Q8) ksc = *reinterpret_cast<const float4_t*>(sct + 32 * hf + 8 * i4 + 4 * hh);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int i = 4 * i4 + k;
              float s = st[i];
              if constexpr (Q8) s *= ksc[k];
              if constexpr (MASK) s = k0 + acc_row(i, lane) > qpos ? -INFINITY : s;
              st[i] = s;
              tmax = fmaxf(tmax, s);
            }
          }
          tmax = halves_max(tmax) * c;
          // deferred rescale, decided per row: the running max only moves when it grows by more than 2^8
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
            float4_t vsc = {1.f, 1.f, 1.f, 1.f};
            if constexpr (Q8) vsc = *reinterpret_cast<const float4_t*>(sct + BN + 32 * hf + 8 * i4 + 4 * hh);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const float p = fexp2(fmaf(st[4 * i4 + k], c, negm));
              lsum += p;  // the denominator sums the unscaled P
              st[4 * i4 + k] = Q8 ? p * vsc[k] : p;
            }
          }
          l += lsum;
        };
        if (k0 + 31 > qminw)  // the half crosses some row's diagonal
          softmax(std::true_type{});
        else
          softmax(std::false_type{});
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
    if constexpr (Q8) {
      if (next) {
        q8_store(nstage + TILE, rg);
        q8_scales(j + 1);
      }
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
  }

  l = halves_sum(l);
  if (valid) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    bf16* orow = out + (((size_t)b * Tq + pl) * H + head) * D;
#pragma unroll
    for (int jd = 0; jd < ND; ++jd)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        store4(orow + 32 * jd + 8 * g + 4 * hh, o[jd][4 * g] * inv, o[jd][4 * g + 1] * inv, o[jd][4 * g + 2] * inv,
               o[jd][4 * g + 3] * inv);
  }
}

CacheKind cache_kind(at::ScalarType t) {
  return t == torch::kBFloat16 ? CacheKind::BF16 : t == torch::kInt8 ? CacheKind::I8 : CacheKind::Other;
}

}  // namespace
}  // namespace penroz

using namespace penroz;

// The launch plan (host_plan.h), for ops/attention.py and the tests: (admitted, tile rows, positions per
// tile, workgroups, LDS bytes). cache: "bf16", "int8" or anything else (refused).
std::tuple<bool, int64_t, int64_t, int64_t, int64_t> prefill_attn_plan(int64_t B, int64_t Tq, int64_t H, int64_t Hkv,
                                                                       int64_t D, bool q_bf16, const std::string& cache) {
  const CacheKind ck = cache == "bf16" ? CacheKind::BF16 : cache == "int8" ? CacheKind::I8 : CacheKind::Other;
  const PrefillAttnPlan p = plan_prefill_attn(B, Tq, H, Hkv, D, q_bf16, ck);
  return {p.ok, p.tile_rows, p.tile_pos, p.grid, p.lds_bytes};
}

// q [B, Tq, H, D] bf16 (a view into the fused QKV rows allowed) against the first S = q_offset + Tq
// slots of the caches [B, Hkv, cap, D]; -> [B, Tq, H·D]
torch::Tensor prefill_attn(torch::Tensor q, torch::Tensor kc, torch::Tensor vc, c10::optional<torch::Tensor> k_scale,
                           c10::optional<torch::Tensor> v_scale, int64_t S, int64_t q_offset, double scale) {
  const char* who = "prefill_attn";
  la_one_device(who, q, {kc, vc, k_scale, v_scale});
  // the same admission as decode_attn: unit dim stride, packed heads, a uniform row stride
  TORCH_CHECK(q.dim() == 4 && q.stride(3) == 1 && q.stride(2) == q.size(3) &&
                  (q.size(1) == 1 || q.stride(0) == q.size(1) * q.stride(1)),
              who, ": q must be [B, Tq, H, D] with packed heads and a uniform row stride");
  const int64_t B = q.size(0), Tq = q.size(1), H = q.size(2), D = q.size(3);
  const bool quant = kc.scalar_type() == torch::kInt8;
  TORCH_CHECK(kc.is_contiguous() && vc.is_contiguous() && kc.dim() == 4 && kc.sizes() == vc.sizes() && kc.size(0) == B &&
                  kc.size(3) == D && vc.scalar_type() == kc.scalar_type() && (quant || kc.scalar_type() == q.scalar_type()),
              who, ": contiguous caches [B, Hkv, cap, D] of q's dtype or int8");
  const int64_t Hkv = kc.size(1), cap = kc.size(2);
  TORCH_CHECK(Tq >= 1 && S <= cap && q_offset >= 0 && q_offset + Tq == S, who, ": bad cache extent (S = q_offset + Tq <= cap)");
  const PrefillAttnPlan p = plan_prefill_attn(B, Tq, H, Hkv, D, q.scalar_type() == torch::kBFloat16, cache_kind(kc.scalar_type()));
  TORCH_CHECK(p.ok, who, ": bf16 q, a bf16 or int8 cache, head_dim 64 / 128 / 256, H / Hkv in {1, 2, 4, 8} (decode_attn takes the rest)");
  const int64_t q_rs = Tq == 1 ? q.stride(0) : q.stride(1);
  TORCH_CHECK(la_aligned(q, 16) && q_rs % 8 == 0 && la_aligned(kc, 16) && la_aligned(vc, 16), who,
              ": q rows and the caches must be 16-B aligned");
  const float* ksp = quant ? la_f32_shape(who, "k_scale", k_scale, {B, Hkv, cap}) : nullptr;
  const float* vsp = quant ? la_f32_shape(who, "v_scale", v_scale, {B, Hkv, cap}) : nullptr;
  auto out = torch::empty({B, Tq, H * D}, q.options());
  int gs = 0;
  while ((Hkv << gs) < H) ++gs;
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto d, auto nw, auto q8) {
    constexpr int DD = decltype(d)::value, NW = decltype(nw)::value;
    constexpr bool Q8 = decltype(q8)::value != 0;
    hipLaunchKernelGGL((prefill_attn_kernel<DD, NW, Q8>), dim3((unsigned)p.grid), dim3(64 * NW), 0, stream,
                       reinterpret_cast<const bf16*>(q.data_ptr()), kc.data_ptr(), vc.data_ptr(), ksp, vsp,
                       reinterpret_cast<bf16*>(out.data_ptr()), (int)Tq, (int)Hkv, gs, (int)cap, (int)S, (int)q_offset,
                       (float)scale, q_rs, (int)(B * Hkv));
  };
  const bool ok = dispatch_exact(launch, PrefillDims{}, (int)D, PrefillWaves{}, p.tile_rows / 32, IntList<0, 1>{}, (int)quant);
  TORCH_CHECK(ok, who, ": no kernel for the planned tile");
  return out;
}

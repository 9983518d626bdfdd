// Decode GEMV for M <= 4 rows on int8 weight rows with one fp32 scale per row (weight-only
// quantisation): out[M, N] = act(scale[n] · (x · Qᵀ)[m, n] + bias). The bf16 decode GEMV
// (decode_linear.hip decode_gemv_kernel) is bound by the weight bytes it reads; this one reads half
// of them. Same structure and the same forms:
//   * one wave per workgroup, no LDS, no barrier; a half-wave (32 lanes) owns one weight row, or
//     the whole wave one row (wave-per-row form);
//   * every load of the wave — weight chunks, x (or residual / delta / dbias / γ / β) chunks, the
//     row scales and bias terms — is issued before the first use, and none is conditional (hipcc
//     branches around a conditional load and waits for everything in flight there): one memory
//     round trip. (The LN forms at 3-4 rows and K near 1024 issue 64-88 loads, more than the 63 the
//     outstanding-load counter holds, so the compiler has to wait inside their load phase.)
//   * a 16-B weight chunk holds 16 weights and pairs with two 16-B chunks of x (K % 16 == 0);
//   * int8 -> bf16 in registers: the fp32 conversion of |q| <= 127 has at most 7 significant bits,
//     so its high half IS the bf16 value, exactly; products by v_dot2c_f32_bf16 into fp32;
//   * scale[n] multiplies the reduced sum once per (row, x row), before the bias; every later
//     rounding point is where the bf16 kernel has it (GELU on the bf16-rounded linear output, both
//     halves of a pair rounded to bf16 before the gated activation / the rotation).
// PRO 1 (LN mode): x = LayerNorm(resid_in + delta + dbias), the sum written to resid_out by
// workgroup 0. EPI 0 independent rows, 1 gated pair on the packed [gate; up] rows, 2 RoPE QKV pair,
// 3 wave-per-row (decode_gemv_kernel's numbering). The embedding-gather prologue has no int8 form.
#include "common.h"
#include "host_plan.h"
#include "launch_args.h"
#include <tuple>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {

typedef __bf16 q8_bf16x2 __attribute__((ext_vector_type(2)));

// bytes 2j, 2j + 1 of w (int8) as one bf16 pair: the high halves of their fp32 conversions
__device__ __forceinline__ uint32_t q8_pair(uint32_t w, int j) {
  const float lo = (float)(int)(int8_t)(w >> (16 * j));
  const float hi = (float)(int)(int8_t)(w >> (16 * j + 8));
  return (__float_as_uint(hi) & 0xffff0000u) | (__float_as_uint(lo) >> 16);
}

struct Q8x16 {  // 16 weights of one chunk as 8 bf16 pairs, in K order
  uint32_t p[8];
};

__device__ __forceinline__ Q8x16 q8_unpack(const uint4& w) {
  Q8x16 r;
  r.p[0] = q8_pair(w.x, 0); r.p[1] = q8_pair(w.x, 1); r.p[2] = q8_pair(w.y, 0); r.p[3] = q8_pair(w.y, 1);
  r.p[4] = q8_pair(w.z, 0); r.p[5] = q8_pair(w.z, 1); r.p[6] = q8_pair(w.w, 0); r.p[7] = q8_pair(w.w, 1);
  return r;
}

__device__ __forceinline__ float q8_dot2(uint32_t a, uint32_t b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(q8_bf16x2, a), __builtin_bit_cast(q8_bf16x2, b), c, false);
}

// 16 weights · the two x chunks (8 bf16 each) they pair with
__device__ __forceinline__ float q8_dot16(const Q8x16& w, const uint4& x0, const uint4& x1, float c) {
  c = q8_dot2(w.p[0], x0.x, c); c = q8_dot2(w.p[1], x0.y, c); c = q8_dot2(w.p[2], x0.z, c); c = q8_dot2(w.p[3], x0.w, c);
  c = q8_dot2(w.p[4], x1.x, c); c = q8_dot2(w.p[5], x1.y, c); c = q8_dot2(w.p[6], x1.z, c); c = q8_dot2(w.p[7], x1.w, c);
  return c;
}

__device__ __forceinline__ float q8_half_sum(float v) {  // sum over the 32 lanes of this half-wave
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void q8_ld4(const float* p, float* v) {
  const float4_t a = *reinterpret_cast<const float4_t*>(p);
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
}

// CPL: 16-B weight chunks (16 weights) per lane. Template arguments as decode_gemv_kernel's.
template <int M, int PRO, int RP, int CPL, int EPI = 0>
__global__ void __launch_bounds__(64) decode_gemv_q8_kernel(
    const float* __restrict__ rin, const bf16* __restrict__ delta, const float* __restrict__ dbias,
    float* __restrict__ rout, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
    const bf16* __restrict__ x, int64_t x_rs, const int8_t* __restrict__ w, const float* __restrict__ scale,
    const bf16* __restrict__ bias, bf16* __restrict__ out, int64_t o_rs, int N, int K, int act, int D, int nrot,
    const float* __restrict__ cosv, const float* __restrict__ sinv) {
  constexpr bool LN = PRO == 1;
  constexpr bool WR = EPI == 3;     // the whole wave on each of its rows: lane l reads chunks l, l + 64, …
  constexpr int CS = WR ? 64 : 32;  // lanes striding over a row's chunks
  static_assert(!WR || PRO == 0, "wave-per-row mode reads a bf16 x");
  static_assert(!LN || EPI == 0, "LN mode has independent rows");
  const int lane = threadIdx.x, h = lane >> 5, l32 = lane & 31;
  const int cl = WR ? lane : l32;
  const int nc = K / 16;  // 16-B weight chunks per row
  const int n0 = blockIdx.x * (EPI == 0 ? 2 * RP : RP);
  const int npair = N / 2;  // modes 1 / 2: output pairs
  auto row_of = [&](int rp) -> int {  // this half's weight row for its rp-th row (pair), clamped into [0, N)
    if constexpr (WR) {
      return min(n0 + rp, N - 1);
    } else if constexpr (EPI == 0) {
      return min(n0 + 2 * rp + h, N - 1);
    } else if constexpr (EPI == 1) {
      return min(n0 + rp, npair - 1) + h * npair;
    } else {
      const int p = min(n0 + rp, npair - 1), hd = D / 2, head = p / hd;
      return head * D + (p - head * hd) + h * hd;
    }
  };
  // 1. every load first, and every load unconditional: a chunk index past the row's end is clamped
  // to the last chunk (an in-bounds address) and the weight chunk zeroed when it is used, so no
  // branch — and with it no wait — stands between two loads. Absent optional operands (bias, delta,
  // dbias) read a valid stand-in address and are dropped by a select.
  auto chunk_of = [&](int i) -> int { return min(cl + CS * i, nc - 1); };
  uint4 wv[RP][CPL];
  float sc[RP];
  uint16_t braw[RP];
  const uint16_t* bsrc = bias ? reinterpret_cast<const uint16_t*>(bias) : reinterpret_cast<const uint16_t*>(scale);
#pragma unroll
  for (int rp = 0; rp < RP; ++rp) {
    const int n = row_of(rp);
    const int8_t* wr = w + (size_t)n * K;
#pragma unroll
    for (int i = 0; i < CPL; ++i) wv[rp][i] = *reinterpret_cast<const uint4*>(wr + 16 * chunk_of(i));
    sc[rp] = scale[n];
    braw[rp] = bsrc[n];
  }
  uint4 xb[M][CPL][2];
  if constexpr (!LN) {
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const uint4* xp = reinterpret_cast<const uint4*>(x + (size_t)m * x_rs + 16 * chunk_of(i));
        xb[m][i][0] = xp[0];
        xb[m][i][1] = xp[1];
      }
    // the scheduler may not sink a load below this point (towards its use, behind a wait), nor hoist
    // arithmetic above it
    __builtin_amdgcn_sched_barrier(0);
  } else {
    float v[M][CPL][16], g[CPL][16], bt[CPL][16];
    // stand-ins of the same extent: resid_in [M, K] fp32 for the bf16 delta, gamma [K] for dbias
    const bf16* dsrc = delta ? delta : reinterpret_cast<const bf16*>(rin);
    const float* esrc = dbias ? dbias : gamma;
    const bool has_d = delta != nullptr, has_e = delta != nullptr && dbias != nullptr;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const int c = chunk_of(i);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        q8_ld4(gamma + 16 * c + 4 * q, &g[i][4 * q]);
        q8_ld4(beta + 16 * c + 4 * q, &bt[i][4 * q]);
      }
    }
    float e[CPL][16];
#pragma unroll
    for (int i = 0; i < CPL; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) q8_ld4(esrc + 16 * chunk_of(i) + 4 * q, &e[i][4 * q]);
    uint4 draw[M][CPL][2];  // delta chunks as loaded: converted after the load phase
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const int c = chunk_of(i);
#pragma unroll
        for (int q = 0; q < 4; ++q) q8_ld4(rin + (size_t)m * K + 16 * c + 4 * q, &v[m][i][4 * q]);
        const uint4* dp = reinterpret_cast<const uint4*>(dsrc + (size_t)m * K + 16 * c);
        draw[m][i][0] = dp[0];
        draw[m][i][1] = dp[1];
      }
    __builtin_amdgcn_sched_barrier(0);  // (as above: every load is issued by here)
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const bool ok = l32 + 32 * i < nc;
        const uint4 d0 = draw[m][i][0], d1 = draw[m][i][1];
        const uint32_t dw[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const float dv = __uint_as_float(k & 1 ? dw[k >> 1] & 0xffff0000u : dw[k >> 1] << 16);
          const float dk = has_d ? dv + (has_e ? e[i][k] : 0.f) : 0.f;
          v[m][i][k] = ok ? v[m][i][k] + dk : 0.f;
        }
      }
    if (delta && rout && blockIdx.x == 0 && h == 0) {
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
          const int c = l32 + 32 * i;
          if (c < nc) {
            float4_t* op = reinterpret_cast<float4_t*>(rout + (size_t)m * K + 16 * c);
#pragma unroll
            for (int q = 0; q < 4; ++q)
              op[q] = float4_t{v[m][i][4 * q], v[m][i][4 * q + 1], v[m][i][4 * q + 2], v[m][i][4 * q + 3]};
          }
        }
    }
    // LayerNorm within the half-wave: fp32 two-pass on the register copy, rounded to bf16
    const float inv_k = 1.f / (float)K;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < CPL; ++i)
#pragma unroll
        for (int k = 0; k < 16; ++k) s += v[m][i][k];
      const float mean = q8_half_sum(s) * inv_k;
      float ss = 0.f;
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const bool ok = l32 + 32 * i < nc;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const float d = v[m][i][k] - mean;
          ss += ok ? d * d : 0.f;
        }
      }
      const float rstd = rsqrtf(q8_half_sum(ss) * inv_k + eps);
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        float y[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) y[k] = (v[m][i][k] - mean) * rstd * g[i][k] + bt[i][k];
        xb[m][i][0] = uint4{pack_bf16x2(y[0], y[1]), pack_bf16x2(y[2], y[3]), pack_bf16x2(y[4], y[5]),
                            pack_bf16x2(y[6], y[7])};
        xb[m][i][1] = uint4{pack_bf16x2(y[8], y[9]), pack_bf16x2(y[10], y[11]), pack_bf16x2(y[12], y[13]),
                            pack_bf16x2(y[14], y[15])};
      }
    }
  }
  // the scales and bias terms are used by the storing lanes only: without a use here their loads
  // are sunk into the epilogue, a second memory round trip
#pragma unroll
  for (int rp = 0; rp < RP; ++rp) asm volatile("" ::"v"(sc[rp]), "v"((uint32_t)braw[rp]));
  // 2. products (each weight chunk converted once, used by every x row), reductions, row scales
  float acc[RP][M];
#pragma unroll
  for (int rp = 0; rp < RP; ++rp) {
#pragma unroll
    for (int m = 0; m < M; ++m) acc[rp][m] = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const bool ok = cl + CS * i < nc;  // (a clamped chunk was loaded: it counts as zeros)
      const uint4 wz = wv[rp][i];
      const Q8x16 wq = q8_unpack(uint4{ok ? wz.x : 0u, ok ? wz.y : 0u, ok ? wz.z : 0u, ok ? wz.w : 0u});
#pragma unroll
      for (int m = 0; m < M; ++m) acc[rp][m] = q8_dot16(wq, xb[m][i][0], xb[m][i][1], acc[rp][m]);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float a = q8_half_sum(acc[rp][m]);
      if constexpr (WR) a += __shfl_xor(a, 32, 64);
      acc[rp][m] = a * sc[rp];
    }
  }
  // 3. epilogue: lane 0 of each half stores its rows
  if constexpr (WR) {
    if (lane != 0) return;
#pragma unroll
    for (int rp = 0; rp < RP; ++rp) {
      const int n = n0 + rp;
      if (n >= N) continue;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        float y = acc[rp][m] + (bias ? bf2f(braw[rp]) : 0.f);
        if (act) y = gelu_f(bf2f(from_f<bf16>(y)), act - 1);
        out[(size_t)m * o_rs + n] = from_f<bf16>(y);
      }
    }
  } else if constexpr (EPI != 0) {
    float other[RP][M];  // the partner half's scaled sums (lane 0 <-> lane 32)
#pragma unroll
    for (int rp = 0; rp < RP; ++rp)
#pragma unroll
      for (int m = 0; m < M; ++m) other[rp][m] = __shfl_xor(acc[rp][m], 32, 64);
    if (l32 != 0) return;
#pragma unroll
    for (int rp = 0; rp < RP; ++rp) {
      const int p = n0 + rp;
      if (p >= npair) continue;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const float mine = bf2f(from_f<bf16>(acc[rp][m])), theirs = bf2f(from_f<bf16>(other[rp][m]));
        if constexpr (EPI == 1) {
          if (h == 0) out[(size_t)m * o_rs + p] = from_f<bf16>(act_f(mine, act) * theirs);
        } else {
          const int hd = D / 2, head = p / hd, j = p - head * hd;
          float y = mine;
          if (head < nrot) {
            const float cs = cosv[j], sn = sinv[j];
            y = h == 0 ? mine * cs - theirs * sn : mine * cs + theirs * sn;
          }
          out[(size_t)m * o_rs + head * D + j + h * hd] = from_f<bf16>(y);
        }
      }
    }
  } else {
    if (l32 != 0) return;
#pragma unroll
    for (int rp = 0; rp < RP; ++rp) {
      const int n = n0 + 2 * rp + h;
      if (n >= N) continue;
#pragma unroll
      for (int m = 0; m < M; ++m) {
        float y = acc[rp][m] + (bias ? bf2f(braw[rp]) : 0.f);
        if (act) y = gelu_f(bf2f(from_f<bf16>(y)), act - 1);
        out[(size_t)m * o_rs + n] = from_f<bf16>(y);
      }
    }
  }
}

}  // namespace penroz

using namespace penroz;

// (rows, K, LN-mode K, paired-row K, K multiple) the two launchers below accept: the Python
// admission checks (models/graph_decode.py) read them here instead of repeating them
std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t> decode_gemv_q8_limits() {
  return {kGemvMaxRows, kGemvMaxK, kLnMaxK, kGemvPairMaxK, kGemvQ8KMult};
}

// The launch plans (host_plan.h), for tests: (form 0 half-wave / 1 wave-per-row / 2 LN, rows, row
// pairs per wave, chunks per lane, grid) and (pairs per wave, chunks per lane, grid)
std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t> decode_gemv_q8_plan(int64_t M, int64_t N, int64_t K, bool ln,
                                                                            int64_t rows_per_wave) {
  const GemvPlan p = plan_decode_gemv_q8((int)M, (int)N, (int)K, ln, (int)rows_per_wave);
  return {(int64_t)p.form, p.m, p.rp, p.cpl, p.grid};
}
std::tuple<int64_t, int64_t, int64_t> decode_gemv_q8_pair_plan(int64_t N, int64_t K, int64_t pairs_per_wave) {
  const GemvPairPlan p = plan_decode_gemv_q8_pair((int)N, (int)K, (int)pairs_per_wave);
  return {p.ppw, p.cpl, p.grid};
}

// out[M, N] = act(scale ⊙ (x · qᵀ) + bias) for M <= 4 decode rows (decode_gemv_q8_kernel). LN mode
// (x undefined): x = LayerNorm(resid_in + delta + dbias) with γ / β, resid_out receives the sum.
// act 0 none, 1 GELU (erf), 2 GELU (tanh). rows_per_wave 2, 4 or 8 at most (0: by N).
void decode_gemv_q8(c10::optional<torch::Tensor> x, c10::optional<torch::Tensor> rin, c10::optional<torch::Tensor> delta,
                    c10::optional<torch::Tensor> dbias, c10::optional<torch::Tensor> rout,
                    c10::optional<torch::Tensor> gamma, c10::optional<torch::Tensor> beta, double eps, torch::Tensor q,
                    torch::Tensor scale, c10::optional<torch::Tensor> bias, torch::Tensor out, int64_t act,
                    int64_t rows_per_wave) {
  const char* who = "decode_gemv_q8";
  const bool ln = !la_defined(x);
  const Q8Weight W = la_weight_q8(who, q, scale);
  const int N = W.N, K = W.K;
  TORCH_CHECK(K <= kGemvMaxK, who, ": K <= ", kGemvMaxK);
  TORCH_CHECK(act >= 0 && act <= 2, who, ": act 0 (none), 1 (GELU erf), 2 (GELU tanh)");
  int M;
  const bf16* xp = nullptr;
  int64_t x_rs = 0;
  ResidArgs r;
  const float *gp = nullptr, *bt = nullptr;
  if (!ln) {
    xp = la_rows(who, *x, K);
    M = x->size(0);
    x_rs = x->stride(0);
  } else {
    TORCH_CHECK(K <= kLnMaxK, who, ": LN mode needs K <= ", kLnMaxK);
    gp = la_f32_vec(who, "gamma", gamma, K);
    bt = la_f32_vec(who, "beta", beta, K);
    r = la_resid(who, rin, delta, dbias, rout, K, true);
    M = r.M;
  }
  TORCH_CHECK(M >= 1 && M <= kGemvMaxRows, who, ": 1..", kGemvMaxRows, " rows");
  bf16* op = la_out(who, out, M, N);
  const bf16* bp = la_bias(who, bias, N);
  const GemvPlan p = plan_decode_gemv_q8(M, N, K, ln, (int)rows_per_wave);
  TORCH_CHECK(p.rp > 0, who, ": rows_per_wave 2, 4 or 8");
  auto stream = at::hip::getCurrentHIPStream();
  bool fits = true;
  auto launch = [&](auto m, auto pro, auto rp, auto cpl, auto epi) {  // decode_gemv_q8_kernel's template arguments
    constexpr int MM = decltype(m)::value, PP = decltype(pro)::value, RR = decltype(rp)::value,
                  CC = decltype(cpl)::value, EE = decltype(epi)::value;
    if constexpr (PP == 1 || gemv_q8_fits(MM, RR, CC)) {
      hipLaunchKernelGGL((decode_gemv_q8_kernel<MM, PP, RR, CC, EE>), dim3(p.grid), dim3(64), 0, stream, r.rin, r.delta,
                         r.dbias, r.rout, gp, bt, (float)eps, xp, x_rs, W.q, W.scale, bp, op, (int64_t)out.stride(0), N, K,
                         (int)act, 0, 0, (const float*)nullptr, (const float*)nullptr);
    } else {
      fits = false;  // (the plan never picks a combination above the register budget)
    }
  };
  const bool ok =
      p.form == GemvForm::WaveRow
          ? dispatch_exact(launch, GemvRows{}, p.m, IntList<0>{}, 0, IntList<1>{}, p.rp, GemvQ8CplWave{}, p.cpl, IntList<3>{}, 3)
      : ln ? dispatch_exact(launch, GemvRows{}, p.m, IntList<1>{}, 1, Pow2To4{}, p.rp, GemvQ8CplLn{}, p.cpl, IntList<0>{}, 0)
           : dispatch_exact(launch, GemvRows{}, p.m, IntList<0>{}, 0, Pow2To4{}, p.rp, GemvQ8CplHalf{}, p.cpl, IntList<0>{}, 0);
  TORCH_CHECK(ok && fits, who, ": no kernel for M = ", M, ", K = ", K);
}

// Paired-row int8-weight decode GEMV for 1..4 rows on a bf16 x (decode_gemv_q8_kernel modes 1 / 2):
//   mode 1 (gated): out[M, I] = act_f(x·Wgᵀ, kind) ⊙ (x·Wuᵀ), q = [Wg; Wu] [2I, K];
//   mode 2 (RoPE QKV): out[M, (H + 2Hkv)·D] = rope(x · Wᵀ) for the first nrot heads, cos / sin [D/2].
void decode_gemv_q8_pair(torch::Tensor x, torch::Tensor q, torch::Tensor scale, torch::Tensor out, int64_t mode,
                         int64_t kind, int64_t D, int64_t nrot, c10::optional<torch::Tensor> cosv,
                         c10::optional<torch::Tensor> sinv, int64_t pairs_per_wave) {
  const char* who = "decode_gemv_q8_pair";
  TORCH_CHECK(mode == 1 || mode == 2, who, ": mode 1 (gated) or 2 (RoPE)");
  const Q8Weight W = la_weight_q8(who, q, scale, 2);
  const int N = W.N, K = W.K;
  TORCH_CHECK(K <= kGemvPairMaxK, who, ": K <= ", kGemvPairMaxK);
  const bf16* xp = la_rows(who, x, K);
  const int M = x.size(0);
  TORCH_CHECK(M >= 1 && M <= kGemvMaxRows, who, ": 1..", kGemvMaxRows, " rows");
  bf16* op = la_out(who, out, M, mode == 1 ? N / 2 : N);
  const float *cp = nullptr, *sp = nullptr;
  if (mode == 1) {
    TORCH_CHECK(kind >= 0 && kind <= 2, who, ": kind 0 gelu, 1 gelu_tanh, 2 silu");
  } else {
    TORCH_CHECK(D >= 2 && D % 2 == 0 && N % D == 0 && nrot >= 0 && nrot <= N / D, who, ": RoPE geometry");
    cp = la_f32_vec(who, "cos", cosv, D / 2, true);
    sp = la_f32_vec(who, "sin", sinv, D / 2, true);
  }
  const GemvPairPlan p = plan_decode_gemv_q8_pair(N, K, (int)pairs_per_wave);
  TORCH_CHECK(p.ppw > 0, who, ": pairs_per_wave 1, 2 or 4");
  auto stream = at::hip::getCurrentHIPStream();
  auto launch = [&](auto m, auto rp, auto cpl, auto epi) {
    constexpr int EE = decltype(epi)::value;
    hipLaunchKernelGGL((decode_gemv_q8_kernel<decltype(m)::value, 0, decltype(rp)::value, decltype(cpl)::value, EE>),
                       dim3(p.grid), dim3(64), 0, stream, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, xp,
                       (int64_t)x.stride(0), W.q, W.scale, nullptr, op, (int64_t)out.stride(0), N, K,
                       EE == 1 ? (int)kind : 0, (int)D, (int)nrot, cp, sp);
  };
  const bool ok = dispatch_exact(launch, GemvRows{}, M, Pow2To4{}, p.ppw, GemvQ8CplPair{}, p.cpl, IntList<1, 2>{}, (int)mode);
  TORCH_CHECK(ok, who, ": no kernel for M = ", M, ", K = ", K);
}

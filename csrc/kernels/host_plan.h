// Host-side launch planning shared by the HIP launch wrappers — plain C++ (no HIP headers), so
// the same code is also compiled into tests/native/host_plan_test.cpp and run under the host
// AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_host_sanitizers.py).
#pragma once
#include "dispatch.h"

#include <algorithm>
#include <cstdint>

namespace penroz {

struct SplitK {
  int splits;  // workgroups per output tile along K
  int klen;    // K range of one split (multiple of bk)
};

// Split-K count for the weight-gradient GEMM from a wave-quantisation cost model: the launch runs
// ceil(ntiles·s / slots) waves of workgroups, each 1/s of the K loop long, plus the fp32 slab
// round trip (s slabs written and read once) priced against the per-workgroup MFMA time.
// slots = resident workgroups (1 per CU for the 256-tile kernel, 2 for the 128-tile one).
inline SplitK plan_wgrad_splits(int M, int N, int K, int tile, int n_cu, int bk) {
  SplitK r{1, 0};
  if (M <= 0 || N <= 0 || K <= 0 || tile <= 0 || bk <= 0) return r;
  const int64_t tiles_m = (M + tile - 1) / tile, tiles_n = (N + tile - 1) / tile;
  const int64_t ntiles = tiles_m * tiles_n;
  const int64_t slots = tile == 256 ? std::max(1, n_cu) : 2 * (int64_t)std::max(1, n_cu);
  const double wg_full_k = (double)tile * tile * 2.0 * K / (tile == 256 ? 2.3e12 : 1.1e12);  // seconds
  double best = 1e30;
  const int smax = std::min(64, std::max(1, K / 512));
  for (int s = 1; s <= smax; ++s) {
    const double waves = (double)((ntiles * s + slots - 1) / slots);
    const double slab = s > 1 ? (double)s * M * N * 8.0 / 4.0e12 : 0.0;
    const double cost = waves * wg_full_k / s + slab;
    if (cost < best * 0.995) best = cost, r.splits = s;
  }
  const int64_t per = ((int64_t)K + r.splits - 1) / r.splits;
  r.klen = (int)((per + bk - 1) / bk * bk);
  r.splits = (int)(((int64_t)K + r.klen - 1) / r.klen);
  return r;
}

// Weight-gradient launch plan with a split TAIL: when the output tiles take more than one round of
// workgroups (one per CU) and the last round is mostly empty, the tiles of the full rounds run
// unsplit (direct read-add-write of the gradient, no slab) and only the last round's tiles are
// split along K, so that round is as full as the CUs allow and takes 1/tail_splits of a tile's
// time. GPT-2 lm_head (591 tiles): 2 + 1/3 rounds instead of 3 (or 5 half-rounds plus two
// full-size slabs). Falls back to the uniform plan above whenever that prices lower.
struct WgradPlan {
  int main_tiles;   // tiles [0, main_tiles): main_splits each
  int main_splits;  // 1 = direct into the gradient, > 1 = full-size fp32 slabs
  int main_klen;
  int tail_splits;  // tiles [main_tiles, ntiles): tail_splits each into per-tile slabs (0: none)
  int tail_klen;
};

inline WgradPlan plan_wgrad(int M, int N, int K, int tile, int n_cu, int bk) {
  const SplitK u = plan_wgrad_splits(M, N, K, tile, n_cu, bk);
  WgradPlan r{0, u.splits, u.klen, 0, 0};
  if (M <= 0 || N <= 0 || K <= 0 || tile != 256 || bk <= 0) {
    r.main_tiles = (M > 0 && N > 0 && tile > 0) ? (int)(((int64_t)(M + tile - 1) / tile) * ((N + tile - 1) / tile)) : 0;
    return r;
  }
  const int64_t ntiles = (int64_t)((M + tile - 1) / tile) * ((N + tile - 1) / tile);
  r.main_tiles = (int)ntiles;
  const int64_t slots = std::max(1, n_cu);
  if (ntiles <= slots) return r;
  const double wg_full_k = (double)tile * tile * 2.0 * K / 2.3e12;
  auto uniform_cost = [&](int s) {
    const double waves = (double)((ntiles * s + slots - 1) / slots);
    return waves * wg_full_k / s + (s > 1 ? (double)s * M * N * 8.0 / 4.0e12 : 0.0);
  };
  const int64_t rounds = (ntiles + slots - 1) / slots;
  const int64_t tail = ntiles - (rounds - 1) * slots;
  const int st = (int)std::min<int64_t>({64, slots / tail, std::max(1, K / 512)});
  if (st < 2) return r;
  const double tail_cost = (double)(rounds - 1) * wg_full_k + wg_full_k / st +
                           (double)tail * st * tile * tile * 8.0 / 4.0e12;
  if (tail_cost >= uniform_cost(u.splits) * 0.995) return r;
  r.main_tiles = (int)(ntiles - tail);
  r.main_splits = 1;
  r.main_klen = (int)(((int64_t)K + bk - 1) / bk * bk);
  const int64_t per = ((int64_t)K + st - 1) / st;
  r.tail_klen = (int)((per + bk - 1) / bk * bk);
  r.tail_splits = (int)(((int64_t)K + r.tail_klen - 1) / r.tail_klen);
  return r;
}

// Slices of the two-stage deterministic column reduction (reduce.h): ~sqrt(G) balances stages.
inline int reduce_slices(int G) {
  int s = 1;
  while ((int64_t)s * s < G) ++s;
  return s;
}

// ---- decode GEMM / GEMV launch plans (decode_linear.hip, skinny_gemm.hip) ----

// Limits the launch checks enforce; graph_decode.py reads the GEMV ones (decode_gemv_limits).
constexpr int kGemvMaxRows = 4;      // decode_gemv / decode_gemv_pair rows
constexpr int kGemvMaxK = 8192;      // 32 chunks of 8 per lane × 32 lanes
constexpr int kLnMaxK = 1024;        // LN mode: the normalised row lives in registers / LDS
constexpr int kGemvPairMaxK = 1792;  // 7 chunks per lane, the widest paired-row instantiation
constexpr int kSkinnyMaxRows = 64;   // skinny_* / decode_ln_linear rows (4 MFMA row blocks)

// Template arguments instantiated per launcher form; the chunk lists are buckets (first >= need).
using GemvRows = IntList<1, 2, 3, 4>;
using Pow2To4 = IntList<1, 2, 4>;  // MB, RP, pairs per wave
using GemvCplHalf = IntList<1, 2, 3, 4, 5, 7, 12, 16, 25, 32>;
using GemvCplLn = IntList<3, 4>;  // LN mode instantiates only the small chunk counts (K <= 1024)
using GemvCplWave = IntList<2, 4, 7, 16>;
using GemvCplPair = IntList<3, 4, 5, 7>;

template <int... Vs>
int bucket_of(IntList<Vs...> list, int v) {  // 0: above every bucket
  int b = 0;
  dispatch_bucket([&](auto c) { b = decltype(c)::value; }, list, v);
  return b;
}

// 16-row MFMA blocks per workgroup of the skinny kernels
inline int row_blocks(int M) { return M <= 16 ? 1 : M <= 32 ? 2 : 4; }

enum class GemvForm { HalfWave, WaveRow, LN };
struct GemvPlan {
  GemvForm form;
  int m;     // kernel template arguments: rows,
  int rp;    // row pairs per wave (wave-per-row: 1 row; 0: bad rows_per_wave),
  int cpl;   // 16-B chunks per lane (0: K has no instantiation in this form)
  int grid;  // workgroups of one wave
  int rows_per_wg() const { return form == GemvForm::WaveRow ? 1 : 2 * rp; }
};

// rows_per_wave 2, 4 or 8 (<= 0: chosen here); rpw_env / wave_row_env: PENROZ_DECODE_GEMV_RPW
// (0: unset) and PENROZ_DECODE_GEMV_WAVE_ROW (true unless "0").
inline GemvPlan plan_decode_gemv(int M, int N, int K, bool ln, int rows_per_wave, int rpw_env, bool wave_row_env) {
  int rpw = rows_per_wave;
  // by shape: the vocabulary projection wants fewer, longer-lived waves (8 rows); everything else
  // 2 rows per wave — the most workgroups in flight. In the replayed step that beat 4 rows for the
  // wider QKV / fc outputs, which the isolated microbench preferred (GPT-2 B = 1 0.3594 / 0.3608 ->
  // 0.3563 / 0.3547 ms, Gemma-3 1B neutral; profiles/decode_r5.md). PENROZ_DECODE_GEMV_RPW forces 2 /
  // 4 / 8 below 16k rows (A/B).
  if (rpw <= 0 && rpw_env > 0 && N < 16384) rpw = rpw_env;
  if (rpw <= 0) rpw = N >= 16384 ? 8 : 2;
  const bool rpw_ok = rpw == 2 || rpw == 4 || rpw == 8;
  // wave-per-row form for the bf16-x GEMVs (proj, fc2, Gemma o / down): one row per wave, the
  // whole wave striding over K — twice the workgroups. Same box: Gemma-3 1B B = 1 1.2626 / 1.2621 ->
  // 1.2577 / 1.2555 ms, GPT-2 B = 4 0.549 / 0.544 -> 0.544 / 0.542, GPT-2 B = 1 even
  // (profiles/decode_r5.md). PENROZ_DECODE_GEMV_WAVE_ROW=0: the half-wave form.
  const bool wave_row = wave_row_env && !ln && rows_per_wave <= 0 && N < 16384;
  const int chunks = K / 8;
  if (wave_row) return {GemvForm::WaveRow, M, rpw_ok ? 1 : 0, bucket_of(GemvCplWave{}, (chunks + 63) / 64), N};
  const int cpl = (chunks + 31) / 32;
  return {ln ? GemvForm::LN : GemvForm::HalfWave, M, rpw_ok ? rpw / 2 : 0,
          ln ? bucket_of(GemvCplLn{}, cpl) : bucket_of(GemvCplHalf{}, cpl), (N + rpw - 1) / rpw};
}

struct GemvPairPlan {
  int ppw;   // output pairs per wave (0: bad pairs_per_wave)
  int cpl;   // 0: K > kGemvPairMaxK
  int grid;
};

// N weight rows = N / 2 output pairs; pairs_per_wave 1, 2 or 4 (<= 0: by the number of pairs)
inline GemvPairPlan plan_decode_gemv_pair(int N, int K, int pairs_per_wave) {
  int ppw = pairs_per_wave;
  if (ppw <= 0) ppw = N / 2 >= 16384 ? 4 : N / 2 <= 1024 ? 1 : 2;
  const bool ppw_ok = ppw == 1 || ppw == 2 || ppw == 4;
  return {ppw_ok ? ppw : 0, bucket_of(GemvCplPair{}, (K / 8 + 31) / 32), (N / 2 + ppw - 1) / ppw};
}

// ---- int8-weight decode GEMV (decode_gemv_q8.hip): W = int8 rows [N, K] + one fp32 scale per row ----
// A 16-B weight chunk holds 16 weights and pairs with two 16-B x chunks, so K % 16 == 0 and a lane
// holds half the chunks of the bf16 kernel for the same K. The K limits are the bf16 kernel's.
constexpr int kGemvQ8KMult = 16;
using GemvQ8CplHalf = IntList<1, 2, 3, 4, 8, 16>;  // 32 lanes × 16 weights: 512 of K per chunk
using GemvQ8CplWave = IntList<1, 2, 3, 4, 7, 8>;   // 64 lanes × 16 weights: 1024 of K per chunk
using GemvQ8CplLn = IntList<1, 2>;                 // K <= kLnMaxK
using GemvQ8CplPair = IntList<2, 3, 4>;            // K <= kGemvPairMaxK
static_assert(16 * 512 >= kGemvMaxK && 8 * 1024 >= kGemvMaxK && 2 * 512 >= kLnMaxK && 4 * 512 >= kGemvPairMaxK,
              "the widest chunk bucket of every form covers its K limit");

// Every load of a wave is in flight before the first use, so a lane holds all its chunks at once:
// 4 VGPRs per weight chunk and row (pair) of the wave, 8 per chunk and x row. Combinations above
// this budget (of the 512 VGPRs a one-wave workgroup can have) are not instantiated: they would
// spill to scratch. The plan below never picks one.
constexpr int kGemvQ8RegBudget = 416;
constexpr bool gemv_q8_fits(int m, int rp, int cpl) { return cpl * (4 * rp + 8 * m) <= kGemvQ8RegBudget; }

// plan_decode_gemv's shape rule (8 rows per wave for the vocabulary projection, else 2; the
// wave-per-row form for the bf16-x GEMVs below 16k rows), without its A/B environment switches.
// rows_per_wave 2, 4 or 8 is an upper bound here: it is halved until the wave's registers fit, and a
// shape whose single row pair does not fit takes the wave-per-row form (half the chunks per lane).
inline GemvPlan plan_decode_gemv_q8(int M, int N, int K, bool ln, int rows_per_wave) {
  int rpw = rows_per_wave > 0 ? rows_per_wave : (N >= 16384 ? 8 : 2);
  const bool rpw_ok = rpw == 2 || rpw == 4 || rpw == 8;
  const int chunks = K / kGemvQ8KMult;
  bool wave_row = !ln && rows_per_wave <= 0 && N < 16384;
  const int cpl = (chunks + 31) / 32;
  const int cb = ln ? bucket_of(GemvQ8CplLn{}, cpl) : bucket_of(GemvQ8CplHalf{}, cpl);
  if (!ln && !wave_row && rpw_ok && cb > 0) {
    while (rpw > 2 && !gemv_q8_fits(M, rpw / 2, cb)) rpw /= 2;
    wave_row = !gemv_q8_fits(M, rpw / 2, cb);
  }
  if (wave_row) return {GemvForm::WaveRow, M, rpw_ok ? 1 : 0, bucket_of(GemvQ8CplWave{}, (chunks + 63) / 64), N};
  return {ln ? GemvForm::LN : GemvForm::HalfWave, M, rpw_ok ? rpw / 2 : 0, cb, (N + rpw - 1) / rpw};
}

inline GemvPairPlan plan_decode_gemv_q8_pair(int N, int K, int pairs_per_wave) {
  int ppw = pairs_per_wave;
  if (ppw <= 0) ppw = N / 2 >= 16384 ? 4 : N / 2 <= 1024 ? 1 : 2;
  const bool ppw_ok = ppw == 1 || ppw == 2 || ppw == 4;
  return {ppw_ok ? ppw : 0, bucket_of(GemvQ8CplPair{}, (K / kGemvQ8KMult + 31) / 32), (N / 2 + ppw - 1) / ppw};
}

// Automatic split-K of the skinny kernels: workgroups ~ 192 when the column tiles alone (16 wide
// for skinny_gemm, 32 for skinny_qkv_rope) are too few; every split keeps >= 4 k-steps of 32.
inline int skinny_auto_split(int ntiles, int steps) {
  return ntiles >= 128 ? 1 : std::max(1, std::min({(192 + ntiles - 1) / ntiles, steps / 4, 16}));
}
inline int skinny_gemm_auto_split(int N, int K) { return skinny_auto_split((N + 15) / 16, K / 32); }
// The fused QKV + RoPE kernel's split and the fp32 workspace it then needs: ONE rule, used by the
// launcher and exported (skinny_qkv_rope_plan) for the Python-side admission check (ops/gemm.py
// skinny_qkv_rope_ok), which must refuse a shape before a graph capture rather than let the
// launcher's workspace check throw inside it.
inline int qkv_rope_auto_split(int N, int K) { return skinny_auto_split(N / 32, K / 32); }
inline int64_t qkv_rope_ws_floats(int M, int N, int splitk) {
  return splitk > 1 ? (int64_t)splitk * (N / 32) * row_blocks(M) * 512 : 0;
}

struct GridPlan {
  int v;     // decode_gemm: row blocks per workgroup (1 / 4); decode_ln_gemm: K split (1 / 2)
  int tw;    // output columns per workgroup
  int grid;
};

// 4 row blocks per workgroup once there are more than two and the columns alone give >= 256
// workgroups (weights read once); otherwise one row block per workgroup (more workgroups)
inline GridPlan plan_decode_gemm(int M, int N) {
  const int rb = (M > 32 && N / 16 >= 256) ? 4 : 1;
  return {rb, 16, ((M + 16 * rb - 1) / (16 * rb)) * (N / 16)};
}

// K halves (KS = 2) by default: GPT-2 decode B = 16 / 32 / 64 0.567 / 0.584 / 0.636 -> 0.532 /
// 0.550 / 0.620 ms/step; quarters (KS = 4) lost: 0.55 / 0.74 / 0.96 — every workgroup repeats the
// LayerNorm of its 16 rows (profiles/decode_r5.md). ks_env 1 (PENROZ_DECODE_LN_KSPLIT=1): 64-column tiles.
inline GridPlan plan_decode_ln_gemm(int M, int N, int K, int ks_env) {
  const int ks = ks_env == 2 && (K / 32) % 2 == 0 ? 2 : 1;
  const int tw = 64 / ks;
  return {ks, tw, ((M + 15) / 16) * ((N + tw - 1) / tw)};
}

// ---- sampler launch plan (sampling.hip) ----
constexpr int kRT = 512;  // threads of the register kernel: 256 VGPRs each, room for a 104-logit slice
constexpr int kPartN = 4096, kPartK = 64, kPartMaxP = 64;  // two-stage: logits per part, largest top_k, most parts
using SampleSlices = IntList<1, 2, 3, 4, 6, 8, 10, 13, 16>;  // register kernel: 16-B chunks per thread (buckets)
enum class Elem { BF16, F32, F16 };
enum class SamplePath { TwoStage, Register, Stream };
struct SamplePlan {
  SamplePath path;
  int slice;          // Register: chunks per thread (else 0)
  int parts, part_k;  // TwoStage: parts per row, the top_k handed to its kernels (0: greedy) (else 0)
};

// Slices the register kernel is built for. With a nucleus filter bf16 stops at 10: the 13- and 16-chunk
// slices already sit at 256 VGPRs and the nucleus code does not fit beside them without more scratch,
// so rows above 40 960 logits take the streaming kernel.
constexpr bool sample_reg_fits(Elem e, int slice, bool nuc) {
  return slice >= 1 && (e == Elem::BF16 ? slice <= (nuc ? 10 : 16) : e == Elem::F32 && slice <= 8);
}

// temp: temperature != 0; nuc: a top-p / min-p filter is in effect; min_rows: PENROZ_SAMPLE_TWO_STAGE_MIN_ROWS
// (default 1). The two-stage pair takes V % 8 == 0 rows of up to 256 Ki logits, greedy or top_k <= 64, that
// are too wide for registers, and any number of rows from min_rows on: P x B part workgroups spread a row
// over P CUs where one workgroup per row leaves most of the chip idle (a batch-64 decode step, and a
// batch-1 step whose single-workgroup register sampler took ~38 µs of a ~600 µs GPT-2 token). The register
// kernel takes the other V % 8 == 0 rows that fit, the streaming kernel the rest (odd V, fp16, wide rows).
inline SamplePlan plan_sample(Elem e, int B, int V, bool temp, int top_k, bool nuc, int min_rows) {
  const bool vec = V >= 8 && V % 8 == 0 && e != Elem::F16;
  const int slice = bucket_of(SampleSlices{}, (V / 8 + kRT - 1) / kRT);  // 0: wider than every slice
  const bool fits = sample_reg_fits(e, slice, nuc);
  if (vec && (!fits || B >= min_rows) && V <= kPartMaxP * kPartN && (!temp || (top_k > 0 && top_k <= kPartK)))
    return {SamplePath::TwoStage, 0, (V + kPartN - 1) / kPartN, temp ? top_k : 0};
  if (vec && fits) return {SamplePath::Register, slice, 0, 0};
  return {SamplePath::Stream, 0, 0, 0};
}

// ---- token log-probabilities launch plan (token_logprobs.hip) ----
constexpr int kLogprobPartN = 4096, kLogprobMaxN = 20, kLogprobMaxParts = 256;  // logits per part, largest n, most parts
struct LogprobPlan {
  int parts;          // part workgroups per row (0: V is outside [1, 1 Mi])
  int64_t ws_floats;  // workspace per row: m [P], s [P] and the parts' candidates, 64-bit keys [P, kLogprobMaxN]
};

// One merge workgroup has a thread per part, so a row has at most 256 parts: V <= 1 Mi.
inline LogprobPlan plan_logprobs(int64_t V) {
  if (V < 1 || V > (int64_t)kLogprobMaxParts * kLogprobPartN) return {0, 0};
  const int parts = (int)((V + kLogprobPartN - 1) / kLogprobPartN);
  return {parts, (int64_t)parts * (2 + 2 * kLogprobMaxN)};
}

// ---- logit bias launch plan (logit_bias.hip) ----
constexpr int kBiasThreads = 256, kBiasMaxEntries = 1024, kBiasSpan = 2048;  // workgroup, most entries, tokens per mask part
struct LogitBiasPlan {
  int per_row;         // workgroups per row: the entries' one, and the mask parts (0: refused)
  int64_t grid;        // B x per_row (0: refused)
  int64_t mask_words;  // 32-bit words of the allowed mask: ceil(V / 32)
};

// Entries alone: one workgroup per row. With the allowed mask: ceil(V / kBiasSpan) more per row, each
// storing into its own span. Refused (all zero): B < 1, V outside [1, 2^31), or a grid of 2^31 or more.
inline LogitBiasPlan plan_logit_bias(int64_t B, int64_t V, bool mask) {
  if (B < 1 || V < 1 || V >= (int64_t(1) << 31)) return {0, 0, 0};
  const int64_t per_row = 1 + (mask ? (V + kBiasSpan - 1) / kBiasSpan : 0);
  if (B > ((int64_t(1) << 31) - 1) / per_row) return {0, 0, 0};
  return {(int)per_row, B * per_row, (V + 31) / 32};
}

// The launch's index arithmetic, shared by the kernel and the host test (constexpr: host and device).
// Workgroup wg serves row wg / per_row; its part wg % per_row is 0 for the entries, p >= 1 for the mask
// span p - 1. Thread tid of a mask part covers, in round k, the token below: consecutive lanes take
// consecutive tokens. Token v's bit is bit v % 32 of word v / 32.
constexpr int kBiasMaskRounds = kBiasSpan / kBiasThreads;
constexpr int64_t bias_row_of(int64_t wg, int per_row) { return wg / per_row; }
constexpr int bias_part_of(int64_t wg, int per_row) { return (int)(wg % per_row); }
constexpr int64_t bias_mask_token(int part, int tid, int k) {
  return (int64_t)(part - 1) * kBiasSpan + (int64_t)k * kBiasThreads + tid;
}
constexpr int64_t bias_mask_word(int64_t v) { return v >> 5; }
constexpr bool bias_allowed(unsigned word, int64_t v) { return (word >> (v & 31)) & 1u; }

// ---- decode attention launch plan (decode_attn.hip) ----
constexpr int kMaxMergeSplits = 16, kMergeMaxKeys = 8192;  // in-launch merge: most splits, longest context
// What is built: decode_kernel<D, GC> with an exact group size GC only for head_dim 64 / 128 / 256 (GC 0: any
// size <= 16); decode_small_kernel<D, G, ROPE> for G·D <= 4096 staged query values, RoPE up to head_dim 256
constexpr bool decode_has(int D, int gc) { return gc == 0 || (D != 32 && D != 512); }
constexpr bool decode_small_has(int64_t D, int64_t G, bool rope) {
  return (D == 64 || D == 128 || D == 256 || D == 512) && (G == 1 || G == 2 || G == 4 || G == 8 || G == 16) &&
         G * D <= 4096 && !(rope && D > 256);
}

struct DecodeAttnEnv {
  int small_items = 64;    // PENROZ_DECODE_SMALL_ITEMS: the largest B·Hkv the small kernel takes (0 disables)
  bool small_any = false;  // PENROZ_DECODE_SMALL_ANY=1 (A/B switch): also MHA head_dim 64 — GPT-2
  int split_keys = 0;      // PENROZ_DECODE_SPLIT_KEYS >= 64: keys per split, and the small kernel's longest context
};
struct DecodeAttnPlan {
  bool small;      // decode_small_kernel: one workgroup per (batch, KV head), no splits
  int splits;      // workgroups per (batch, KV head, query row) along the keys
  int split_keys;  // keys per split at least
  bool merge;      // the last split workgroup to arrive merges the partials (arrival counters)
};

// The small kernel takes one query row over up to 1024 keys (GQA batch 1: Gemma-3 1B 1.57 -> 1.26 ms/token
// at a 1024-slot cache, profiles/decode_r5.md); GQA or wide heads only: at G = 1, D = 64 (GPT-2 batch 1) the
// general kernel is ~1 µs faster per layer. It runs ONE workgroup per item over the whole cache, so longer
// contexts keep the key-split grid.
// S: the keys the launch is sized for (a graph captures the cache capacity; the kernel stops at the
// device-side length); bf16_plain: bf16 q over an unquantised bf16 cache; counters: element count of the
// zeroed arrival counters (0: none). Enough splits for >= 512 workgroups. With a counter per item the
// merge costs no second launch and contexts beyond 256 keys are split; without, a split costs the
// combine launch (~4.6 µs in a replayed step) and only contexts beyond 1024 keys are. GPT-2 B = 1 at
// 1024 keys: 0.489 ms/token unsplit vs 0.418 split four ways (profiles/decode_longctx_r6.log). Beyond
// 8192 keys the combine launch wins again: every merging item costs its split workgroups a device-scope
// release (Gemma-3 1B batch 1 at 16k keys, 16 splits either way: 10.89-10.91 ms/token vs 10.54-10.56).
inline DecodeAttnPlan plan_decode_attn(int64_t B, int64_t Tq, int64_t H, int64_t Hkv, int64_t D, int64_t S, bool bf16_plain,
                                       int64_t counters, const DecodeAttnEnv& env) {
  const int64_t items = B * Hkv * Tq, G = Hkv > 0 && H % Hkv == 0 ? H / Hkv : 0;
  if (bf16_plain && Tq == 1 && B * Hkv <= env.small_items && S <= (env.split_keys ? env.split_keys : 1024) &&
      (G >= 2 || D >= 128 || env.small_any) && decode_small_has(D, G, false))
    return {true, 1, 0, false};
  const bool merge = items >= 1 && counters >= items && S <= kMergeMaxKeys;
  const int keys = env.split_keys ? env.split_keys : merge ? 256 : 1024;
  int64_t splits = items >= 1 ? std::min((512 + items - 1) / items, (S + keys - 1) / keys) : 1;
  if (merge) splits = std::min<int64_t>(splits, kMaxMergeSplits);
  return {false, (int)std::max<int64_t>(1, splits), keys, merge};
}

}  // namespace penroz

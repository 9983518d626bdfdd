// Host-side unit test of the launch planners in csrc/kernels/host_plan.h, built and run by
// tests/test_host_sanitizers.py with -fsanitize=address,undefined (any report aborts the run).
#include "host_plan.h"

#include <cstdio>
#include <cstdlib>

using penroz::plan_wgrad_splits;

static int fails = 0;
#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      ++fails;                                                      \
    }                                                               \
  } while (0)

using namespace penroz;

template <class L>
static bool in_list(L list, int v) {
  return dispatch_exact([](auto) {}, list, v);
}

// dispatch.h: exact match hits each listed value (once, with that value) and nothing else; the
// bucket form picks the first V >= v
static void test_dispatch() {
  using L = IntList<1, 2, 3, 4, 5, 7, 12, 16, 25, 32>;
  for (int v = -2; v <= 40; ++v) {
    int calls = 0, got = -1;
    const bool hit = dispatch_exact([&](auto c) { ++calls, got = decltype(c)::value; }, L{}, v);
    const bool listed = (v >= 1 && v <= 5) || v == 7 || v == 12 || v == 16 || v == 25 || v == 32;
    EXPECT(hit == listed && calls == (listed ? 1 : 0) && (!listed || got == v));
    calls = 0, got = -1;
    const bool bhit = dispatch_bucket([&](auto c) { ++calls, got = decltype(c)::value; }, L{}, v);
    EXPECT(bhit == (v <= 32) && calls == (bhit ? 1 : 0));
    if (bhit) EXPECT(got >= v && in_list(L{}, got));
    for (int u = v; bhit && u < got; ++u) EXPECT(!in_list(L{}, u));  // nothing listed in [v, got)
    EXPECT(bucket_of(L{}, v) == (bhit ? got : 0));
  }
  // several (list, value) pairs: one call with all constants, false when any value is unlisted
  for (int m = 0; m <= 5; ++m)
    for (int r = 0; r <= 5; ++r) {
      int calls = 0, gm = 0, gr = 0;
      const bool hit = dispatch_exact([&](auto a, auto b) { ++calls, gm = decltype(a)::value, gr = decltype(b)::value; },
                                      GemvRows{}, m, Pow2To4{}, r);
      const bool want = m >= 1 && m <= 4 && (r == 1 || r == 2 || r == 4);
      EXPECT(hit == want && calls == (want ? 1 : 0) && (!want || (gm == m && gr == r)));
    }
  EXPECT(row_blocks(1) == 1 && row_blocks(16) == 1 && row_blocks(17) == 2 && row_blocks(32) == 2 &&
         row_blocks(33) == 4 && row_blocks(64) == 4);
}

// Every decode_gemv / decode_gemv_pair plan names an instantiated kernel whose lanes cover K and
// whose grid covers N
static void test_gemv_plan_properties() {
  const int Ns[] = {16, 33, 768, 2304, 16383, 16384, 50304, 262144};
  for (int M = 1; M <= kGemvMaxRows; ++M)
    for (int K = 8; K <= kGemvMaxK; K += 8)
      for (int N : Ns)
        for (int ln = 0; ln < 2; ++ln)
          for (int rpw : {0, 2, 4, 8})
            for (int env = 0; env < 4; ++env) {  // bit 0: PENROZ_DECODE_GEMV_WAVE_ROW=0, bit 1: ..._RPW=4
              const GemvPlan p = plan_decode_gemv(M, N, K, ln != 0, rpw, env & 2 ? 4 : 0, !(env & 1));
              EXPECT(p.m == M && in_list(Pow2To4{}, p.rp));
              EXPECT((p.form == GemvForm::LN) == (ln != 0));
              if (ln && K > kLnMaxK) {  // LN mode is never planned above its limit
                EXPECT(p.cpl == 0);
                continue;
              }
              const bool wr = p.form == GemvForm::WaveRow;
              EXPECT(wr ? in_list(GemvCplWave{}, p.cpl) : ln ? in_list(GemvCplLn{}, p.cpl) : in_list(GemvCplHalf{}, p.cpl));
              EXPECT(p.cpl * (wr ? 64 : 32) * 8 >= K);
              EXPECT(!wr || (p.rp == 1 && rpw == 0 && N < 16384 && !(env & 1)));
              EXPECT((long long)p.grid * p.rows_per_wg() >= N && (long long)(p.grid - 1) * p.rows_per_wg() < N);
              if (rpw) EXPECT(!wr && p.rp == rpw / 2);
            }
  EXPECT(plan_decode_gemv(1, 768, 768, false, 3, 0, true).rp == 0);   // bad rows_per_wave
  EXPECT(plan_decode_gemv(1, 768, 768, true, 0, 16, true).rp == 0);   // bad PENROZ_DECODE_GEMV_RPW
  for (int K = 8; K <= kGemvMaxK; K += 8)
    for (int N : {2, 66, 256, 2048, 2050, 13824, 32768, 65536})
      for (int ppw : {0, 1, 2, 4}) {
        const GemvPairPlan p = plan_decode_gemv_pair(N, K, ppw);
        EXPECT(in_list(Pow2To4{}, p.ppw) && (!ppw || p.ppw == ppw));
        EXPECT((long long)p.grid * p.ppw >= N / 2 && (long long)(p.grid - 1) * p.ppw < N / 2);
        if (K > kGemvPairMaxK) EXPECT(p.cpl == 0);
        else EXPECT(in_list(GemvCplPair{}, p.cpl) && p.cpl * 32 * 8 >= K);
      }
  EXPECT(plan_decode_gemv_pair(256, 64, 3).ppw == 0);
}

// Values worked out by hand from the launch rules (environment switches unset)
static void test_decode_plan_goldens() {
  struct G { int M, K, N, rpw; GemvForm form; int rp, cpl, grid; };
  const G gemv[] = {{1, 768, 768, 0, GemvForm::WaveRow, 1, 2, 768},     {4, 768, 50304, 0, GemvForm::HalfWave, 4, 3, 6288},
                    {2, 6912, 1152, 0, GemvForm::WaveRow, 1, 16, 1152}, {1, 8192, 16, 0, GemvForm::WaveRow, 1, 16, 16},
                    {3, 40, 33, 0, GemvForm::WaveRow, 1, 2, 33},        {1, 3072, 768, 4, GemvForm::HalfWave, 2, 12, 192},
                    {1, 768, 2304, 0, GemvForm::LN, 1, 3, 1152},        {4, 1024, 75, 0, GemvForm::LN, 1, 4, 38},
                    {3, 96, 50, 0, GemvForm::LN, 1, 3, 25}};
  for (const G& g : gemv) {
    const GemvPlan p = plan_decode_gemv(g.M, g.N, g.K, g.form == GemvForm::LN, g.rpw, 0, true);
    EXPECT(p.form == g.form && p.m == g.M && p.rp == g.rp && p.cpl == g.cpl && p.grid == g.grid);
  }
  const int pair[][5] = {{1152, 13824, 2, 5, 3456}, {1792, 66, 1, 7, 33}, {64, 256, 1, 3, 128}};  // K, N, ppw, CPL, grid
  for (auto& g : pair) {
    const GemvPairPlan p = plan_decode_gemv_pair(g[1], g[0], 0);
    EXPECT(p.ppw == g[2] && p.cpl == g[3] && p.grid == g[4]);
  }
  EXPECT(skinny_gemm_auto_split(768, 768) == 4 && skinny_gemm_auto_split(2304, 768) == 1);
  EXPECT(skinny_gemm_auto_split(768, 3072) == 4 && skinny_gemm_auto_split(40, 96) == 1);
  EXPECT(qkv_rope_auto_split(512, 2048) == 12 && qkv_rope_ws_floats(64, 512, 12) == 12 * 16 * 4 * 512);
  EXPECT(qkv_rope_auto_split(4096, 4096) == 1 && qkv_rope_ws_floats(64, 4096, 1) == 0);
  EXPECT(plan_decode_gemm(64, 1536).v == 1 && plan_decode_gemm(64, 4096).v == 4);
  EXPECT(plan_decode_gemm(40, 13824).v == 4 && plan_decode_gemm(17, 1152).v == 1);
  EXPECT(plan_decode_gemm(64, 4096).grid == 256 && plan_decode_gemm(17, 1152).grid == 2 * 72);
  const GridPlan a = plan_decode_ln_gemm(64, 2304, 768, 2), b = plan_decode_ln_gemm(9, 1040, 96, 2);
  EXPECT(a.v == 2 && a.tw == 32 && a.grid == 288);
  EXPECT(b.v == 1 && b.tw == 64 && b.grid == 17);
  EXPECT(plan_decode_ln_gemm(64, 2304, 768, 1).v == 1);  // PENROZ_DECODE_LN_KSPLIT=1
}

// Every sampler plan names a kernel that is built and covers the row
static void test_sample_plan_properties() {
  const int Vs[] = {0, 1, 7, 8, 64, 1024, 4096, 4104, 8192, 24576, 32768, 32776, 40960, 40968, 50257, 50304,
                    65536, 65544, 96000, 262144, 262152, 1 << 22};
  for (Elem e : {Elem::BF16, Elem::F32, Elem::F16})
    for (int V : Vs)
      for (int B : {0, 1, 2, 16, 64})
        for (int temp = 0; temp < 2; ++temp)
          for (int k : {0, 1, 50, 64, 65, 1000})
            for (int nuc = 0; nuc <= temp; ++nuc)  // a filter is in effect only with a temperature
              for (int min_rows : {0, 1, 2, 16, 1 << 30}) {
                const SamplePlan p = plan_sample(e, B, V, temp != 0, k, nuc != 0, min_rows);
                if (e == Elem::F16 || V % 8 != 0) EXPECT(p.path == SamplePath::Stream);
                if (p.path == SamplePath::Register) {
                  EXPECT(in_list(SampleSlices{}, p.slice) && sample_reg_fits(e, p.slice, nuc != 0));
                  EXPECT((long long)p.slice * kRT * 8 >= V && p.parts == 0 && p.part_k == 0);
                  EXPECT(B < min_rows || (temp && (k == 0 || k > kPartK)));  // else the two-stage pair has it
                } else if (p.path == SamplePath::TwoStage) {
                  EXPECT(p.parts >= 1 && p.parts <= kPartMaxP && (long long)p.parts * kPartN >= V && p.slice == 0);
                  EXPECT(temp ? (p.part_k == k && k >= 1 && k <= kPartK) : p.part_k == 0);
                } else {
                  EXPECT(p.slice == 0 && p.parts == 0 && p.part_k == 0);
                }
              }
  // the fit rule: bf16 up to 16 chunks, 10 with a filter; fp32 up to 8; fp16 never; nothing outside the list
  for (int c = -1; c <= 20; ++c) {
    EXPECT(sample_reg_fits(Elem::BF16, c, false) == (c >= 1 && c <= 16) && sample_reg_fits(Elem::BF16, c, true) == (c >= 1 && c <= 10));
    EXPECT(sample_reg_fits(Elem::F32, c, false) == (c >= 1 && c <= 8) && sample_reg_fits(Elem::F32, c, true) == (c >= 1 && c <= 8));
    EXPECT(!sample_reg_fits(Elem::F16, c, false) && !sample_reg_fits(Elem::F16, c, true));
  }
  // by hand, default switch (1 row): GPT-2's padded vocabulary
  const SamplePlan a = plan_sample(Elem::BF16, 1, 50304, true, 50, false, 1), b = plan_sample(Elem::BF16, 1, 50304, true, 0, false, 1);
  EXPECT(a.path == SamplePath::TwoStage && a.parts == 13 && a.part_k == 50 && b.path == SamplePath::Register && b.slice == 13);
  EXPECT(plan_sample(Elem::BF16, 1, 50304, true, 0, true, 1).path == SamplePath::Stream);
  EXPECT(plan_sample(Elem::BF16, 1, 50304, true, 50, false, 2).slice == 13);
}

// Every decode attention plan is launchable: at least one split, a merge only within its limits,
// the small kernel only where it is built
static void test_decode_attn_plan_properties() {
  const DecodeAttnEnv envs[] = {{}, {0, false, 0}, {1024, true, 0}, {64, false, 64}, {64, false, 4096}};
  for (const DecodeAttnEnv& env : envs)
    for (int B : {0, 1, 3, 64, 65, 512})
      for (int Tq : {0, 1, 2, 17})
        for (int Hkv : {0, 1, 2, 3, 12})
          for (int G : {1, 2, 3, 4, 8, 16, 32})
            for (int D : {0, 32, 64, 96, 128, 256, 512})
              for (long long S : {0LL, 1LL, 256LL, 257LL, 1024LL, 1025LL, 8192LL, 8193LL, 16384LL, 1LL << 20})
                for (long long counters : {0LL, 1LL, 4096LL, 1LL << 13})
                  for (int plain = 0; plain < 2; ++plain) {
                    const int H = Hkv ? G * Hkv : G;  // Hkv = 0: degenerate, must not divide
                    const DecodeAttnPlan p = plan_decode_attn(B, Tq, H, Hkv, D, S, plain != 0, counters, env);
                    EXPECT(p.splits >= 1);
                    if (p.merge) EXPECT(!p.small && p.splits <= 16 && S <= 8192 && counters >= (long long)B * Hkv * Tq);
                    if (!p.small) EXPECT(p.split_keys >= 64 && (long long)(p.splits - 1) * p.split_keys < (S > 0 ? S : 1));
                    if (p.small) {
                      EXPECT(plain && Tq == 1 && Hkv >= 1 && p.splits == 1 && !p.merge);
                      EXPECT((G == 1 || G == 2 || G == 4 || G == 8 || G == 16) && (D == 64 || D == 128 || D == 256 || D == 512));
                      EXPECT(G * D <= 4096 && B * Hkv <= env.small_items && S <= (env.split_keys ? env.split_keys : 1024));
                      EXPECT(decode_small_has(D, G, false));
                    }
                  }
  EXPECT(!plan_decode_attn(1, 1, 7, 2, 64, 100, true, 0, {}).small);  // H % Hkv != 0
  EXPECT(!decode_small_has(512, 16, false) && decode_small_has(512, 8, false) && !decode_small_has(512, 8, true));
  EXPECT(decode_small_has(256, 16, true) && !decode_small_has(32, 1, false) && !decode_small_has(64, 3, false));
  EXPECT(decode_has(32, 0) && decode_has(512, 0) && !decode_has(32, 1) && !decode_has(512, 8) && decode_has(64, 4));
  // by hand, default switches: GPT-2 (12 heads of 64) and a Gemma-3 1B layer (4 query heads on 1 KV head of 256)
  struct G { int B, H, Hkv, D; long long S, counters; bool small; int splits, keys; bool merge; };
  const G gold[] = {{1, 12, 12, 64, 1024, 4096, false, 4, 256, true}, {1, 12, 12, 64, 1024, 0, false, 1, 1024, false},
                    {64, 12, 12, 64, 1024, 4096, false, 1, 256, true}, {1, 4, 1, 256, 1024, 4096, true, 1, 0, false},
                    {1, 4, 1, 256, 1025, 0, false, 2, 1024, false}, {65, 4, 1, 256, 1024, 0, false, 1, 1024, false},
                    {1, 16, 1, 512, 512, 0, false, 1, 1024, false}, {1, 8, 1, 512, 512, 0, true, 1, 0, false},
                    {1, 4, 1, 256, 16384, 8192, false, 16, 1024, false}, {1, 4, 1, 256, 8192, 8192, false, 16, 256, true}};
  for (const G& g : gold) {
    const DecodeAttnPlan p = plan_decode_attn(g.B, 1, g.H, g.Hkv, g.D, g.S, true, g.counters, {});
    EXPECT(p.small == g.small && p.splits == g.splits && p.split_keys == g.keys && p.merge == g.merge);
  }
}

int main() {
  // GPT-2 124M / XL weight-gradient shapes (K = tokens per step) and edge cases
  const int shapes[][3] = {{2304, 768, 65536}, {768, 768, 65536}, {3072, 768, 65536}, {768, 3072, 65536},
                           {50304, 768, 65536}, {50257, 768, 65536}, {4800, 1600, 65536}, {6400, 1600, 16384},
                           {8, 8, 1}, {200, 136, 1000}, {1, 1, 511}, {65536, 65536, 2147483647 / 2}};
  for (auto& s : shapes) {
    for (int tile : {128, 256}) {
      for (int bk : {32, 64}) {
        const auto p = plan_wgrad_splits(s[0], s[1], s[2], tile, 256, bk);
        EXPECT(p.splits >= 1 && p.splits <= 64);
        EXPECT(p.klen > 0 && p.klen % bk == 0);
        EXPECT((long long)p.klen * p.splits >= s[2]);              // covers K
        EXPECT((long long)p.klen * (p.splits - 1) < s[2]);         // no empty split
      }
    }
  }
  // split-tail plans: every tile covered once, the tail's splits cover K without an empty one
  const int tshapes[][3] = {{50304, 768, 65536}, {50257, 768, 65536}, {13824, 1152, 8192}, {262144, 1152, 8192},
                            {1152, 6912, 8192}, {6400, 1600, 16384}, {8, 8, 1}, {1 << 20, 768, 4096}};
  for (auto& s : tshapes) {
    const auto p = penroz::plan_wgrad(s[0], s[1], s[2], 256, 256, 32);
    const long long nt = (long long)((s[0] + 255) / 256) * ((s[1] + 255) / 256);
    EXPECT(p.main_tiles >= 0 && p.main_tiles <= nt);
    EXPECT(p.main_splits >= 1 && p.main_klen > 0 && p.main_klen % 32 == 0);
    EXPECT((long long)p.main_klen * p.main_splits >= s[2]);
    if (p.tail_splits > 0) {
      EXPECT(p.main_splits == 1 && p.main_tiles < nt && p.tail_splits >= 2);
      EXPECT(p.tail_klen % 32 == 0 && (long long)p.tail_klen * p.tail_splits >= s[2]);
      EXPECT((long long)p.tail_klen * (p.tail_splits - 1) < s[2]);
      EXPECT((nt - p.main_tiles) * p.tail_splits <= 256);  // the tail fits one round
    } else {
      EXPECT(p.main_tiles == nt);
    }
  }
  {  // GPT-2 lm_head: 591 tiles -> 512 direct + 79 tiles split 3 ways
    const auto p = penroz::plan_wgrad(50304, 768, 65536, 256, 256, 32);
    EXPECT(p.main_tiles == 512 && p.tail_splits == 3);
  }
  // degenerate inputs never divide by zero or overflow
  for (int bad : {0, -1}) {
    const auto p = plan_wgrad_splits(bad, 768, 1024, 256, 256, 64);
    EXPECT(p.splits == 1);
    const auto q = plan_wgrad_splits(768, 768, bad, 256, 0, 64);
    EXPECT(q.splits == 1);
    const auto w = penroz::plan_wgrad(768, bad, 1024, 256, 0, 32);
    EXPECT(w.tail_splits == 0 && w.main_splits >= 1);
  }
  for (int g : {0, 1, 2, 1024, 1 << 20, 2147483647}) {
    const int s = penroz::reduce_slices(g);
    EXPECT(s >= 1 && (long long)s * s >= g && (long long)(s - 1) * (s - 1) < (g > 1 ? g : 2));
  }
  test_dispatch();
  test_gemv_plan_properties();
  test_decode_plan_goldens();
  test_sample_plan_properties();
  test_decode_attn_plan_properties();
  std::printf("host_plan_test: %s (%d failures)\n", fails ? "FAILED" : "ok", fails);
  return fails ? 1 : 0;
}

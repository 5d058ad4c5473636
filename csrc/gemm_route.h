// GEMM dispatch (k_gemm.hip): which kernel instantiation, grid and LDS size a forward / data-gradient GEMM
// (gemm_route) or a weight gradient (wgrad_route) runs with.  Pure host functions of the problem, the switches
// and the CU count: no HIP, no side effects; the launchers in k_gemm.hip launch what they return and nothing
// else.  Checked on the CPU by selftest_gemm_route.cpp.
#pragma once
#include <algorithm>

#include "k256_split.h"

// Tile, block and dynamic-LDS sizes of the kernel families (k_gemm.hip static_asserts them against the kernels')
namespace rk {
constexpr int BM = 128, BN = 128, BK = 64, NT = 256;  // 128x128 kernels
constexpr int BM3 = 256, BG = 256, NT3 = 512;         // 256x128 ring, 256x256 big64 (and K = 256): 8 waves
constexpr int LDS_EPI = BM * 132 * 4;                 // fp32 epilogue staging tile >= 2 stages x (A+B) = 64 KiB
constexpr int LDS_REG = 2 * 2 * BM * BK * 2;
constexpr int RING_LDS = 3 * (BM3 + BN) * BK * 2;
constexpr int B64_LDS = 256 * 528;
constexpr int K2_LDS = 3 * K256_ROWS * 256 * 2 + K256_ROWS * 528 + 3 * K256_ROWS * 32;
constexpr int WB64_LDS = 128 * 1088;  // the LDS-staged slab epilogue tile (> 2 stages of 64 KiB)
constexpr int WB64_LDS_MAX = 160 * 1024;
constexpr int W128_LDS = 2 * 2 * 64 * 256;
constexpr int ACT_RELU = 1, ACT_LRELU = 2;
constexpr int EPI_GEN = 0, EPI_BNH = 1, EPI_MASK = 2;
}  // namespace rk

// Every switch the dispatch reads (ssamd_gemm_set_* / ssamd_wgrad_set_*), with the defaults.
struct GemmKnobs {
  int variant = -1;  // -1 auto, 0: register staging, 1: LDS-DMA 128x128, 4: 256x256 big64, other >= 2: 256x128 ring
  bool force_lds_epilogue = false;
  // s_setprio 1 for waves 4-7 of the 8-wave big64 blocks (MI355X_MICROARCH "static priority for the
  // younger half"), measured per kernel (tools/exp_prio.py): weight gradients on packed rows -2..-4 %,
  // others neutral -> on for wgrad; forward mixed (k9 N = 1024 fwd -4 %, k9 N = 256 dgrad +8 %) -> on for
  // N >= 1024 convs only
  int prio = -1;      // forward -1: auto (on for wide k > 1 convs only)
  int ngrp = 1;       // 256x256 tile order: N-tile groups (tile_of); experiment knob
  int splitk = -1;    // -1 auto, 0 off, S > 1 forced slices (big64 split-K + reduce)
  int splitk_tiny = 3;  // min k-steps per slice for <= 8 tiles (0: the general rule only)
  int ring_maxk = 0, ring_maxn = 256;  // 0: the 256x128 ring only for <= 64 big tiles (A/B knob)
  int skinny = 1;     // skinny_gemm_kernel for M <= skinny_maxm rows (0: off, A/B)
  // 8-wave skinny blocks from this many k-steps (0: always 4 waves).  Batch 1: 4 waves 1.674 / 1.676 ms, 8 from 16
  // steps 1.625 / 1.624 / 1.605, from 8 steps 1.613 / 1.618; 16 waves from 32 or 64 steps no better (r6_b1_latency.txt)
  int skinny_w8 = 16;
  int skinny_maxm = 1024;  // measured at batch 1: 64 -> 2.19 ms, 128 -> 1.80, 1024 -> 1.76 (r6_b1_latency.txt)
  int skinny_any_cin = 1;  // the skinny kernel also for Cin % 32 != 0 (per-lane taps; 0: tile kernels, A/B)
  int num_cus_gemm = 256;  // split-K's wave of blocks (not the device's count)
  int buf = 1;  // big64 / ring (FASTK) LDS-DMA through buffer descriptors (0: flat global_load_lds)
  // big64 buffer-descriptor path: 1 = the staggered 8-phase main loop for K >= 512 (tools/exp_stg.py: +5 % on
  // the k9 convs and K = 1024, +2 % PostNet k5, -1..4 % at K = 256 where the prologue / epilogue dominate)
  int stg = 1;
  int mask_pre = 1;  // EPI_MASK for the ReLU-mask data gradient (0: the generic epilogue, A/B)
  int bnh_stg = 1;   // the BatchNorm-backward-head data gradient on the staggered main loop (0: A/B)
  // weight-stationary K = 256 kernel (conv_gemm_k256_kernel): -1 auto (the measured rule in gemm_route), 0 off,
  // 1 on wherever the shape qualifies regardless of M
  int k256 = -1;
  int k256_min_rows = 28672;  // N = 512 / 768: the measured crossover lies between 14336 and 28672 rows
  int k256_blocks = 0;        // > 0: grid budget instead of the device's CUs (tests: many chunks per block)
  int wgrad_variant = -1;  // -1 auto (256x256 BK=64 when it applies), 0: force the 128x128 kernels
  int wgrad_imm = -1;      // -1 auto, 0 / 1: force the big64 wgrad read schedule
  int wgrad_buf = 1;       // big64 wgrad LDS-DMA through buffer descriptors (0: flat global_load_lds)
  // big64 wgrad (buffer-descriptor path) ping-pong main loop: -1 auto = on packed rows (decoder k9 wgrad
  // 646 -> 519 us vs 718 before, tools/exp_wgrad_pp.py), off on plain rows (PostNet k5 -14 %)
  int wgrad_pp = -1;
  int wgrad_prio = 1;
  int wgrad_blocks = 0;  // > 0: fixed split-M target (blocks per launch) instead of the cost model
  // > 0: plan the split-M rounds for this many CUs instead of the device's (a weight gradient on the side
  // stream then leaves the other CUs to the data-gradient chain instead of holding every CU's LDS)
  // The budget applies to launches on ONE stream (the weight-gradient side stream): a main-stream weight
  // gradient (first step, --no-side-wgrad) keeps the whole-device plan, so the split-M count -- and with it
  // the fp32 reduction order -- of a main-stream launch does not depend on the side-stream setting.
  int wgrad_cus = 0;
};

// What conv_gemm_impl knows about one launch.
struct GemmProblem {
  int M = 0, N = 0, Cin = 0, ks = 1, pad = 0;  // M = B * L rows, K = ks * Cin
  int ldy = 0, act = 0, ksplit = 0;
  bool out_f32 = false;
  bool bias = false, aux = false, resid = false, lens = false, rinfo = false;  // operands present
  bool bnh = false, mask_in = false, mask_out = false, acc = false, y2 = false;
  int post_act = 0;
  bool scale_one = true, bn_stats = false, bn_part = false;
};

enum { GEMM_NONE, GEMM_SKINNY, GEMM_SPLITK, GEMM_K256, GEMM_BIG64, GEMM_RING, GEMM_GLDS, GEMM_REG, GEMM_LDS_EPI };

// Template flags of one instantiation; a family reads the fields its template has, the others stay 0.
struct GemmFlags {
  bool f32, fastk, packed, buf;  // OUT_F32, FASTK (Cin % 64 == 0), PACKED (rinfo), BUF (buffer-descriptor DMA)
  int epi;                       // big64: rk::EPI_*
  bool stg;                      // big64: staggered 8-phase main loop
  int waves;                     // skinny: 4 or 8
  bool aligned, mask, has_bias;  // skinny: Cin % 32 == 0; K = 256: MASK, HB
};
constexpr bool operator==(const GemmFlags& a, const GemmFlags& b) {
  return a.f32 == b.f32 && a.fastk == b.fastk && a.packed == b.packed && a.buf == b.buf && a.epi == b.epi &&
         a.stg == b.stg && a.waves == b.waves && a.aligned == b.aligned && a.mask == b.mask && a.has_bias == b.has_bias;
}

struct GemmRoute {
  int rc = 0;  // 0, or the error conv_gemm_impl returns (-2 bad Cin, -3 no kernel implements the epilogue)
  int kind = GEMM_NONE;
  GemmFlags fl{};
  int grid_x = 0, grid_y = 1, block = 0, lds = 0;
  int S = 0;           // SPLITK: k slices (grid_y)
  int nb = 0, ng = 0;  // K256: blocks per column group, column groups
  int ksplit = 0;      // ConvGeom::ksplit in effect
};

// The instantiations that exist, per family: {f32, fastk, packed, buf, epi, stg}.  BUF needs FASTK; the staggered
// loop and EPI_MASK need BUF; EPI_BNH and EPI_MASK are bf16-out, EPI_BNH never packed.
constexpr GemmFlags kBig64Flags[] = {
    {1, 1, 0, 0}, {1, 0, 0, 0}, {1, 1, 1, 0}, {1, 0, 1, 0}, {1, 1, 0, 1}, {1, 1, 1, 1},  // fp32 out (split-K partials)
    {0, 1, 0, 0}, {0, 0, 0, 0}, {0, 1, 1, 0}, {0, 0, 1, 0}, {0, 1, 0, 1}, {0, 1, 1, 1},
    {0, 1, 0, 1, rk::EPI_BNH}, {0, 1, 0, 1, rk::EPI_BNH, 1}, {0, 1, 0, 0, rk::EPI_BNH}, {0, 0, 0, 0, rk::EPI_BNH},
    {0, 1, 0, 1, rk::EPI_GEN, 1}, {0, 1, 1, 1, rk::EPI_GEN, 1}, {1, 1, 0, 1, rk::EPI_GEN, 1}, {1, 1, 1, 1, rk::EPI_GEN, 1},
    {0, 1, 0, 1, rk::EPI_MASK}, {0, 1, 1, 1, rk::EPI_MASK}, {0, 1, 0, 1, rk::EPI_MASK, 1}, {0, 1, 1, 1, rk::EPI_MASK, 1}};
constexpr GemmFlags kRingFlags[] = {{1, 1, 0, 0}, {0, 1, 0, 0}, {1, 0, 0, 0}, {0, 0, 0, 0}, {1, 1, 1, 0}, {0, 1, 1, 0},
                                    {1, 0, 1, 0}, {0, 0, 1, 0}, {1, 1, 0, 1}, {0, 1, 0, 1}, {1, 1, 1, 1}, {0, 1, 1, 1}};
constexpr GemmFlags kC128Flags[] = {{1}, {0}};  // GLDS, REG and LDS_EPI: {f32}
constexpr GemmFlags kSkinnyFlags[] = {{0, 0, 0, 0, 0, 0, 8, 1}, {0, 0, 0, 0, 0, 0, 4, 1},  // {waves, aligned}
                                      {0, 0, 0, 0, 0, 0, 8, 0}, {0, 0, 0, 0, 0, 0, 4, 0}};
constexpr GemmFlags kK256Flags[] = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 1},  // {mask, has_bias}
                                    {0, 0, 0, 0, 0, 0, 0, 0, 1, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 1, 1}};

// index of `want` in a family table, or -1: such an instantiation does not exist
template <class F, int N>
constexpr int flags_index(const F (&tab)[N], const F& want) {
  for (int i = 0; i < N; ++i)
    if (tab[i] == want) return i;
  return -1;
}

// every byte offset of the descriptors must stay below the out-of-range marker 0x80000000
inline bool big64_buf_ok(const GemmProblem& p, const GemmKnobs& k) {
  return k.buf != 0 && (long)(p.M + p.pad) * p.Cin * 2 < (1L << 31) && (long)p.N * (p.ks * p.Cin) * 2 + 512 < (1L << 31);
}

// The rules, in order of precedence: skinny, split-K, K = 256, then the epilogue constraints (BatchNorm head, ReLU
// bitmask, extended epilogue: -3 where no kernel implements the combination) over the tile kernels.
inline GemmRoute gemm_route(const GemmProblem& p, const GemmKnobs& k, int cus) {
  using namespace rk;
  GemmRoute r;
  if (p.Cin % 8 != 0) { r.rc = -2; return r; }
  if (p.M == 0 || p.N == 0) return r;
  const int M = p.M, N = p.N, Cin = p.Cin, K = p.ks * Cin, act = p.act, ldy = p.ldy;
  const auto fail = [] { GemmRoute e; e.rc = -3; return e; };
  const auto tiled = [&](int kind, int tm, int tn, int block, int lds) {
    r.kind = kind;
    r.grid_x = ((M + tm - 1) / tm) * ((N + tn - 1) / tn);
    r.block = block;
    r.lds = lds;
  };
  if (p.ksplit > 0 && p.ks == 3 && Cin % 64 == 0 && p.ksplit % 256 == 0 && p.ksplit < N) r.ksplit = p.ksplit;
  // register epilogue needs N % 4 == 0 and an 8-B aligned ldy; LDS-staged epilogue otherwise
  const bool reg = (N % 4 == 0) && (ldy % 4 == 0) && !k.force_lds_epilogue;
  const int tiles = ((M + BG - 1) / BG) * ((N + BG - 1) / BG);  // 256x256
  int variant = k.variant;
  // measured on MI355X (tools/bench_kernels.py): the 256x256 tile with a BK=64 double buffer wins for
  // every N >= 256 shape (+3..15 % over the 256x128 ring, +4..8 % over 256x256 with a BK=32 4-stage ring);
  // the 256x128 ring for narrower N when K-slabs are tap-aligned, LDS-DMA 128x128 otherwise
  if (variant < 0) variant = N >= 256 ? 4 : (Cin % BK == 0) ? 2 : 1;
  // Few 256x256 tiles (encoder / variance-predictor GEMMs at M = B*T ~ 5k-30k rows with N = 256): the
  // big tile leaves most of the 256 CUs idle; the 256x128 ring (or the 128x128 LDS-DMA kernel) doubles
  // (quadruples) the tile count.  Measured at M = 14k (tools/exp_small_m.py): -20..36 % time for every
  // N = 256 shape (k9 dgrad 219 -> 141 us), while N >= 768 keeps the 256x256 tile.
  if (k.variant < 0 && N >= 256 && N <= 256 && tiles <= 64) variant = (Cin % BK == 0) ? 2 : 1;
  // (A/B) the 256x128 ring also for short-K GEMMs with more tiles (K <= ring_maxk, N <= ring_maxn)
  if (k.variant < 0 && k.ring_maxk > 0 && N >= 256 && N <= k.ring_maxn && K <= k.ring_maxk && Cin % BK == 0)
    variant = 2;
  const bool xon = p.acc || p.y2 || p.post_act || !p.scale_one;  // EpiX's accumulate / scale / y2 / post activation
  const bool fastk = Cin % 64 == 0;
  const bool buf = fastk && big64_buf_ok(p, k);

  // Skinny M (<= skinny_maxm rows): 16 x 16 output tiles, k split over the block's waves (skinny_gemm_kernel);
  // Cin % 32 != 0 (still % 8): conv_pre / PostNet conv 0 over 80 mel channels, the GST's first im2col layer
  if (k.skinny && M <= k.skinny_maxm && (Cin % 32 == 0 || k.skinny_any_cin) && N % 16 == 0 && !p.bnh && !p.mask_out &&
      !p.mask_in && act >= 0 && (p.post_act == 0 || p.post_act == ACT_LRELU) && (!p.out_f32 || !xon)) {
    r.kind = GEMM_SKINNY;
    r.fl.waves = (k.skinny_w8 > 0 && K / 32 >= k.skinny_w8) ? 8 : 4;  // long K: 8 waves split it (shorter chains)
    r.fl.aligned = Cin % 32 == 0;
    r.grid_x = N / 16;
    r.grid_y = (M + 15) / 16;
    r.block = 64 * r.fl.waves;
    return r;
  }
  // Split-K for few 256x256 tiles with a long K (encoder-sized M, k = 9 data gradients, K = 9216):
  // S slices of the k range as extra blocks writing fp32 partials, one fixed-order reduce kernel
  // applies the epilogue.  Measured (tools/exp_splitk.py) on the tile-poor shapes only.
  {
    const int nk64 = (K + 63) / 64;
    // the reduce applies EpiX's accumulate / scale / y2 / post activation (bf16 output, as the big64 epilogue)
    const bool plain = !(p.mask_out || p.mask_in || p.bnh) &&
                       (!xon || (!p.out_f32 && (p.post_act == 0 || p.post_act == ACT_LRELU)));
    int S = 0;
    if (k.splitk > 0) S = k.splitk;
    else if (k.splitk < 0 && k.variant < 0 && tiles <= 128 && nk64 >= 16)
      // as many slices as keep the split grid within ONE wave of blocks (a second partial wave
      // costs more than it saves: M = 10800 / 43 tiles: S = 4 81 us, S = 6 111 us, unsplit 149 us)
      S = std::min(std::min(8, k.num_cus_gemm / tiles), nk64 / 6);
    // a handful of tiles at <= 1024 rows (batch-1 inference: one utterance's phonemes / frames / first vocoder
    // stages) is a serial chain of k-steps on a few CUs: shorter slices (>= splitk_tiny k-steps each), also
    // for the shorter K of the k = 3 convs
    if (k.splitk < 0 && k.variant < 0 && k.splitk_tiny > 0 && tiles <= 8 && M <= 1024 && nk64 >= 2 * k.splitk_tiny)
      S = std::max(S, std::min(8, nk64 / k.splitk_tiny));
    if (S > 1 && plain && reg && N >= 256 && (N % 8) == 0 && ldy == N && act >= 0 && (ldy % 8) == 0) {
      tiled(GEMM_SPLITK, BG, BG, NT3, B64_LDS);
      r.fl.f32 = true;  // fp32 partials; the reduce writes Y
      r.fl.fastk = fastk;
      r.fl.packed = p.rinfo;
      r.fl.buf = buf;
      r.grid_y = r.S = S;
      return r;
    }
  }
  // K = 256 Linear layers (QKV, attention fc and its data gradient, the w_2 data gradient with its ReLU
  // bitmask): the weight-stationary streaming kernel, one block per CU.  Only the epilogue forms the training
  // step uses at K = 256 (bias, mask_in, bf16 out, ldy == N); everything else stays on the tile kernels.
  // Rows: every byte offset of its descriptors (two chunks of read-ahead included) stays below 2^31.
  // Auto rule, measured against the kernel each shape ran on before (tools/bench_kernels.py --k256, 5 interleaved
  // rounds, routed only where every round of the new kernel beat every round of the old;
  // profiles/k256_stream.txt; us old -> new):
  //   N >= 1024 (ReLU-mask dgrad)  from 2048 rows: 100352 rows 147 -> 80, 14336 rows 22.4 -> 21.5, 2048 19.5 -> 12.3
  //   N = 512 / 768 (QKV)          from 28672 rows: 100352 rows 77 -> 55, 28672 26.6 -> 23; 8192 / 14336 rows LOSE
  //                                (13.8 -> 15.5, 15.8 -> 18.3: 3 groups x 85 blocks of ~3 chunks, prologue-bound)
  //   N = 256 (fc fwd / dgrad)     <= 64 tiles, where the 256x128 ring ran (14336 rows 14.6 -> 13.1, 2048 13.1 -> 10.9),
  //                                and from 1.5 waves of 256-row tiles (100352 rows 29.3 -> 27.7, 30.0 -> 28.6 in
  //                                a second session); up to one wave the balanced 256x256 tiles win (28672 rows
  //                                13.8 -> 16.0, 50176 15.3 -> 19.4), between 1 and 1.5 waves it is mixed (69632 rows
  //                                26.5 -> 23.5 every round, 81920 rows 27.7 -> 27.3 with one round behind)
  // Below 2048 rows nothing was measured (the skinny kernel takes <= 1024).
  const int k256_tiles = (M + BG - 1) / BG;
  const bool k256_auto = k.variant < 0 && M >= 2048 &&
                         (N >= 1024 || (N >= 512 && M >= k.k256_min_rows) ||
                          (N == 256 && (k256_tiles <= 64 || 2 * k256_tiles >= 3 * cus)));
  if (k.k256 != 0 && p.ks == 1 && Cin == 256 && N >= 256 && N % 256 == 0 && !p.out_f32 && !p.aux && !p.resid &&
      !p.lens && !p.rinfo && !p.bnh && p.ksplit == 0 && act == 0 && ldy == N && reg && !xon && !p.mask_out &&
      !p.bn_stats && !p.bn_part && ((long)M + 4 * K256_ROWS) * (N > 256 ? N : 256) * 2 < (1L << 31) &&
      (k.k256 > 0 || k256_auto)) {
    r.kind = GEMM_K256;
    r.fl.mask = p.mask_in;
    r.fl.has_bias = p.bias;
    r.ng = N / 256;
    r.nb = k256_blocks_per_group(k.k256_blocks > 0 ? k.k256_blocks : cus, r.ng, k256_chunks(M));
    r.grid_x = r.nb * r.ng;
    r.block = NT3;
    r.lds = K2_LDS;
    return r;
  }
  if (p.bnh) {  // BatchNorm-backward head (EpiX aliases: acc = bn_h, ln_w = stats, mean = partials): big64 only
    if (N < 256 || (N % 8) || ldy != N || p.out_f32 || !reg || act != 0 || p.post_act == 2 || p.aux || p.resid ||
        p.lens || !p.acc || !p.bn_stats || !p.bn_part || p.rinfo || p.y2 || p.mask_out || p.mask_in)
      return fail();
    variant = 4;
  } else {
    if (p.mask_out || p.mask_in) {  // the bitmask lives in the big64 LDS-staged epilogue only
      if (N < 256 || (N % 8) || ldy != N || p.out_f32 || !reg || act < 0) return fail();
      if (p.mask_out && act != ACT_RELU) return fail();
      variant = 4;
    }
    if (xon) {  // only the big64 (LDS-staged bf16 epilogue) and ring kernels implement EpiX
      if (p.out_f32 || !reg || (N % 8) || (ldy % 8) || act < 0) return fail();
      if (N >= 256) variant = 4;
      else if (variant != 2) return fail();
    }
  }
  if (reg && variant == 4 && N >= 256) {
    tiled(GEMM_BIG64, BG, BG, NT3, B64_LDS);
    const bool stg = buf && k.stg && K >= 512;
    r.fl.f32 = p.out_f32;
    r.fl.fastk = fastk;
    r.fl.buf = buf;
    if (p.bnh) {
      r.fl.epi = EPI_BNH;
      r.fl.stg = stg && k.bnh_stg;
    } else {
      r.fl.packed = p.rinfo;
      r.fl.stg = stg;
      // the ReLU-mask data gradient with nothing else in its epilogue: mask bytes prefetched (EPI_MASK)
      if (buf && k.mask_pre && p.mask_in && !p.mask_out && !p.aux && !p.resid && !p.lens && !xon && !p.out_f32 &&
          act >= 0 && ldy == N)
        r.fl.epi = EPI_MASK;
    }
  } else if (reg && variant >= 2) {
    tiled(GEMM_RING, BM3, BN, NT3, RING_LDS);
    r.fl.f32 = p.out_f32;
    r.fl.fastk = fastk;
    r.fl.packed = p.rinfo;
    r.fl.buf = buf;
  } else {
    tiled(!reg ? GEMM_LDS_EPI : variant == 1 ? GEMM_GLDS : GEMM_REG, BM, BN, NT, reg ? LDS_REG : LDS_EPI);
    r.fl.f32 = p.out_f32;
  }
  return r;
}

// ---- weight gradient ----

struct WgradProblem {
  int M = 0, N = 0, Cin = 0, ks = 1, pad = 0;
  bool packed = false;  // rinfo given
  bool cu = false;      // packed rows' sequence offsets given
  int nseq = 0;
  int max_splits = 1;
  long ws_floats = 0;
};

enum { WGRAD_NONE, WGRAD_BIG64, WGRAD_REG, WGRAD_DMA };

struct WgradFlags { bool packed, imm, buf, pp; };
constexpr bool operator==(const WgradFlags& a, const WgradFlags& b) {
  return a.packed == b.packed && a.imm == b.imm && a.buf == b.buf && a.pp == b.pp;
}
// {packed, imm, buf, pp}: the ping-pong loop exists on the buffer-descriptor path, single-wait schedule, only
constexpr WgradFlags kWgradBig64Flags[] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}, {0, 0, 1},
                                           {1, 0, 1}, {0, 1, 1}, {1, 1, 1}, {0, 0, 1, 1}, {1, 0, 1, 1}};
constexpr WgradFlags kWgrad128Flags[] = {{1}, {0}};  // WGRAD_REG and WGRAD_DMA: {packed}

struct WgradRoute {
  int rc = 0;  // 0, -2 (Cin or N not a multiple of 8) or -3 (the workspace does not hold one split)
  int kind = WGRAD_NONE;  // NONE with rc 0: M == 0, the gradients are zero
  WgradFlags fl{};
  int tiles = 0, splits = 0, rows_per_split = 0;
  int grid_x = 0, block = 0, lds = 0;
};

// Split-M count of the 256x256 weight-gradient kernel (one block per CU): the blocks run in
// ceil(tiles * S / CUs) rounds of ceil(M / S / 64) row steps each, and every split adds a 256x256
// fp32 slab to write and reduce (~8 % of a 64-row step per slab tile).  The old fixed target of 512
// blocks left partial rounds (packed k9 wgrad: 36 tiles x 15 = 540 blocks = 2.1 rounds -> 3) and,
// capped by the 128x128 kernels' split limit, single-tile weights ran on 64 CUs.
inline int choose_wgrad_splits(int tiles, int M, int max_splits, long ws_splits, int cus, int fixed_blocks) {
  const int steps_all = (M + 63) / 64;
  int smax = max_splits;
  if (smax > steps_all / 4) smax = steps_all / 4 > 0 ? steps_all / 4 : 1;  // >= 4 row steps per split
  if ((long)smax > ws_splits) smax = (int)ws_splits;
  if (smax < 1) return (int)(ws_splits >= 1 ? 1 : 0);
  if (fixed_blocks > 0) {
    const int sp = (fixed_blocks + tiles - 1) / tiles;
    return sp < smax ? sp : smax;
  }
  int best = 1;
  double best_c = 1e30;
  for (int sp = 1; sp <= smax; ++sp) {
    const long rounds = ((long)tiles * sp + cus - 1) / cus;
    const long steps = (steps_all + sp - 1) / sp;
    const double c = (double)rounds * (double)steps + 0.08 * (double)sp * tiles;
    if (c < best_c - 1e-9) { best_c = c; best = sp; }
  }
  return best;
}

// cus: the CU budget that applies to this launch (the side-stream budget or the device's count)
inline WgradRoute wgrad_route(const WgradProblem& p, const GemmKnobs& k, int cus) {
  WgradRoute r;
  if (p.Cin % 8 != 0 || p.N % 8 != 0) { r.rc = -2; return r; }
  if (p.M == 0) return r;
  const int M = p.M, N = p.N, K = p.ks * p.Cin;
  const long slab = (long)N * K;
  r.fl.packed = p.packed;
  // 256x256 kernel (split-M slabs + fixed-order reduce) when there are >= 2 output tiles; variant 0
  // forces the 128x128 kernels (the choice for single-tile and narrow problems)
  const bool big = k.wgrad_variant != 0 && N >= 256 && K >= 256 && (long)N * K >= 2L * 256 * 256 &&
                   (!p.packed || (p.cu && p.nseq > 0 && p.nseq < 8192));
  int splits;
  if (big) {
    r.tiles = ((N + 255) / 256) * ((K + 255) / 256);
    splits = choose_wgrad_splits(r.tiles, M, p.max_splits, p.ws_floats / (slab + N), cus, k.wgrad_blocks);
  } else {
    r.tiles = ((N + 127) / 128) * ((K + 127) / 128);
    splits = (1536 + r.tiles - 1) / r.tiles;
    const int max_by_rows = (M + 511) / 512;
    if (splits > max_by_rows) splits = max_by_rows;
    if (splits > p.max_splits) splits = p.max_splits;
    if ((long)splits * (slab + N) > p.ws_floats) splits = (int)(p.ws_floats / (slab + N));
  }
  if (splits < 1) { r.rc = -3; return r; }
  r.rows_per_split = ((M + splits - 1) / splits + 63) / 64 * 64;
  r.splits = (M + r.rows_per_split - 1) / r.rows_per_split;
  r.grid_x = r.tiles * r.splits;
  if (big) {
    r.kind = WGRAD_BIG64;
    r.block = rk::NT3;
    r.lds = rk::WB64_LDS;
    // buffer-descriptor DMA needs every byte offset in 31 bits (out-of-range marker 0x80000000)
    r.fl.buf = k.wgrad_buf != 0 && (long)(M + p.pad) * p.Cin * 2 < (1L << 31) &&
               (long)r.rows_per_split * N * 2 < (1L << 31);
    r.fl.pp = r.fl.buf && (k.wgrad_pp < 0 ? p.packed : k.wgrad_pp != 0);
    // immediate-offset fragment reads: measured faster on packed rows (the decoder FFN), the
    // single-wait schedule on plain rows (tools/exp_packed_wgrad.py); wgrad_imm overrides
    r.fl.imm = !r.fl.pp && (k.wgrad_imm < 0 ? p.packed : k.wgrad_imm != 0);
  } else {
    r.kind = K > 1024 ? WGRAD_REG : WGRAD_DMA;
    r.block = rk::NT;
    r.lds = rk::W128_LDS;
  }
  return r;
}

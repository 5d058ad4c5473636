// Host self-test of the GEMM dispatch (gemm_route.h).  A sweep over shapes, operand / epilogue forms and switches
// asserts on every route what a launch relies on (an instantiation that exists, descriptor offsets below 2^31, the
// grid of the chosen tile, workspace bounds); a list of routes derived by hand from the rules and their measurement
// tables pins the decisions themselves.
#include <cstdio>

#include "gemm_route.h"

static int fails = 0;
#define CHECK(c, ...)                         \
  do {                                        \
    if (!(c)) {                               \
      if (++fails <= 20) {                    \
        std::printf("FAIL %s: ", #c);         \
        std::printf(__VA_ARGS__);             \
        std::printf("\n");                    \
      }                                       \
    }                                         \
  } while (0)

static const long LIM31 = 1L << 31;
static long cdivl(long a, long b) { return (a + b - 1) / b; }

static void check_route(const GemmProblem& p, const GemmKnobs& k, int cus, const char* what) {
  const GemmRoute r = gemm_route(p, k, cus);
  const long M = p.M, N = p.N, K = (long)p.ks * p.Cin;
  const GemmFlags& f = r.fl;
#define CTX "%s: M %ld N %ld Cin %d ks %d f32 %d ldy %d act %d variant %d splitk %d k256 %d cus %d -> kind %d rc %d", what, \
            M, N, p.Cin, p.ks, (int)p.out_f32, p.ldy, p.act, k.variant, k.splitk, k.k256, cus, r.kind, r.rc
  CHECK(r.rc == 0 || r.rc == -2 || r.rc == -3, CTX);
  CHECK((r.rc == -2) == (p.Cin % 8 != 0), CTX);
  if (r.rc < 0) {
    CHECK(r.kind == GEMM_NONE, CTX);
    return;
  }
  const bool xon = p.acc || p.y2 || p.post_act || !p.scale_one;
  int in_table = -1;
  switch (r.kind) {
    case GEMM_SKINNY: in_table = flags_index(kSkinnyFlags, f); break;
    case GEMM_SPLITK:
    case GEMM_BIG64: in_table = flags_index(kBig64Flags, f); break;
    case GEMM_RING: in_table = flags_index(kRingFlags, f); break;
    case GEMM_K256: in_table = flags_index(kK256Flags, f); break;
    case GEMM_GLDS:
    case GEMM_REG:
    case GEMM_LDS_EPI: in_table = flags_index(kC128Flags, f); break;
    default: break;
  }
  CHECK(in_table >= 0, CTX);
  CHECK(r.grid_x > 0 && r.grid_y > 0 && r.block > 0, CTX);
  if (f.buf) {
    CHECK(f.fastk && p.Cin % 64 == 0, CTX);
    CHECK((M + p.pad) * p.Cin * 2 < LIM31 && N * K * 2 + 512 < LIM31, CTX);
  }
  if (f.fastk) CHECK(p.Cin % 64 == 0, CTX);
  if (f.stg) CHECK(f.buf && K >= 512, CTX);
  if (f.epi == rk::EPI_MASK) CHECK(!f.f32 && f.buf && p.mask_in && !p.out_f32, CTX);
  if (f.epi == rk::EPI_BNH) CHECK(p.bnh && !f.packed && !f.f32 && !p.out_f32, CTX);
  if (p.bnh) CHECK(r.kind == GEMM_BIG64 && f.epi == rk::EPI_BNH, CTX);
  if (p.mask_out) CHECK(r.kind == GEMM_BIG64 && p.act == rk::ACT_RELU, CTX);
  if (p.mask_in) CHECK(r.kind == GEMM_BIG64 || r.kind == GEMM_K256, CTX);
  if (xon && !p.bnh) CHECK(r.kind == GEMM_SKINNY || r.kind == GEMM_SPLITK || r.kind == GEMM_BIG64 || r.kind == GEMM_RING, CTX);
  CHECK(r.ksplit == 0 || (r.ksplit == p.ksplit && p.ks == 3 && p.Cin % 64 == 0 && p.ksplit % 256 == 0 && p.ksplit < N), CTX);
  const long tiles256 = cdivl(M, 256) * cdivl(N, 256);
  switch (r.kind) {
    case GEMM_SKINNY:
      CHECK(k.skinny && M <= k.skinny_maxm && N % 16 == 0, CTX);
      CHECK(r.grid_x == N / 16 && r.grid_y == cdivl(M, 16) && r.block == 64 * f.waves && r.lds == 0, CTX);
      CHECK((f.waves == 8) == (k.skinny_w8 > 0 && K / 32 >= k.skinny_w8) && (f.waves == 8 || f.waves == 4), CTX);
      CHECK(f.aligned == (p.Cin % 32 == 0), CTX);
      break;
    case GEMM_SPLITK:
      CHECK(r.grid_x == tiles256 && r.grid_y == r.S && r.block == 512 && r.lds == rk::B64_LDS, CTX);
      CHECK(f.f32 && f.packed == p.rinfo && f.epi == rk::EPI_GEN && !f.stg, CTX);
      CHECK(r.S >= 2 && N >= 256 && p.ldy == N && !p.mask_in && !p.mask_out && !p.bnh, CTX);
      if (k.splitk < 0) {
        CHECK(r.S <= 8 && tiles256 * r.S <= k.num_cus_gemm, CTX);
        CHECK((long)r.S * M * N * 4 <= (64L << 20), CTX);  // the workspace is sized once
      }
      break;
    case GEMM_K256:
      CHECK(k.k256 != 0 && p.ks == 1 && p.Cin == 256 && N % 256 == 0 && !p.out_f32, CTX);
      CHECK(!p.aux && !p.resid && !p.lens && !p.rinfo && !p.acc && !p.y2 && !p.post_act && !p.mask_out && !p.bnh, CTX);
      CHECK(p.scale_one && p.act == 0 && p.ldy == N && p.ksplit == 0, CTX);
      CHECK((M + 4 * K256_ROWS) * N * 2 < LIM31, CTX);
      if (k.k256 < 0) CHECK(M >= 2048 && k.variant < 0, CTX);
      CHECK(r.ng == N / 256 && r.nb >= 1 && r.nb <= k256_chunks(p.M) && r.grid_x == r.nb * r.ng && r.grid_y == 1, CTX);
      CHECK(r.block == 512 && r.lds == rk::K2_LDS && f.mask == p.mask_in && f.has_bias == p.bias, CTX);
      break;
    case GEMM_BIG64:
      CHECK(r.grid_x == tiles256 && r.grid_y == 1 && r.block == 512 && r.lds == rk::B64_LDS && N >= 256, CTX);
      CHECK(f.f32 == p.out_f32 && (p.bnh || f.packed == p.rinfo), CTX);
      break;
    case GEMM_RING:
      CHECK(r.grid_x == cdivl(M, 256) * cdivl(N, 128) && r.grid_y == 1 && r.block == 512 && r.lds == rk::RING_LDS, CTX);
      CHECK(f.f32 == p.out_f32 && f.packed == p.rinfo && !p.mask_in && !p.mask_out, CTX);
      break;
    default:  // the 128x128 kernels implement neither packed rows' flag nor EpiX nor the bitmask
      CHECK(r.grid_x == cdivl(M, 128) * cdivl(N, 128) && r.grid_y == 1 && r.block == 256, CTX);
      CHECK(r.lds == (r.kind == GEMM_LDS_EPI ? rk::LDS_EPI : rk::LDS_REG) && f.f32 == p.out_f32, CTX);
      CHECK(!xon && !p.mask_in && !p.mask_out, CTX);
      CHECK((r.kind == GEMM_LDS_EPI) == (N % 4 != 0 || p.ldy % 4 != 0 || k.force_lds_epilogue), CTX);
  }
#undef CTX
}

// The forms the library's entry points produce (ssamd_conv_gemm, _ex / _ex2 / _ex3, _bnbwd, _mask), each operand
// and epilogue flag alone and in the pairs that occur together.
static int make_forms(GemmProblem* out) {
  int n = 0;
  const auto add = [&](GemmProblem p) { out[n++] = p; return &out[n - 1]; };
  const GemmProblem z;
  for (int m = 0; m < 16; ++m) {  // ssamd_conv_gemm: bias, aux, resid, lens
    if (__builtin_popcount(m) > 2) continue;
    GemmProblem* p = add(z);
    p->bias = m & 1; p->aux = m & 2; p->resid = m & 4; p->lens = m & 8;
  }
  for (int m = 0; m < 16; ++m) {  // the extended epilogue: acc, y2, scale, post_act with bias / resid
    if (__builtin_popcount(m) > 2 || m == 0) continue;
    for (int pa : {rk::ACT_LRELU, 3}) {
      GemmProblem* p = add(z);
      p->bias = true; p->acc = m & 1; p->y2 = m & 2; p->scale_one = !(m & 4); p->post_act = (m & 8) ? pa : 0;
      p->resid = m == 1;
    }
  }
  for (int ksplit : {256, 512, 100}) add(z)->ksplit = ksplit;  // _ex2 / _ex3 without an extended operand
  add(z)->ksplit = 256, out[n - 1].acc = true;
  for (int pa = 0; pa < 3; ++pa) {  // _bnbwd
    GemmProblem* p = add(z);
    p->bnh = p->acc = p->bn_stats = p->bn_part = true; p->post_act = pa;
  }
  for (int m = 1; m < 4; ++m)  // _mask
    for (int bias = 0; bias < 2; ++bias) {
      GemmProblem* p = add(z);
      p->mask_in = m & 1; p->mask_out = m & 2; p->bias = bias;
    }
  return n;
}

static void sweep() {
  static GemmProblem forms[128];
  const int nforms = make_forms(forms);
  GemmKnobs knobs[16];
  int nk = 1;
  for (int v : {0, 1, 2, 4, 5}) knobs[nk++].variant = v;
  for (int v : {0, 4}) knobs[nk++].splitk = v;  // -1 is the default
  for (int v : {0, 1}) knobs[nk++].k256 = v;
  knobs[nk++].skinny = 0;
  knobs[nk++].force_lds_epilogue = true;
  const int Ms[] = {1, 15, 16, 17, 1024, 1025, 2047, 2048, 14336, 28671, 28672, 100352, 4194304};
  const int Ns[] = {8, 16, 20, 80, 128, 256, 320, 512, 768, 1024, 2048};
  const int Cins[] = {8, 32, 64, 80, 256, 1024};
  for (int M : Ms) for (int N : Ns) for (int Cin : Cins) for (int ks : {1, 3, 9})
    for (int fi = 0; fi < nforms; ++fi) {
      GemmProblem p = forms[fi];
      p.M = M; p.N = N; p.Cin = Cin; p.ks = ks; p.pad = (ks - 1) / 2;
      const bool plain_entry = !p.bnh && !p.mask_in && !p.mask_out && !p.acc && !p.y2 && !p.post_act && p.scale_one &&
                               !p.ksplit;  // ssamd_conv_gemm alone takes out_f32, ldy and act < 0
      for (int f32 = 0; f32 < 2; ++f32) for (int packed = 0; packed < 2; ++packed)
        for (int ldy : {N, N + 8, N + 1}) for (int act : {0, 1, -1}) {
          if (!plain_entry && (ldy != N || act < 0)) continue;
          if (p.bnh && (packed || act)) continue;
          p.out_f32 = f32; p.rinfo = packed; p.ldy = ldy; p.act = act;
          for (int ki = 0; ki < nk; ++ki) for (int cus : {64, 256}) check_route(p, knobs[ki], cus, "sweep");
        }
    }
  GemmProblem e;
  e.Cin = 256; e.N = 256; e.ldy = 256;
  CHECK(gemm_route(e, knobs[0], 256).rc == 0 && gemm_route(e, knobs[0], 256).kind == GEMM_NONE, "M = 0");
  e.M = 4096; e.N = 0;
  CHECK(gemm_route(e, knobs[0], 256).rc == 0 && gemm_route(e, knobs[0], 256).kind == GEMM_NONE, "N = 0");
  e.M = 0; e.Cin = 12;  // Cin % 8 is tested before the empty problem
  CHECK(gemm_route(e, knobs[0], 256).rc == -2, "Cin 12, M = 0");
}

// ---- pinned routes: default switches, 256 CUs; each expectation is read off the rule named beside it ----

static GemmProblem lin(int M, int N, int Cin = 256, int ks = 1) {  // bias, bf16 out, ldy == N
  GemmProblem p;
  p.M = M; p.N = N; p.Cin = Cin; p.ks = ks; p.pad = (ks - 1) / 2; p.ldy = N; p.bias = true;
  return p;
}
static GemmFlags b64(bool f32, bool fastk, bool packed, bool buf, int epi = rk::EPI_GEN, bool stg = false) {
  return GemmFlags{f32, fastk, packed, buf, epi, stg};
}
static void pin(const char* name, const GemmProblem& p, const GemmKnobs& k, int kind, GemmFlags fl, int gx, int gy = 1,
                int rc = 0) {
  const GemmRoute r = gemm_route(p, k, 256);
  CHECK(r.rc == rc && r.kind == kind && r.fl == fl && (rc < 0 || (r.grid_x == gx && r.grid_y == gy)),
        "%s: rc %d kind %d grid (%d, %d) flags f32 %d fastk %d packed %d buf %d epi %d stg %d waves %d al %d mask %d hb %d",
        name, r.rc, r.kind, r.grid_x, r.grid_y, r.fl.f32, r.fl.fastk, r.fl.packed, r.fl.buf, r.fl.epi, r.fl.stg,
        r.fl.waves, r.fl.aligned, r.fl.mask, r.fl.has_bias);
}

static void pinned() {
  const GemmKnobs d;
  GemmFlags k256f{}, k256m{};
  k256f.has_bias = k256m.has_bias = k256m.mask = true;
  GemmFlags sk4{}, sk8{};
  sk4.waves = 4; sk8.waves = 8; sk4.aligned = sk8.aligned = true;
  GemmProblem p;
  // K = 256 table, "N >= 1024 (ReLU-mask dgrad) from 2048 rows"; the grid is one block per CU: 256 / (N / 256) per group
  p = lin(100352, 1024); p.mask_in = true;
  pin("w2 dgrad 100352", p, d, GEMM_K256, k256m, 256);
  p = lin(2048, 1024); p.mask_in = true;  // 2048 rows = 32 chunks of 64 < 64 blocks per group: one block per chunk
  pin("w2 dgrad 2048", p, d, GEMM_K256, k256m, 32 * 4);
  // "N = 512 / 768 (QKV) from 28672 rows": 448 chunks, 256 / 3 = 85 blocks per group
  pin("qkv 28672", lin(28672, 768), d, GEMM_K256, k256f, 85 * 3);
  // "8192 / 14336 rows LOSE": the 256x256 tile (N >= 256 -> variant 4, 56 x 3 tiles); Cin % 64 == 0 and small
  // offsets -> fastk and buf; the staggered loop needs K >= 512
  pin("qkv 14336", lin(14336, 768), d, GEMM_BIG64, b64(0, 1, 0, 1), 56 * 3);
  // "N = 256 ... <= 64 tiles, where the 256x128 ring ran": 56 tiles; 224 chunks, 256 blocks -> one per chunk
  pin("fc 14336", lin(14336, 256), d, GEMM_K256, k256f, 224);
  GemmKnobs no_k256;
  no_k256.k256 = 0;  // the small-M tile note: N == 256 and <= 64 big tiles -> the ring (Cin % 64 == 0), 56 x 2 tiles
  pin("fc 14336, k256 off", lin(14336, 256), no_k256, GEMM_RING, b64(0, 1, 0, 1), 56 * 2);
  // "up to one wave the balanced 256x256 tiles win": 112 tiles, 2 * 112 < 3 * 256
  pin("fc 28672", lin(28672, 256), d, GEMM_BIG64, b64(0, 1, 0, 1), 112);
  // "from 1.5 waves of 256-row tiles": 392 tiles, 2 * 392 >= 3 * 256; 1568 chunks over 256 blocks
  pin("fc 100352", lin(100352, 256), d, GEMM_K256, k256f, 256);
  // skinny: M <= skinny_maxm = 1024; K / 32 = 8 < skinny_w8 = 16 -> 4 waves; grid (N / 16, M / 16)
  pin("skinny", lin(1024, 256), d, GEMM_SKINNY, sk4, 16, 64);
  pin("skinny k9", lin(1024, 256, 256, 9), d, GEMM_SKINNY, sk8, 16, 64);  // K / 32 = 72 >= 16 -> 8 waves
  // the split-K notes: 43 tiles <= 128, 144 k-steps >= 16: S = min(8, 256 / 43 = 5, 144 / 6 = 24) = 5
  pin("k9 dgrad 10800", lin(10800, 256, 1024, 9), d, GEMM_SPLITK, b64(1, 1, 0, 1), 43, 5);
  CHECK(gemm_route(lin(10800, 256, 1024, 9), d, 256).S == 5, "k9 dgrad 10800: S");
  // N < 256: the 256x128 ring when Cin % 64 == 0 (56 x 1 tiles), the 128x128 LDS-DMA kernel otherwise (112 x 1)
  pin("N 80", lin(14336, 80), d, GEMM_RING, b64(0, 1, 0, 1), 56);
  pin("N 128, 80 mel channels", lin(14336, 128, 80), d, GEMM_GLDS, GemmFlags{}, 112);
  // N == 256 at 56 <= 64 big tiles leaves the 256x256 tile ("variant = (Cin % BK == 0) ? 2 : 1"): Cin = 80 ->
  // LDS-DMA 128x128, 112 x 2 tiles.  The big tile without fastk takes N = 256 from 65 tiles on (112 here).
  pin("N 256, 80 mel channels, 56 tiles", lin(14336, 256, 80), d, GEMM_GLDS, GemmFlags{}, 224);
  pin("N 256, 80 mel channels, 112 tiles", lin(28672, 256, 80), d, GEMM_BIG64, b64(0, 0, 0, 0), 112);
  // the epilogue constraints
  p = lin(14336, 1024); p.mask_out = true; p.act = 0;  // "if (mask_out && act != ACT_RELU) return -3"
  pin("mask_out without ReLU", p, d, GEMM_NONE, GemmFlags{}, 0, 1, -3);
  p.act = rk::ACT_RELU;  // ... and with it: big64, generic epilogue (EPI_MASK is the mask_in-only form)
  pin("mask_out", p, d, GEMM_BIG64, b64(0, 1, 0, 1), 56 * 4);
  GemmKnobs v1;
  v1.variant = 1;
  p = lin(14336, 128); p.acc = true;  // "if (N >= 256) variant = 4; else if (variant != 2) return -3"
  pin("EpiX, N 128, variant 1", p, v1, GEMM_NONE, GemmFlags{}, 0, 1, -3);
  p = lin(14336, 512, 512, 5); p.bias = false; p.bnh = p.acc = p.bn_stats = p.bn_part = true; p.out_f32 = true;
  pin("bnh, fp32 out", p, d, GEMM_NONE, GemmFlags{}, 0, 1, -3);  // the BatchNorm head's first test lists out_f32
  p.out_f32 = false;  // K = 2560 >= 512: staggered loop (bnh_stg), 56 x 2 tiles
  pin("bnh", p, d, GEMM_BIG64, b64(0, 1, 0, 1, rk::EPI_BNH, 1), 112);
  p = lin(14336, 1024, 256, 9); p.mask_in = true; p.rinfo = true;  // k9 ReLU-mask dgrad on packed rows: EPI_MASK, staggered
  pin("k9 mask dgrad", p, d, GEMM_BIG64, b64(0, 1, 1, 1, rk::EPI_MASK, 1), 56 * 4);
}

// ---- weight gradient ----

static void check_wgrad(const WgradProblem& p, const GemmKnobs& k, int cus) {
  const WgradRoute r = wgrad_route(p, k, cus);
  const long M = p.M, N = p.N, K = (long)p.ks * p.Cin, slab = N * K;
#define CTX "wgrad M %ld N %ld Cin %d ks %d packed %d cu %d max %d ws %ld cus %d -> kind %d rc %d splits %d rows %d", M, N, \
            p.Cin, p.ks, (int)p.packed, (int)p.cu, p.max_splits, p.ws_floats, cus, r.kind, r.rc, r.splits, r.rows_per_split
  CHECK((r.rc == -2) == (p.Cin % 8 != 0 || N % 8 != 0), CTX);
  if (r.rc == -2) return;
  CHECK((r.rc == -3) == (p.ws_floats < slab + N), CTX);  // not even one split fits
  CHECK(r.rc == 0 || r.rc == -3, CTX);
  if (r.rc < 0) { CHECK(r.kind == WGRAD_NONE, CTX); return; }
  CHECK(r.kind != WGRAD_NONE, CTX);
  CHECK(r.splits >= 1 && r.splits <= p.max_splits && (long)r.splits * (slab + N) <= p.ws_floats, CTX);
  CHECK(r.rows_per_split > 0 && r.rows_per_split % 64 == 0, CTX);
  CHECK((long)r.splits * r.rows_per_split >= M && (long)(r.splits - 1) * r.rows_per_split < M, CTX);
  const bool big = r.kind == WGRAD_BIG64;
  CHECK(big == (k.wgrad_variant != 0 && N >= 256 && K >= 256 && N * K >= 2L * 256 * 256 &&
                (!p.packed || (p.cu && p.nseq > 0 && p.nseq < 8192))), CTX);
  const long tile = big ? 256 : 128;
  CHECK(r.tiles == cdivl(N, tile) * cdivl(K, tile) && r.grid_x == r.tiles * r.splits, CTX);
  CHECK((big ? flags_index(kWgradBig64Flags, r.fl) : flags_index(kWgrad128Flags, r.fl)) >= 0 && r.fl.packed == p.packed, CTX);
  CHECK(r.block == (big ? 512 : 256) && r.lds == (big ? rk::WB64_LDS : rk::W128_LDS), CTX);
  if (r.fl.pp) CHECK(r.fl.buf, CTX);
  if (r.fl.buf) CHECK((M + p.pad) * p.Cin * 2 < LIM31 && (long)r.rows_per_split * N * 2 < LIM31, CTX);
  if (!big) CHECK((r.kind == WGRAD_REG) == (K > 1024), CTX);
#undef CTX
}

static void wgrad_sweep() {
  GemmKnobs knobs[12];
  int nk = 1;
  knobs[nk++].wgrad_variant = 0;
  knobs[nk++].wgrad_blocks = 512;
  knobs[nk++].wgrad_buf = 0;
  for (int v : {0, 1}) knobs[nk++].wgrad_pp = v;
  for (int v : {0, 1}) knobs[nk++].wgrad_imm = v;
  for (int M : {1, 63, 64, 1000, 14336, 100352, 4194304}) for (int N : {8, 20, 128, 256, 512, 1024})
    for (int Cin : {8, 12, 80, 256, 1024}) for (int ks : {1, 5, 9}) for (int form = 0; form < 3; ++form)
      for (int max_splits : {1, 14, 64, 256}) for (int wsn : {0, 1, 2, 4}) {
        WgradProblem p;
        p.M = M; p.N = N; p.Cin = Cin; p.ks = ks; p.pad = (ks - 1) / 2;
        p.packed = form > 0; p.cu = form == 2; p.nseq = form == 2 ? 32 : 0;
        p.max_splits = max_splits;
        const long one = (long)N * ks * Cin + N;  // 0, one split less a float, half and all of max_splits
        p.ws_floats = wsn == 0 ? 0 : wsn == 1 ? one - 1 : one * ((max_splits + (wsn == 2)) / (wsn == 2 ? 2 : 1));
        for (int ki = 0; ki < nk; ++ki) for (int cus : {64, 256}) check_wgrad(p, knobs[ki], cus);
      }
}

static void pin_wgrad(const char* name, const WgradProblem& p, int kind, WgradFlags fl, int tiles, int splits, int rows) {
  const WgradRoute r = wgrad_route(p, GemmKnobs{}, 256);
  CHECK(r.rc == 0 && r.kind == kind && r.fl == fl && r.tiles == tiles && r.splits == splits && r.rows_per_split == rows,
        "%s: rc %d kind %d flags %d %d %d %d tiles %d splits %d rows %d", name, r.rc, r.kind, r.fl.packed, r.fl.imm,
        r.fl.buf, r.fl.pp, r.tiles, r.splits, r.rows_per_split);
}

// max_splits and the workspace as the Python binding sizes them; split counts from choose_wgrad_splits at 256 CUs
static void wgrad_pinned() {
  WgradProblem p;
  // decoder FFN k = 9 on packed rows: 4 x 9 tiles; 7 splits x 36 = 252 blocks = one round; packed -> ping-pong loop
  p.M = 100352; p.N = 1024; p.Cin = 256; p.ks = 9; p.pad = 4; p.packed = p.cu = true; p.nseq = 128;
  p.max_splits = 14; p.ws_floats = 14L * (1024 * 2304 + 1024);
  pin_wgrad("decoder k9 packed", p, WGRAD_BIG64, WgradFlags{1, 0, 1, 1}, 36, 7, 14336);
  // PostNet k = 5 on plain rows: 2 x 10 tiles; 12 splits x 20 = 240 blocks; ceil(100352 / 12) = 8363 -> 8384 rows;
  // plain rows -> the single-wait schedule, no ping-pong
  p = WgradProblem{};
  p.M = 100352; p.N = 512; p.Cin = 512; p.ks = 5; p.pad = 2; p.max_splits = 24; p.ws_floats = 24L * (512 * 2560 + 512);
  pin_wgrad("PostNet k5", p, WGRAD_BIG64, WgradFlags{0, 0, 1, 0}, 20, 12, 8384);
  // a 256 x 256 Linear is one 256x256 tile (N * K < 2 tiles): the 128x128 LDS-DMA kernel (K <= 1024), 4 tiles;
  // splits = min(1536 / 4, rows / 512 = 196, max_splits) = 196 of 512 rows
  p = WgradProblem{};
  p.M = 100352; p.N = 256; p.Cin = 256; p.max_splits = 256; p.ws_floats = 256L * (256 * 256 + 256);
  pin_wgrad("Linear 256", p, WGRAD_DMA, WgradFlags{0, 0, 0, 0}, 4, 196, 512);
}

int main() {
  sweep();
  pinned();
  wgrad_sweep();
  wgrad_pinned();
  if (fails) {
    std::printf("selftest_gemm_route: %d failures\n", fails);
    return 1;
  }
  std::printf("selftest_gemm_route ok\n");
  return 0;
}

// Host self-test of the iSTFTNet head's index arithmetic (istft_index.h), n_fft 16 / hop 4.  For every T in
// 2..200 and tile heights 32, 64 and 128, against a brute-force overlap-add over all frames 0..T: every sample
// of [0, 4 T) is owned by exactly one tile; the covering-frame range of a sample equals the brute-force set and
// lies inside the frames its tile computes; every padded position such a frame reads is staged by the tile and
// maps to a row of the utterance (position 0 to row 1) inside the documented row range; and the envelope equals
// the brute-force sum of squared window values (1.5 in the interior, never below 1.25).
#include <cmath>
#include <cstdio>
#include <vector>

#include "istft_index.h"

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

int main() {
  constexpr int N = 16, H = 4;
  static_assert(istft_frame_halo(N, H) == 1 && istft_tile_frames(64, N, H) == 67 &&
                    istft_tile_positions(64, N, H) == 73,
                "tile geometry of n_fft 16 / hop 4");
  for (int i = 0; i < N; ++i) {
    const double w = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / N);
    CHECK(std::fabs((double)istft_hann16(i) - w) < 6e-8, "window[%d] = %.9g vs %.17g", i, istft_hann16(i), w);
  }
  long checked = 0;
  const int heights[] = {32, 64, 128};
  for (int bm : heights)
    for (int T = 2; T <= 200; ++T) {
      std::vector<int> owner((size_t)H * T, 0);
      for (int t0 = 0; t0 < T; t0 += bm) {
        const int fr0 = istft_tile_frame0(t0, N, H), nfr = istft_tile_frames(bm, N, H);
        const int p0 = istft_tile_pos0(t0, N, H), npos = istft_tile_positions(bm, N, H);
        CHECK(fr0 == t0 - 1 && nfr == bm + 3 && p0 == t0 - 4 && npos == bm + 9, "tile t0 %d bm %d", t0, bm);
        const int b = istft_tile_sample_begin(t0, H), e = istft_tile_sample_end(t0, bm, T, H);
        CHECK(b >= 0 && b < e && e <= H * T, "T %d bm %d t0 %d: samples [%d, %d)", T, bm, t0, b, e);
        for (int n = b; n < e && n < H * T; ++n) {
          ++owner[(size_t)n];
          // brute force: every frame of 0..T whose index lies in the window
          int b0 = -1, b1 = -1;
          float env = 0.f;
          double envd = 0.0;
          for (int f = 0; f <= T; ++f) {
            const int i = n + N / 2 - H * f;
            if (i < 0 || i >= N) continue;
            if (b0 < 0) b0 = f;
            b1 = f;
            const float w = istft_hann16(i);
            env += w * w;
            const double wd = 0.5 - 0.5 * std::cos(2.0 * M_PI * i / N);
            envd += wd * wd;
          }
          const int f0 = istft_first_frame(n, N, H), f1 = istft_last_frame(n, N, H, T);
          CHECK(b0 >= 0 && f0 == b0 && f1 == b1, "T %d n %d: frames [%d, %d] vs brute [%d, %d]", T, n, f0, f1, b0, b1);
          CHECK(f0 >= fr0 && f1 < fr0 + nfr && f0 >= n / H - 1 && f1 <= n / H + 2,
                "T %d bm %d t0 %d n %d: frames [%d, %d] outside the tile's [%d, %d]", T, bm, t0, n, f0, f1, fr0,
                fr0 + nfr - 1);
          const float eh = istft_env16(n, H, T);
          CHECK(eh == env, "T %d n %d: envelope %.9g vs brute %.9g", T, n, eh, env);
          CHECK(std::fabs((double)eh - envd) < 1e-6 && eh >= 1.25f - 1e-6f, "T %d n %d: envelope %.9g vs %.17g", T, n,
                eh, envd);
          if (n >= N / 2 && n < H * T - N / 2) CHECK(std::fabs(envd - 1.5) < 1e-12, "interior envelope %.17g", envd);
          for (int f = f0; f <= f1; ++f)
            for (int tap = 0; tap < ISTFT_TAPS; ++tap) {
              const int j = f + tap - (ISTFT_TAPS - 1) / 2;
              CHECK(j >= p0 && j < p0 + npos, "T %d bm %d t0 %d: position %d not staged [%d, %d)", T, bm, t0, j, p0,
                    p0 + npos);
              const int r = istft_pos_row(j, T);
              if (j < 0 || j > T) {
                CHECK(r == -1, "position %d outside 0..%d maps to row %d", j, T, r);
              } else {
                CHECK(r >= 0 && r < T && r == (j == 0 ? 1 : j - 1), "T %d: position %d -> row %d", T, j, r);
                CHECK(r >= t0 - 5 && r <= t0 + bm + 3, "T %d bm %d t0 %d: row %d outside the staged rows", T, bm, t0, r);
                CHECK(r >= n / H - 6 && r <= n / H + 6, "T %d n %d: row %d beyond 6 rows", T, n, r);
              }
            }
          ++checked;
        }
      }
      for (int n = 0; n < H * T; ++n) CHECK(owner[(size_t)n] == 1, "T %d bm %d: sample %d owned %d times", T, bm, n, owner[(size_t)n]);
      // a tile past the utterance owns nothing
      const int tp = ((T + bm - 1) / bm) * bm;
      CHECK(istft_tile_sample_end(tp, bm, T, H) == istft_tile_sample_begin(tp, H), "T %d bm %d: tile past the end", T, bm);
    }
  if (fails) {
    std::printf("selftest_istft_index: %d failures\n", fails);
    return 1;
  }
  std::printf("selftest_istft_index ok (%ld samples)\n", checked);
  return 0;
}

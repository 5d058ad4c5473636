// Host self-test of the Griffin-Lim index arithmetic (gl_frames.h).  For the geometries the kernels
// are tested at and every T from the minimum frame count to 12: the covering-frame range of every
// padded position equals a brute-force scan over all frames (and is never empty, with every offset
// inside the frame), every reflected analysis index lies in [0, N), every sample of [0, N) is read
// by some analysis frame, and the minimum frame count is the first T with N > n_fft/2.
#include <cstdio>
#include <vector>

#include "gl_frames.h"

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
  const int geo[][2] = {{1024, 256}, {512, 128}, {2048, 300}, {1024, 1024}, {512, 100}};
  long checked = 0;
  for (const auto& g : geo) {
    const int n_fft = g[0], hop = g[1];
    const int tmin = gl_min_frames(n_fft, hop);
    CHECK(gl_num_samples(tmin, hop) > n_fft / 2, "n_fft %d hop %d: N(%d) = %d", n_fft, hop, tmin,
          gl_num_samples(tmin, hop));
    CHECK(gl_num_samples(tmin - 1, hop) <= n_fft / 2, "n_fft %d hop %d: N(%d) = %d", n_fft, hop, tmin - 1,
          gl_num_samples(tmin - 1, hop));
    // the 32-bit guard: the largest T it admits keeps every position (and the reflection's 2 (N - 1)) in an int
    const long tmax = (2147483646L - n_fft) / (2L * hop);
    CHECK(gl_fits_int(tmax, n_fft, hop) && !gl_fits_int(tmax + 1, n_fft, hop) && !gl_fits_int(-1, n_fft, hop),
          "n_fft %d hop %d: guard at T = %ld", n_fft, hop, tmax);
    CHECK(2L * hop * (tmax - 1) + n_fft < 2147483647L, "guard too weak at T = %ld", tmax);
    {  // at that T the last 3 n_fft analysis positions stay exact in 32 bits (UBSan watches the header's arithmetic)
      const int T = (int)tmax, N = gl_num_samples(T, hop);
      for (int d = 0; d < 3 * n_fft; ++d) {
        const int s = gl_reflect(N + n_fft / 2 - 1 - d, N);
        CHECK(s >= 0 && s < N, "T %d: reflected %d outside [0, %d)", T, s, N);
        const long u = (long)s + n_fft / 2, a = u - n_fft + 1;
        const long e0 = a <= 0 ? 0 : (a + hop - 1) / hop, e1 = u / hop > T - 1 ? T - 1 : u / hop;
        CHECK(gl_first_frame((int)u, n_fft, hop) == e0 && gl_last_frame((int)u, hop, T) == e1, "T %d u %ld", T, u);
      }
    }
    CHECK(gl_num_samples(1, hop) == 0 && gl_num_samples(0, hop) == 0, "hop %d: T <= 1 has samples", hop);
    for (int T = 2; T <= 12; ++T) {  // the overlap-add range also serves utterances below the minimum
      const int N = gl_num_samples(T, hop);
      CHECK(N == hop * (T - 1), "N %d", N);
      for (int s = 0; s < N; ++s) {
        const int u = s + n_fft / 2;
        int b0 = -1, b1 = -1;
        for (int f = 0; f < T; ++f)
          if ((long)f * hop <= u && u < (long)f * hop + n_fft) {
            if (b0 < 0) b0 = f;
            b1 = f;
          }
        const int g0 = gl_first_frame(u, n_fft, hop), g1 = gl_last_frame(u, hop, T);
        CHECK(b0 >= 0 && g0 == b0 && g1 == b1, "n_fft %d hop %d T %d u %d: [%d, %d] vs brute [%d, %d]", n_fft, hop, T,
              u, g0, g1, b0, b1);
        for (int f = g0; f <= g1 && f < T; ++f) {
          const int o = u - f * hop;
          CHECK(f >= 0 && o >= 0 && o < n_fft, "offset %d of frame %d", o, f);
        }
        ++checked;
      }
      if (T < tmin) continue;
      std::vector<char> seen((size_t)N, 0);
      for (int f = 0; f < T; ++f)
        for (int i = 0; i < n_fft; ++i) {
          const int q = f * hop - n_fft / 2 + i;
          const int s = gl_reflect(q, N);
          CHECK(s >= 0 && s < N, "n_fft %d hop %d T %d: q %d -> %d outside [0, %d)", n_fft, hop, T, q, s, N);
          if (q >= 0 && q < N) CHECK(s == q, "q %d inside [0, %d) moved to %d", q, N, s);
          if (s >= 0 && s < N) seen[(size_t)s] = 1;
        }
      for (int s = 0; s < N; ++s) CHECK(seen[(size_t)s], "n_fft %d hop %d T %d: sample %d never read", n_fft, hop, T, s);
    }
  }
  if (fails) {
    std::printf("selftest_gl_frames: %d failures\n", fails);
    return 1;
  }
  std::printf("selftest_gl_frames ok (%ld positions)\n", checked);
  return 0;
}

// Tile / frame / row / sample index arithmetic of the iSTFTNet head kernel (k_istft.hip), shared with host code.
//
// Conventions (torch.istft(center=True) on the conv of the reflect-padded last-stage rows): an utterance of T
// rows (T >= 2) has T + 1 padded positions j = 0..T (position 0 is row 1, position j >= 1 is row j - 1) and as many
// frames f = 0..T; frame f is a 7-tap conv over positions f - 3 .. f + 3 (zeros outside 0..T).  Frame f covers
// the samples n with 0 <= n + n_fft/2 - hop*f < n_fft, and the kept samples are n in [0, hop*T).  A tile of bm
// rows at t0 owns the samples [hop*t0, hop*min(t0 + bm, T)).  Everything here is pure arithmetic on ints (and one
// 16-entry table): csrc/selftest_istft_index.cpp checks it against a brute-force overlap-add on the CPU.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISTFT_HD __host__ __device__
#else
#define ISTFT_HD
#endif

constexpr int ISTFT_TAPS = 7;  // conv_post kernel size; pad (ISTFT_TAPS - 1) / 2 positions each side

// frames beyond a tile's own rows on each side that its samples still read: floor((n_fft/2 - 1) / hop)
ISTFT_HD constexpr int istft_frame_halo(int n_fft, int hop) { return (n_fft / 2 - 1) / hop; }

// frames a tile of bm rows computes: [t0 - halo, t0 + bm + halo]
ISTFT_HD constexpr int istft_tile_frames(int bm, int n_fft, int hop) { return bm + 2 * istft_frame_halo(n_fft, hop) + 1; }

// padded positions a tile stages: [t0 - halo - 3, t0 + bm + halo + 3]
ISTFT_HD constexpr int istft_tile_positions(int bm, int n_fft, int hop) {
  return istft_tile_frames(bm, n_fft, hop) + ISTFT_TAPS - 1;
}

// first frame / first staged position of the tile at t0 (may be negative: frames / positions < 0 do not exist)
ISTFT_HD inline int istft_tile_frame0(int t0, int n_fft, int hop) { return t0 - istft_frame_halo(n_fft, hop); }
ISTFT_HD inline int istft_tile_pos0(int t0, int n_fft, int hop) {
  return istft_tile_frame0(t0, n_fft, hop) - (ISTFT_TAPS - 1) / 2;
}

// the row behind padded position j of an utterance of T rows, or -1 where the conv sees zeros
ISTFT_HD inline int istft_pos_row(int j, int T) {
  if (j < 0 || j > T) return -1;
  return j == 0 ? 1 : j - 1;
}

// samples [begin, end) of its utterance that the tile at t0 owns (empty when t0 >= T)
ISTFT_HD inline int istft_tile_sample_begin(int t0, int hop) { return hop * t0; }
ISTFT_HD inline int istft_tile_sample_end(int t0, int bm, int T, int hop) {
  const int e = t0 + bm < T ? t0 + bm : T;
  return e < t0 ? hop * t0 : hop * e;
}

// first / last frame of 0..T that covers sample n >= 0
ISTFT_HD inline int istft_first_frame(int n, int n_fft, int hop) {
  const int a = n + n_fft / 2 - n_fft + 1;
  return a <= 0 ? 0 : (a + hop - 1) / hop;
}
ISTFT_HD inline int istft_last_frame(int n, int n_fft, int hop, int T) {
  const int g = (n + n_fft / 2) / hop;
  return g > T ? T : g;
}

// periodic Hann window of length 16 (0.5 - 0.5 cos(2 pi i / 16), rounded to fp32)
ISTFT_HD inline float istft_hann16(int i) {
  constexpr float w[16] = {0.0f,         0.038060233f, 0.14644662f, 0.30865827f, 0.5f,        0.6913417f,
                           0.8535534f,   0.96193975f,  1.0f,        0.96193975f, 0.8535534f,  0.6913417f,
                           0.5f,         0.30865827f,  0.14644662f, 0.038060233f};
  return w[i & 15];
}

// overlap-add envelope of sample n (n_fft = 16): the squared window summed over the covering frames in
// ascending frame order, exactly as the kernel's and the self-test's sums run
ISTFT_HD inline float istft_env16(int n, int hop, int T) {
  const int f0 = istft_first_frame(n, 16, hop), f1 = istft_last_frame(n, 16, hop, T);
  float e = 0.f;
  for (int f = f0; f <= f1; ++f) {
    const float w = istft_hann16(n + 8 - hop * f);
    e += w * w;
  }
  return e;
}

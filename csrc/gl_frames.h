// Frame / sample index arithmetic of the Griffin-Lim kernels (k_griffin.hip), shared with host code.
//
// Conventions (torch.stft(center=True, pad_mode="reflect") / torch.istft): an utterance of T frames
// has N = hop * (T - 1) samples; frame g covers the padded positions u = g*hop .. g*hop + n_fft - 1,
// where padded position u is sample s = u - n_fft/2.  Analysis frame f reads sample q = f*hop -
// n_fft/2 + i reflected into [0, N) (no edge repeat), which needs N > n_fft/2.
// Positions inside one utterance are 32-bit (the kernels divide by hop per sample, and a 64-bit
// division costs as much as a butterfly stage): the caller keeps 2 * hop * T + n_fft below 2^31
// (gl_fits_int; the factor 2 is the reflection's).  Everything here is pure integer arithmetic:
// csrc/selftest_gl_frames.cpp proves it on the CPU.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GL_HD __host__ __device__
#else
#define GL_HD
#endif

// every position of an utterance of T frames fits an int
GL_HD inline bool gl_fits_int(long T, int n_fft, int hop) { return T >= 0 && 2L * hop * T + n_fft < 2147483647L; }

// samples of an utterance of T frames (T <= 1: none)
GL_HD inline int gl_num_samples(int T, int hop) { return T > 1 ? hop * (T - 1) : 0; }

// fewest frames at which reflect padding is defined (N > n_fft/2); shorter utterances get no iteration
GL_HD inline int gl_min_frames(int n_fft, int hop) { return n_fft / (2 * hop) + 2; }

// reflect q in [-n_fft/2, N + n_fft/2) into [0, N); valid when N > n_fft/2
GL_HD inline int gl_reflect(int q, int N) {
  if (q < 0) q = -q;
  if (q >= N) q = 2 * (N - 1) - q;
  return q;
}

// first / last frame g of 0 .. T-1 that covers padded position u >= 0 (g*hop <= u < g*hop + n_fft)
GL_HD inline int gl_first_frame(int u, int n_fft, int hop) {
  const int a = u - n_fft + 1;
  return a <= 0 ? 0 : (int)(((unsigned)a + (unsigned)hop - 1u) / (unsigned)hop);
}
GL_HD inline int gl_last_frame(int u, int hop, int T) {
  const int g = (int)((unsigned)u / (unsigned)hop);
  return g > T - 1 ? T - 1 : g;
}

// Griffin-Lim / iSTFT synthesis (reference audio/audio_processing.py:66-82, audio/stft.py:83-122;
// SURVEY A3): the synthesis half of k_audio.hip.  torch.stft(center, reflect) / torch.istft semantics,
// fp32 throughout, one workgroup per packed frame row, one launch per iteration.
//
// A batch is R = sum T_b frame rows back to back: rows[r] = {utterance, local frame}, cu[b] = first
// row of utterance b.  The state between launches is the windowed synthesis frames
// frame[R][n_fft] = w * irfft(S): the overlap-add never materialises.  An iteration's block gathers
// each of its n_fft analysis samples straight from the <= ceil(n_fft/hop) covering frames of its own
// utterance in the INPUT buffer (fixed ascending order, divided by the window envelope), then
// window -> FFT -> momentum -> project onto |mag| -> inverse FFT -> window into the OUTPUT buffer.
// No block reads what a block of the same launch writes; stream order is the only synchronisation,
// there are no atomics, and every result is bitwise reproducible and independent of the batch an
// utterance is packed into.  The index arithmetic lives in gl_frames.h (host-tested).
//
// The FFT is logmel_kernel's radix-2 decimation-in-time pass on LDS; the per-block twiddle table holds one
// contiguous run per stage (measured against the shared table in profiles/griffin_lim.txt).
#include <float.h>

#include "common.h"
#include "gl_frames.h"

namespace {

constexpr int NT = 256;

template <int NFFT>
__device__ __forceinline__ int brev(int i) {
  return (int)(__brev((unsigned)i) >> (32 - __builtin_ctz(NFFT)));
}

// Twiddles exp(-2 pi i j / (2 half)) (the forward kernel; the inverse pass conjugates), one contiguous run
// per butterfly stage at cs/sn[half + j], j < half: the lanes of a stage read consecutive words.  (One shared
// table of NFFT/2 entries indexed j * NFFT / (2 half) puts the 64 lanes of the middle stages on 2 - 8 banks.)
// The values are those of the shared table bit for bit: j / half is exact.
template <int NFFT>
__device__ __forceinline__ void twiddles(float* cs, float* sn, int tid) {
  for (int t = tid; t < NFFT / 2; t += NT) {  // the last stage: half = NFFT/2
    float s, c;
    sincospif((float)t / (float)(NFFT / 2), &s, &c);
    cs[NFFT / 2 + t] = c;
    sn[NFFT / 2 + t] = -s;
  }
  __syncthreads();
  for (int i = tid; i < NFFT / 2; i += NT) {  // stage half = 2^floor(log2 i): every (NFFT/2 / half)-th entry of the last
    if (i == 0) continue;
    const int half = 1 << (31 - __clz(i));
    const int src = NFFT / 2 + (i - half) * (NFFT / 2 / half);
    cs[i] = cs[src];
    sn[i] = sn[src];
  }
}

// in place on bit-reversed input (which the caller has synchronised); INV: unscaled inverse transform
template <int NFFT, bool INV>
__device__ __forceinline__ void fft_lds(float* re, float* im, const float* cs, const float* sn, int tid) {
  constexpr int LOG2 = __builtin_ctz(NFFT);
#pragma unroll 1
  for (int lh = 0; lh < LOG2; ++lh) {
    const int half = 1 << lh;
    for (int k = tid; k < NFFT / 2; k += NT) {
      const int j = k & (half - 1);
      const int i0 = ((k >> lh) << (lh + 1)) + j, i1 = i0 + half;
      const float wr = cs[half + j], wi = INV ? -sn[half + j] : sn[half + j];
      const float xr = re[i1] * wr - im[i1] * wi;
      const float xi = re[i1] * wi + im[i1] * wr;
      re[i1] = re[i0] - xr;
      im[i1] = im[i0] - xi;
      re[i0] += xr;
      im[i0] += xi;
    }
    __syncthreads();
  }
}

// Half spectrum held in registers (bin k = tid + j*NT) -> windowed synthesis frame dst[NFFT].
// C2R semantics: the imaginary parts of bins 0 and NFFT/2 are dropped.  The caller has synchronised
// every earlier use of re / im.
template <int NFFT, int PER>
__device__ __forceinline__ void spec_to_frame(const float (&sr)[PER], const float (&si)[PER], float* re, float* im,
                                              const float* cs, const float* sn, const float* __restrict__ window,
                                              float* __restrict__ dst, int tid) {
  constexpr int NB = NFFT / 2 + 1;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = tid + j * NT;
    if (k < NB) {
      const bool edge = (k == 0) | (k == NFFT / 2);
      const float vi = edge ? 0.f : si[j];
      const int p = brev<NFFT>(k);
      re[p] = sr[j];
      im[p] = vi;
      if (!edge) {
        const int q = brev<NFFT>(NFFT - k);
        re[q] = sr[j];
        im[q] = -vi;
      }
    }
  }
  __syncthreads();
  fft_lds<NFFT, true>(re, im, cs, sn, tid);
  constexpr float inv = 1.f / (float)NFFT;
  for (int i = tid; i < NFFT; i += NT) dst[i] = window[i] * (re[i] * inv);
}

// Overlap-add value at padded position u of an utterance whose T frames start at fr: the covering
// frames summed in ascending order over the window envelope (left undivided where the envelope is
// not above the smallest normal float: the reference's window_sumsquare rule).
template <int NFFT>
__device__ __forceinline__ float ola_sample(const float* __restrict__ fr, int u, int T, int hop,
                                            const float* __restrict__ window) {
  const int g0 = gl_first_frame(u, NFFT, hop), g1 = gl_last_frame(u, hop, T);
  float num = 0.f, den = 0.f;
  for (int g = g0; g <= g1; ++g) {
    const int o = u - g * hop;  // in [0, NFFT) by the choice of g0, g1
    const float w = window[o];
    num += fr[(long)g * NFFT + o];
    den += w * w;
  }
  return den > FLT_MIN ? num / den : num;
}

// mode 0: in = magnitude rows [R, NB]; 1: log-mel rows [R, n_mel] through pinv [NB, n_mel]; 2: complex
// spectrum rows [R, NB] (re, im interleaved: the plain iSTFT front, no phase, mag not written)
template <int NFFT>
__global__ void __launch_bounds__(NT) gl_init_kernel(const float* __restrict__ in, int mode, int n_mel,
                                                     const float* __restrict__ pinv, const float* __restrict__ phase,
                                                     unsigned seed, const int* __restrict__ rows,
                                                     const float* __restrict__ window, float* __restrict__ mag,
                                                     float* __restrict__ frame) {
  constexpr int NB = NFFT / 2 + 1;
  constexpr int PER = (NB + NT - 1) / NT;
  __shared__ float re[NFFT], im[NFFT], cs[NFFT], sn[NFFT];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int f = rows[2 * r + 1];
  twiddles<NFFT>(cs, sn, tid);
  if (mode == 1) {  // exp(mel) staged in re[] (n_mel <= NFFT, checked by the host)
    for (int m = tid; m < n_mel; m += NT) re[m] = expf(in[(long)r * n_mel + m]);
    __syncthreads();
  }
  float sr[PER], si[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = tid + j * NT;
    sr[j] = si[j] = 0.f;
    if (k < NB) {
      const long o = (long)r * NB + k;
      if (mode == 2) {
        sr[j] = in[2 * o];
        si[j] = in[2 * o + 1];
      } else {
        float m;
        if (mode == 1) {
          const float* prow = pinv + (long)k * n_mel;
          float acc = 0.f;
          for (int c = 0; c < n_mel; ++c) acc += prow[c] * re[c];
          m = fmaxf(acc, 0.f);
        } else {
          m = in[o];
        }
        mag[o] = m;
        float s, c;
        if (phase) {
          sincosf(phase[o], &s, &c);
        } else {  // uniform phase from (seed, local frame, bin): the same whatever batch the row is packed into
          const unsigned h = hash_u32(hash_u32(seed ^ (unsigned)f * 0x9E3779B9U) ^ (unsigned)k);
          sincospif((float)h * (2.f / 4294967296.f), &s, &c);
        }
        sr[j] = m * c;
        si[j] = m * s;
      }
    }
  }
  __syncthreads();  // re[] (exp(mel)) is free
  spec_to_frame<NFFT, PER>(sr, si, re, im, cs, sn, window, frame + (long)r * NFFT, tid);
}

template <int NFFT>
__global__ void __launch_bounds__(NT) gl_iter_kernel(const float* __restrict__ fin, float* __restrict__ fout,
                                                     const float* __restrict__ mag, float* __restrict__ cprev,
                                                     float momentum, int first, const int* __restrict__ rows,
                                                     const int* __restrict__ cu, int hop,
                                                     const float* __restrict__ window) {
  constexpr int NB = NFFT / 2 + 1;
  constexpr int PER = (NB + NT - 1) / NT;
  __shared__ float re[NFFT], im[NFFT], cs[NFFT], sn[NFFT];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int b = rows[2 * r], f = rows[2 * r + 1];
  const int r0 = cu[b], T = cu[b + 1] - r0;
  float* dst = fout + (long)r * NFFT;
  if (T < gl_min_frames(NFFT, hop)) {  // too short for reflect padding: zero iterations (block-uniform)
    const float* src = fin + (long)r * NFFT;
    for (int i = tid; i < NFFT; i += NT) dst[i] = src[i];
    return;
  }
  twiddles<NFFT>(cs, sn, tid);
  const int N = gl_num_samples(T, hop);  // positions of one utterance fit an int (gl_fits_int, checked by the caller)
  const float* fr = fin + (long)r0 * NFFT;
  const int start = f * hop - NFFT / 2;
  for (int i = tid; i < NFFT; i += NT) {
    const int s = gl_reflect(start + i, N);
    const float y = ola_sample<NFFT>(fr, s + NFFT / 2, T, hop, window);
    const int p = brev<NFFT>(i);
    re[p] = window[i] * y;
    im[p] = 0.f;
  }
  __syncthreads();
  fft_lds<NFFT, false>(re, im, cs, sn, tid);
  float sr[PER], si[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int k = tid + j * NT;
    sr[j] = si[j] = 0.f;
    if (k < NB) {
      const long o = (long)r * NB + k;
      const float cr = re[k], ci = im[k];
      float tr = cr, ti = ci;
      if (cprev) {  // fast Griffin-Lim: extrapolate along the last step; only this block touches its row
        if (!first) {
          tr = cr + momentum * (cr - cprev[2 * o]);
          ti = ci + momentum * (ci - cprev[2 * o + 1]);
        }
        cprev[2 * o] = cr;
        cprev[2 * o + 1] = ci;
      }
      const float m = mag[o];
      const float n = sqrtf(tr * tr + ti * ti);
      if (n > 0.f) {
        sr[j] = m * (tr / n);
        si[j] = m * (ti / n);
      } else {
        sr[j] = m;
      }
    }
  }
  __syncthreads();  // every bin is in registers before re / im are overwritten
  spec_to_frame<NFFT, PER>(sr, si, re, im, cs, sn, window, dst, tid);
}

template <int NFFT>
__global__ void __launch_bounds__(NT) gl_final_kernel(const float* __restrict__ frame, const int* __restrict__ cu,
                                                      int hop, const float* __restrict__ window, float scale,
                                                      float* __restrict__ outf, int16_t* __restrict__ outi, long W) {
  const int b = blockIdx.y;
  const long s = (long)blockIdx.x * NT + threadIdx.x;
  if (s >= W) return;
  const int r0 = cu[b], T = cu[b + 1] - r0;
  float y = 0.f;
  if (s < gl_num_samples(T, hop)) y = ola_sample<NFFT>(frame + (long)r0 * NFFT, (int)s + NFFT / 2, T, hop, window);
  const long o = (long)b * W + s;
  if (outi) {
    float v = y * scale;
    v = fminf(fmaxf(v, -32768.f), 32767.f);
    outi[o] = (int16_t)v;
  } else {
    outf[o] = y;
  }
}

inline bool gl_geometry_ok(int n_fft, int hop) {
  return (n_fft == 512 || n_fft == 1024 || n_fft == 2048) && hop > 0 && hop <= n_fft;
}

}  // namespace

#define GL_DISPATCH(KERN, GRID, ...)                                                  \
  switch (n_fft) {                                                                    \
    case 512: hipLaunchKernelGGL(KERN<512>, GRID, dim3(NT), 0, s, __VA_ARGS__); break;   \
    case 1024: hipLaunchKernelGGL(KERN<1024>, GRID, dim3(NT), 0, s, __VA_ARGS__); break; \
    default: hipLaunchKernelGGL(KERN<2048>, GRID, dim3(NT), 0, s, __VA_ARGS__); break;   \
  }

// in: mode 0 magnitude [R, NB] | 1 log-mel [R, n_mel] (pinv [NB, n_mel]) | 2 complex [R, NB, 2];
// phase [R, NB] radians or null (hash of seed, local frame, bin); rows [R, 2] {utterance, local frame}
// -> mag [R, NB] (modes 0, 1), frame [R, n_fft]
SSAMD_API int ssamd_gl_init(const float* in, int mode, int n_mel, const float* pinv, const float* phase,
                            unsigned long long seed, const int* rows, int R, int n_fft, const float* window,
                            float* mag, float* frame, hipStream_t s) {
  if (!gl_geometry_ok(n_fft, 1) || mode < 0 || mode > 2) return -2;
  if (mode == 1 && (!pinv || n_mel <= 0 || n_mel > n_fft)) return -2;
  if (mode != 2 && !mag) return -2;
  if (R <= 0) return 0;
  GL_DISPATCH(gl_init_kernel, dim3(R), in, mode, n_mel, pinv, phase, (unsigned)seed, rows, window, mag, frame);
  return (int)hipGetLastError();
}

// one Griffin-Lim iteration fin -> fout (two different [R, n_fft] buffers); cprev [R, NB, 2] or null (momentum 0)
SSAMD_API int ssamd_gl_iter(const float* fin, float* fout, const float* mag, float* cprev, float momentum, int first,
                            const int* rows, const int* cu, int R, int n_fft, int hop, const float* window,
                            hipStream_t s) {
  if (!gl_geometry_ok(n_fft, hop) || fin == fout) return -2;
  if (R <= 0) return 0;
  GL_DISPATCH(gl_iter_kernel, dim3(R), fin, fout, mag, cprev, momentum, first, rows, cu, hop, window);
  return (int)hipGetLastError();
}

// frames -> wav [B, W]: utterance b's hop * (T_b - 1) samples, zeros after; fp32 (outf) or int16 (outi, * scale, clamp)
SSAMD_API int ssamd_gl_final(const float* frame, const int* cu, int B, int n_fft, int hop, const float* window,
                             float scale, float* outf, int16_t* outi, long W, hipStream_t s) {
  if (!gl_geometry_ok(n_fft, hop)) return -2;
  if (B <= 0 || W <= 0) return 0;  // an empty output has no address
  if (!outf && !outi) return -2;
  GL_DISPATCH(gl_final_kernel, dim3(cdiv(W, NT), B), frame, cu, hop, window, scale, outf, outi, W);
  return (int)hipGetLastError();
}

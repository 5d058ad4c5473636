// Packed feature front-end of the batched preprocessing pipeline (speakingstyle_amd/data/preprocess.py with a device):
// log-mel + energy of a whole mixed-length batch in one launch, and the unvoiced frames of the F0 contours filled in.
// Semantics: ops/reference.py::frame_features (TacotronSTFT.mel_spectrogram per utterance, rows transposed and
// concatenated) and ::interp_unvoiced (data.preprocess.interpolate_unvoiced per utterance).
//
// frame_features_kernel<NFFT>: one workgroup of 4 waves per PAIR of consecutive frame rows 2p, 2p + 1 of one
// utterance (a last odd row pairs with a zero frame); the table entry of the workgroup {sample offset lo / hi, N,
// first frame, output row, rows} comes from the host (ops/reference.py::frame_pairs).
//   1  gather both frames with gl_frames.h's reflect arithmetic (optionally clamped to [-1, 1]), times the window:
//      frame a -> re, frame b -> im, at the bit-reversed position.  A frame whose windowed samples are all zero is
//      flagged (sum of squares by a block reduction) and comes out as exact zeros.
//   2  one radix-2 decimation-in-time complex FFT in LDS (log2 NFFT stages, NFFT / 2 butterflies each), then
//        Xa[k] = (Z[k] + conj Z[NFFT - k]) / 2,   Xb[k] = (Z[k] - conj Z[NFFT - k]) / (2 i)
//      -> the two magnitude rows in LDS; energy = sqrt(sum |X|^2): wave butterflies, the 4 wave sums added in order.
//   3  mel row m = sum over the filter's support [k_lo, k_hi) only (host table from the basis it is given: zeros
//      inside contribute nothing, an empty support gives log(clip)); 16 lanes per mel row stride over the support
//      for both frames, a 4-step butterfly inside the 16 lanes; log(max(., clip)) with log(clip) from the host.
// LDS addressing (32 banks of 4 bytes for 32-bit accesses, conflicts inside a 32-lane half): the data and the twiddle
// tables are stored at i + (i >> 5), one pad word per 32.  The bit-reversed scatter of step 1 (32 consecutive i land
// NFFT / 32 words apart: one bank without the pad) and the twiddle reads of the middle stages (index j * 2^s: 16
// lanes on one bank at s = 5) become conflict-free; the butterfly reads of the stages with half < 32 stay 2-way.
// (By construction from the bank rule; no counter run has measured it.)
// Resources (hipcc -O3, gfx950; VGPRs / LDS bytes, no scratch): NFFT 512: 32 / 8432, 1024: 36 / 16816,
// 2048: 48 / 33584 (4 workgroups per CU by LDS).
// The pairing depends on the frame's index inside its utterance alone and a workgroup reads nothing but its own
// utterance: every utterance comes out bitwise as if alone.  fp32, no atomics, no scratch.
//
// interp_unvoiced_kernel: a workgroup per utterance; the nearest voiced (non-zero) frame at or before / at or after
// every frame from a forward max-scan and a backward min-scan over chunks of 256 frames with carries (wg_scan.h, which
// k_prosody.hip stage C uses too); the forward indices wait in the output row itself, so the length is not limited by LDS.
// 32 VGPRs, 16 LDS bytes, no scratch.
#include "common.h"
#include "gl_frames.h"
#include "wg_scan.h"

namespace {

constexpr int NT = 256;
constexpr int FF_TAB = 6;      // table words per workgroup
constexpr int MEL_LANES = 16;  // lanes per mel row in step 3

__device__ __forceinline__ int pad32(int i) { return i + (i >> 5); }

template <int NFFT>
__global__ void __launch_bounds__(NT) frame_features_kernel(const float* __restrict__ wav, const int* __restrict__ tab,
                                                            int hop, const float* __restrict__ window,
                                                            const float* __restrict__ basis,
                                                            const int2* __restrict__ supp, int n_mel, float clip,
                                                            float log_clip, int clip_wave, float* __restrict__ mel,
                                                            float* __restrict__ energy) {
  constexpr int NB = NFFT / 2 + 1;
  constexpr int LOG2 = __builtin_ctz(NFFT);
  __shared__ float re[NFFT + NFFT / 32], im[NFFT + NFFT / 32], cs[NFFT / 2 + NFFT / 64], sn[NFFT / 2 + NFFT / 64];
  __shared__ float mag[2][NB];
  __shared__ float red[2][NT / 64];
  const int tid = threadIdx.x;
  const int* e = tab + (long)FF_TAB * blockIdx.x;
  const long off = (long)(((unsigned long long)(unsigned)e[1] << 32) | (unsigned)e[0]);
  const int N = e[2], f0 = e[3], row = e[4], rows = e[5];
  const float* x = wav + off;
  for (int t = tid; t < NFFT / 2; t += NT) {
    float s, c;
    sincospif(2.f * (float)t / (float)NFFT, &s, &c);
    cs[pad32(t)] = c;
    sn[pad32(t)] = -s;  // forward transform: exp(-2 pi i t / NFFT)
  }
  // centre-padded frame f starts at sample f*hop - NFFT/2 (reflect padding, no edge repeat)
  const int qa = f0 * hop - NFFT / 2;
  constexpr int PER = NFFT / NT;
  float va[PER], vb[PER], sa = 0.f, sb = 0.f;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int i = tid + q * NT;
    const float w = window[i];
    float a = 0.f, b = 0.f;
    int s = gl_reflect(qa + i, N);
    if (s >= 0 && s < N) a = x[s];
    if (rows > 1) {
      s = gl_reflect(qa + hop + i, N);
      if (s >= 0 && s < N) b = x[s];
    }
    if (clip_wave) {
      a = fminf(fmaxf(a, -1.f), 1.f);
      b = fminf(fmaxf(b, -1.f), 1.f);
    }
    va[q] = a * w;
    vb[q] = b * w;
    sa += va[q] * va[q];
    sb += vb[q] * vb[q];
  }
  // A frame of exact zeros must come out as exact zeros (the split would leave it the other frame's rounding
  // noise): the frames' sums of squares, by a fixed-order block reduction.
  sa = wave_sum(sa);
  sb = wave_sum(sb);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = sa;
    red[1][tid >> 6] = sb;
  }
  __syncthreads();
  float pa = red[0][0], pb = red[1][0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) {
    pa += red[0][w];
    pb += red[1][w];
  }
  const float down_a = pa > 0.f ? 1.f : 0.f, down_b = pb > 0.f ? 1.f : 0.f;
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int r = pad32((int)(__brev((unsigned)(tid + q * NT)) >> (32 - LOG2)));
    re[r] = va[q];
    im[r] = vb[q];
  }
  __syncthreads();
#pragma unroll 1
  for (int lh = 0; lh < LOG2; ++lh) {
    const int half = 1 << lh;
    const int tstep = NFFT >> (lh + 1);  // twiddle index stride for span 2*half
    for (int k = tid; k < NFFT / 2; k += NT) {
      const int j = k & (half - 1);
      const int i0 = ((k >> lh) << (lh + 1)) + j;
      const int p0 = pad32(i0), p1 = pad32(i0 + half), pt = pad32(j * tstep);
      const float wr = cs[pt], wi = sn[pt];
      const float xr = re[p1] * wr - im[p1] * wi;
      const float xi = re[p1] * wi + im[p1] * wr;
      re[p1] = re[p0] - xr;
      im[p1] = im[p0] - xi;
      re[p0] += xr;
      im[p0] += xi;
    }
    __syncthreads();
  }
  float ea = 0.f, eb = 0.f;
  for (int k = tid; k < NB; k += NT) {
    const int pk = pad32(k), pn = pad32((NFFT - k) & (NFFT - 1));
    const float zr = re[pk], zi = im[pk], yr = re[pn], yi = im[pn];
    const float ar = 0.5f * (zr + yr), ai = 0.5f * (zi - yi);
    const float br = 0.5f * (zi + yi), bi = 0.5f * (yr - zr);
    const float m2a = ar * ar + ai * ai, m2b = br * br + bi * bi;
    mag[0][k] = sqrtf(m2a) * down_a;
    mag[1][k] = sqrtf(m2b) * down_b;
    ea += m2a;
    eb += m2b;
  }
  ea = wave_sum(ea);
  eb = wave_sum(eb);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = ea;
    red[1][tid >> 6] = eb;
  }
  __syncthreads();
  if (tid < 2 && tid < rows) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += red[tid][w];
    energy[(long)row + tid] = sqrtf(s) * (tid == 0 ? down_a : down_b);
  }
  const int lane = tid & (MEL_LANES - 1);
  for (int m = tid / MEL_LANES; m < n_mel; m += NT / MEL_LANES) {
    const int2 sp = supp[m];
    const int k_lo = sp.x < 0 ? 0 : sp.x, k_hi = sp.y > NB ? NB : sp.y;
    const float* brow = basis + (long)m * NB;
    float a = 0.f, b = 0.f;
    for (int k = k_lo + lane; k < k_hi; k += MEL_LANES) {
      const float w = brow[k];
      a += w * mag[0][k];
      b += w * mag[1][k];
    }
#pragma unroll
    for (int o = MEL_LANES / 2; o > 0; o >>= 1) {
      a += __shfl_xor(a, o, MEL_LANES);
      b += __shfl_xor(b, o, MEL_LANES);
    }
    if (lane == 0) {
      mel[(long)row * n_mel + m] = a > clip ? logf(a) : log_clip;
      if (rows > 1) mel[((long)row + 1) * n_mel + m] = b > clip ? logf(b) : log_clip;
    }
  }
}

__global__ void __launch_bounds__(WG_SCAN_THREADS) interp_unvoiced_kernel(const float* __restrict__ f0,
                                                                          const int* __restrict__ cu,
                                                                          float* __restrict__ out,
                                                                          int* __restrict__ n_voiced) {
  __shared__ int wtot[WG_SCAN_WAVES];
  const int p = blockIdx.x, t = threadIdx.x;
  const int y0 = cu[p], T = cu[p + 1] - y0;
  const float* fy = f0 + y0;
  float* g = out + y0;
  int* gi = reinterpret_cast<int*>(g);  // the forward scan's indices, then the contour
  int carry = -1, cnt = 0;
  for (int c0 = 0; c0 < T; c0 += WG_SCAN_THREADS) {
    const int j = c0 + t;
    const bool v = j < T && fy[j] != 0.f;
    cnt += v ? 1 : 0;
    int all;
    int s = block_scan(v ? j : -1, OpMax(), wtot, all);
    s = s > carry ? s : carry;
    if (j < T) gi[j] = s;
    carry = all > carry ? all : carry;
  }
  int nv;
  block_scan(cnt, OpAdd(), wtot, nv);
  __syncthreads();  // the backward scan reads indices other threads wrote
  carry = WG_SCAN_NONE;
  for (int c0 = 0; c0 < T; c0 += WG_SCAN_THREADS) {
    const int j = T - 1 - (c0 + t);
    int all;
    int b = block_scan((j >= 0 && fy[j] != 0.f) ? j : WG_SCAN_NONE, OpMin(), wtot, all);
    b = b < carry ? b : carry;
    carry = all < carry ? all : carry;
    if (j >= 0) {
      const int a = gi[j];
      float gv = fy[j];
      if (gv == 0.f && nv > 0) gv = interp_voiced_rn(fy, j, a, b);
      g[j] = gv;
    }
  }
  if (t == 0) n_voiced[p] = nv;
}

}  // namespace

// wav: the packed samples; tab [G, 6] int32 {sample offset lo, hi, N, first frame, output row, rows (1 | 2)} per
// workgroup; window [n_fft]; basis [n_mel, n_fft/2+1]; supp [n_mel, 2] int32 {k_lo, k_hi}
// -> mel [R, n_mel] (log, clamp at `clip`, log_clip = log(clip) as the host rounds it), energy [R]
SSAMD_API int ssamd_frame_features(const float* wav, const int* tab, int G, int n_fft, int hop, const float* window,
                                   const float* basis, const int* supp, int n_mel, float clip, float log_clip,
                                   int clip_wave, float* mel, float* energy, hipStream_t s) {
  if (G < 0 || hop <= 0 || n_mel < 0) return -2;
  if (G == 0) return 0;
  if (!wav || !tab || !window || !basis || !supp || !mel || !energy) return -2;
  const int2* sp = reinterpret_cast<const int2*>(supp);
  switch (n_fft) {
    case 512:
      hipLaunchKernelGGL(frame_features_kernel<512>, dim3(G), dim3(NT), 0, s, wav, tab, hop, window, basis, sp, n_mel,
                         clip, log_clip, clip_wave, mel, energy);
      break;
    case 1024:
      hipLaunchKernelGGL(frame_features_kernel<1024>, dim3(G), dim3(NT), 0, s, wav, tab, hop, window, basis, sp, n_mel,
                         clip, log_clip, clip_wave, mel, energy);
      break;
    case 2048:
      hipLaunchKernelGGL(frame_features_kernel<2048>, dim3(G), dim3(NT), 0, s, wav, tab, hop, window, basis, sp, n_mel,
                         clip, log_clip, clip_wave, mel, energy);
      break;
    default:
      return -2;
  }
  return (int)hipGetLastError();
}

// f0 [R] packed contours, cu [P + 1] int32 row offsets -> out [R] (must not alias f0), n_voiced [P] int32
SSAMD_API int ssamd_interp_unvoiced(const float* f0, const int* cu, int P, float* out, int* n_voiced, hipStream_t s) {
  if (P <= 0) return 0;
  if (!f0 || !cu || !out || !n_voiced || f0 == out) return -2;
  hipLaunchKernelGGL(interp_unvoiced_kernel, dim3(P), dim3(WG_SCAN_THREADS), 0, s, f0, cu, out, n_voiced);
  return (int)hipGetLastError();
}

// Alignment learning (speakingstyle_amd/models/aligner.py): forward-sum loss and monotonic alignment search over
// the T x N lattice of a padded batch lp [B, Tmax, Nmax] (frames t < T_b, tokens n < N_b, 1 <= N_b <= T_b).
//
//   alpha(0, 0) = lp(0, 0), alpha(0, n > 0) = -inf
//   alpha(t, n) = lp(t, n) + logaddexp(alpha(t-1, n), alpha(t-1, n-1))                nll = -alpha(T-1, N-1)
//   beta(T-1, N-1) = 0,  beta(t, n) = logaddexp(lp(t+1, n) + beta(t+1, n), lp(t+1, n+1) + beta(t+1, n+1))
//   d nll / d lp(t, n) = -exp(alpha(t, n) + beta(t, n) - alpha(T-1, N-1))
//   MAS: max in place of logaddexp; stay wins a tie, advance only on strict >
//
// align_fwd (sum and max forms of one template): one workgroup per utterance, wave w owns tokens 64 w .. 64 w + 63,
// one per lane.  alpha(t-1, n-1) is the neighbouring lane's value (one DPP shift); the token below a wave's first
// lane comes from the previous wave through an LDS ring of 2 x 64 frames: wave w runs one block of 64 frames behind
// wave w - 1 (tick k: wave w sweeps block k - w), one barrier per tick, T/64 + W - 1 ticks.  The lp rows of the next
// 16 frames are in flight in registers while 16 frames are computed (a lane per token: coalesced rows).  The sum
// form writes the alpha plane for the backward; the max form keeps one __ballot word per (frame, wave) -- the
// advance bits -- and stores a block's 64 words with one wave store: plane [W][Tpad] of 64-bit words per utterance.
//
// align_fsum_bwd: the mirror image: t descending, lp + beta of the next token from lane + 1, the first lane of
// wave w + 1 through the ring, wave w one block behind wave w + 1.  It writes the utterance's whole [Tmax, Nmax]
// gradient slab (zeros outside the lattice), scaled by the incoming gradient of nll.
//
// align_mas_path: one wave per utterance walks the advance plane back from (T-1, N-1) in chunks of 64 frames loaded
// into LDS, counting frames per token.  segment_mean: one wave per utterance, prefix sum of the durations, a lane
// per token adds its run of frames in order.
//
// No atomics, no scratch, fixed order: an utterance's result depends on nothing but its own cells.
#include "common.h"

namespace {

constexpr int AL_BLOCK = 64;   // frames per block (one tick of a wave)
constexpr int AL_MAX_W = 16;   // waves per workgroup: Nmax <= 1024
constexpr int AL_PF = 16;      // frames of lp in flight per lane

__device__ __forceinline__ float al_lane_shr1(float v, float self) {  // value of lane l - 1; lane 0 gets `self`
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(self), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float al_lane_shl1(float v, float self) {  // value of lane l + 1; lane 63 gets `self`
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(self), __float_as_int(v), 0x130, 0xf, 0xf, false));
}
__device__ __forceinline__ float al_read_lane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// max + log1p(exp(-|d|)) with the hardware exp2 / log2 (v_exp_f32 / v_log_f32; the argument of the log is in [1, 2],
// no denormal handling needed); -inf when both are -inf.  exp(-|d|) <= 1, so log(1 + e) loses at most 2^-24 absolute
// against log1p -- below the rounding of the sum with max.
__device__ __forceinline__ float al_logaddexp(float x, float y) {
  const float m = fmaxf(x, y);
  const float e = __builtin_amdgcn_exp2f(-1.44269504088896341f * fabsf(x - y));
  const float r = m + 0.69314718055994531f * __builtin_amdgcn_logf(1.f + e);
  return m == -__builtin_inff() ? m : r;
}

// Utterance b's lengths if they fit the launch (the host rejects everything else; never false there).
__device__ __forceinline__ bool al_lens(const int* t_lens, const int* n_lens, int b, int Tmax, int Nmax, int W, int& T,
                                        int& N) {
  T = __builtin_amdgcn_readfirstlane(t_lens[b]);  // wave-uniform: the frame loop's control flow stays scalar
  N = __builtin_amdgcn_readfirstlane(n_lens[b]);
  return N >= 1 && N <= T && T <= Tmax && N <= Nmax && N <= 64 * W;
}

template <bool MAS>
__global__ __launch_bounds__(AL_MAX_W * 64) void align_fwd_kernel(const float* __restrict__ lp,
                                                                   const int* __restrict__ t_lens,
                                                                   const int* __restrict__ n_lens, int Tmax, int Nmax,
                                                                   float* __restrict__ alpha, float* __restrict__ nll,
                                                                   unsigned long long* __restrict__ plane, int Tpad) {
  __shared__ float edge[AL_MAX_W][2][AL_BLOCK];  // [wave][block parity][frame]: the wave's lane-63 value
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  int T, N;
  if (!al_lens(t_lens, n_lens, b, Tmax, Nmax, W, T, N)) return;  // uniform over the workgroup
  const int Wb = (N + 63) >> 6, nblk = (T + AL_BLOCK - 1) / AL_BLOCK;
  const int n = wave * 64 + lane;
  const bool tok = n < N;
  const float NINF = -__builtin_inff();
  const long cell0 = (long)b * Tmax * Nmax + n;  // dereferenced only where tok
  float a = NINF;      // alpha(t - 1, n)
  float carry = NINF;  // alpha(t0 - 1, 64 wave - 1): the last frame of the previous block of the wave below
  for (int k = 0; k < nblk + Wb - 1; ++k) {
    const int blk = k - wave;
    if (wave < Wb && blk >= 0 && blk < nblk) {
      const int t0 = blk * AL_BLOCK;
      const int nu = min(AL_BLOCK, T - t0);
      const float hin = wave > 0 ? edge[wave - 1][blk & 1][lane] : NINF;  // lane u: alpha(t0 + u, 64 wave - 1)
      float hout = NINF;
      unsigned long long word = 0;
      float cur[AL_PF], nxt[AL_PF], out[AL_PF];  // out: the chunk's alpha, stored together after its 16 steps
#pragma unroll
      for (int i = 0; i < AL_PF; ++i) cur[i] = (tok && i < nu) ? lp[cell0 + (long)(t0 + i) * Nmax] : NINF;
#pragma unroll 1
      for (int q = 0; q * AL_PF < nu; ++q) {
#pragma unroll
        for (int i = 0; i < AL_PF; ++i) {
          const int u = (q + 1) * AL_PF + i;
          nxt[i] = (tok && u < nu) ? lp[cell0 + (long)(t0 + u) * Nmax] : NINF;
        }
#pragma unroll
        for (int i = 0; i < AL_PF; ++i) {
          const int u = q * AL_PF + i;
          if (u < nu) {  // uniform
            const int t = t0 + u;
            const float below = u == 0 ? carry : al_read_lane(hin, u > 0 ? u - 1 : 0);
            const float move = al_lane_shr1(a, below);
            float in;
            if (MAS) {
              const bool go = t > 0 && move > a;
              in = go ? move : a;
              const unsigned long long bits = __ballot(go && tok);
              if (lane == u) word = bits;
            } else {
              in = al_logaddexp(a, move);
            }
            if (t == 0) in = n == 0 ? 0.f : NINF;
            a = cur[i] + in;
            out[i] = a;
            const float last = al_read_lane(a, 63);
            if (lane == u) hout = last;
          }
        }
        if (!MAS && tok) {
#pragma unroll
          for (int i = 0; i < AL_PF; ++i) {
            const int u = q * AL_PF + i;
            if (u < nu) alpha[cell0 + (long)(t0 + u) * Nmax] = out[i];
          }
        }
#pragma unroll
        for (int i = 0; i < AL_PF; ++i) cur[i] = nxt[i];
      }
      carry = al_read_lane(hin, 63);
      edge[wave][blk & 1][lane] = hout;
      if (MAS && lane < nu) plane[((long)b * W + wave) * Tpad + t0 + lane] = word;
    }
    __syncthreads();
  }
  if (tok && n == N - 1) nll[b] = -a;
}

__global__ __launch_bounds__(AL_MAX_W * 64) void align_fsum_bwd_kernel(const float* __restrict__ lp,
                                                                        const float* __restrict__ alpha,
                                                                        const float* __restrict__ nll,
                                                                        const float* __restrict__ gnll,
                                                                        const int* __restrict__ t_lens,
                                                                        const int* __restrict__ n_lens, int Tmax,
                                                                        int Nmax, float* __restrict__ grad) {
  __shared__ float edge[AL_MAX_W][2][AL_BLOCK];  // [wave][block parity][frame]: the wave's lane-0 lp + beta
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, W = blockDim.x >> 6;
  const long slab = (long)b * Tmax * Nmax;
  int T, N;
  if (!al_lens(t_lens, n_lens, b, Tmax, Nmax, W, T, N)) return;  // uniform over the workgroup
  const int Wb = (N + 63) >> 6, nblk = (T + AL_BLOCK - 1) / AL_BLOCK;
  const int ncov = min(64 * Wb, Nmax);  // the sweep writes the cells t < T, n < ncov; the rest is zeroed here
  for (int t = 0; t < Tmax; ++t)
    for (int nn = (t < T ? ncov : 0) + (int)threadIdx.x; nn < Nmax; nn += blockDim.x) grad[slab + (long)t * Nmax + nn] = 0.f;
  const int n = wave * 64 + lane;
  const bool tok = n < N;
  const float NINF = -__builtin_inff();
  const long cell0 = slab + n;  // dereferenced only where n < ncov
  const float end = -nll[b], gs = gnll[b];
  float g = NINF;      // lp(t + 1, n) + beta(t + 1, n)
  float carry = NINF;  // the same of token 64 (wave + 1) at frame t0 + 64
  for (int k = 0; k < nblk + Wb - 1; ++k) {
    const int j = k - (Wb - 1 - wave);
    const int blk = nblk - 1 - j;
    if (wave < Wb && j >= 0 && j < nblk) {
      const int t0 = blk * AL_BLOCK;
      const int nu = min(AL_BLOCK, T - t0);
      const float hin = wave + 1 < Wb ? edge[wave + 1][blk & 1][lane] : NINF;  // lane u: (lp + beta)(t0 + u, 64 (wave + 1))
      float hout = NINF;
#pragma unroll 1
      for (int q = AL_BLOCK / AL_PF - 1; q >= 0; --q) {
        if (q * AL_PF >= nu) continue;  // uniform
        float lpr[AL_PF], alr[AL_PF], out[AL_PF];  // out: the chunk's gradient, stored together after its 16 steps
#pragma unroll
        for (int i = 0; i < AL_PF; ++i) {
          const int u = q * AL_PF + i;
          const bool ok = tok && u < nu;
          lpr[i] = ok ? lp[cell0 + (long)(t0 + u) * Nmax] : NINF;
          alr[i] = ok ? alpha[cell0 + (long)(t0 + u) * Nmax] : NINF;
        }
#pragma unroll
        for (int i = AL_PF - 1; i >= 0; --i) {
          const int u = q * AL_PF + i;
          if (u < nu) {  // uniform
            const int t = t0 + u;
            const float above = u == AL_BLOCK - 1 ? carry : al_read_lane(hin, u < AL_BLOCK - 1 ? u + 1 : 0);
            const float gn = al_lane_shl1(g, above);
            float beta = al_logaddexp(g, gn);
            if (t == T - 1) beta = n == N - 1 ? 0.f : NINF;
            g = lpr[i] + beta;
            const float post = tok ? __expf(alr[i] + beta - end) : 0.f;
            out[i] = -gs * post;
            const float first = al_read_lane(g, 0);
            if (lane == u) hout = first;
          }
        }
        if (n < ncov) {
#pragma unroll
          for (int i = 0; i < AL_PF; ++i) {
            const int u = q * AL_PF + i;
            if (u < nu) grad[cell0 + (long)(t0 + u) * Nmax] = out[i];
          }
        }
      }
      carry = al_read_lane(hin, 0);
      edge[wave][blk & 1][lane] = hout;
    }
    __syncthreads();
  }
}

// one wave per utterance: walk the advance plane back from (T - 1, N - 1)
__global__ __launch_bounds__(64) void align_mas_path_kernel(const unsigned long long* __restrict__ plane, int W,
                                                            int Tpad, const int* __restrict__ t_lens,
                                                            const int* __restrict__ n_lens, int Tmax, int Nmax,
                                                            int* __restrict__ dur) {
  __shared__ unsigned long long chunk[AL_MAX_W][AL_BLOCK];
  __shared__ int count[AL_MAX_W * 64];
  __shared__ int state;
  const int b = blockIdx.x, lane = threadIdx.x;
  int T, N;
  if (!al_lens(t_lens, n_lens, b, Tmax, Nmax, W, T, N)) {  // rejected on the host; never reached
    for (int i = lane; i < Nmax; i += 64) dur[(long)b * Nmax + i] = 0;
    return;
  }
  const int Wb = (N + 63) >> 6, nblk = (T + AL_BLOCK - 1) / AL_BLOCK;
  for (int i = lane; i < AL_MAX_W * 64; i += 64) count[i] = 0;
  int n = N - 1;
  for (int blk = nblk - 1; blk >= 0; --blk) {
    const int t0 = blk * AL_BLOCK;
    const int nu = min(AL_BLOCK, T - t0);
    for (int w = 0; w < Wb; ++w) chunk[w][lane] = lane < nu ? plane[((long)b * W + w) * Tpad + t0 + lane] : 0ull;
    __syncthreads();
    if (lane == 0) {
      // n stays in [0, N - 1]: it only falls, and token 0 never has its advance bit set
      for (int u = nu - 1; u >= 0; --u) {
        count[n] += 1;
        if (t0 + u > 0 && n > 0 && ((chunk[n >> 6][u] >> (n & 63)) & 1ull)) --n;
      }
      state = n;
    }
    __syncthreads();
    n = state;
    __syncthreads();
  }
  for (int i = lane; i < Nmax; i += 64) dur[(long)b * Nmax + i] = i < N ? count[i] : 0;
}

// one wave per utterance: out[b, n] = mean(values[b, start_n .. start_n + d_n - 1]), start_n = sum(d[:n])
__global__ __launch_bounds__(64) void segment_mean_kernel(const float* __restrict__ values, const int* __restrict__ dur,
                                                          int Tmax, int Nmax, float* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* v = values + (long)b * Tmax;
  long base = 0;
  for (int n0 = 0; n0 < Nmax; n0 += 64) {
    const int n = n0 + lane;
    const int d = n < Nmax ? max(dur[(long)b * Nmax + n], 0) : 0;
    long s = d;  // inclusive prefix sum over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int lo = __shfl_up((int)(s & 0xffffffffll), o, 64);
      const int hi = __shfl_up((int)(s >> 32), o, 64);
      if (lane >= o) s += ((long)hi << 32) | (unsigned int)lo;
    }
    const long start = base + s - d;
    const int cnt = start < Tmax ? (int)min((long)d, (long)Tmax - start) : 0;  // frames inside the row
    float acc = 0.f;
    for (int i = 0; i < cnt; ++i) acc += v[start + i];
    if (n < Nmax) out[(long)b * Nmax + n] = d > 0 ? acc / (float)d : 0.f;
    const int tlo = __shfl((int)(s & 0xffffffffll), 63, 64), thi = __shfl((int)(s >> 32), 63, 64);
    base += ((long)thi << 32) | (unsigned int)tlo;
  }
}

inline bool al_shape_ok(int B, int Tmax, int Nmax, int W) {
  return B >= 0 && Tmax >= 1 && Nmax >= 1 && Nmax <= AL_MAX_W * 64 && W >= 1 && W <= AL_MAX_W;
}

}  // namespace

// lp [B, Tmax, Nmax] fp32, t_lens / n_lens [B] int32; W waves per workgroup (64 W >= every N_b).
// Writes alpha [B, Tmax, Nmax] on the lattice cells and nll [B].
SSAMD_API int ssamd_align_fsum_fwd(const float* lp, const int* t_lens, const int* n_lens, int B, int Tmax, int Nmax,
                                   int W, float* alpha, float* nll, hipStream_t s) {
  if (!al_shape_ok(B, Tmax, Nmax, W)) return -2;
  if (B == 0) return 0;
  if (!lp || !t_lens || !n_lens || !alpha || !nll) return -2;
  hipLaunchKernelGGL(align_fwd_kernel<false>, dim3(B), dim3(64 * W), 0, s, lp, t_lens, n_lens, Tmax, Nmax, alpha, nll,
                     (unsigned long long*)nullptr, 0);
  return (int)hipGetLastError();
}

// grad [B, Tmax, Nmax] = gnll[b] * d nll_b / d lp, every cell written (0 outside the lattice)
SSAMD_API int ssamd_align_fsum_bwd(const float* lp, const float* alpha, const float* nll, const float* gnll,
                                   const int* t_lens, const int* n_lens, int B, int Tmax, int Nmax, int W, float* grad,
                                   hipStream_t s) {
  if (!al_shape_ok(B, Tmax, Nmax, W)) return -2;
  if (B == 0) return 0;
  if (!lp || !alpha || !nll || !gnll || !t_lens || !n_lens || !grad) return -2;
  hipLaunchKernelGGL(align_fsum_bwd_kernel, dim3(B), dim3(64 * W), 0, s, lp, alpha, nll, gnll, t_lens, n_lens, Tmax,
                     Nmax, grad);
  return (int)hipGetLastError();
}

// 64-bit words of the advance plane of a batch: [B][W][Tpad], Tpad = Tmax rounded up to the block
SSAMD_API long ssamd_align_mas_plane_words(int B, int Tmax, int W) {
  return (long)B * W * ((Tmax + AL_BLOCK - 1) / AL_BLOCK * AL_BLOCK);
}

// durations [B, Nmax] int32 of the best path; score [B] = minus its total; plane: ssamd_align_mas_plane_words words
SSAMD_API int ssamd_align_mas(const float* lp, const int* t_lens, const int* n_lens, int B, int Tmax, int Nmax, int W,
                              unsigned long long* plane, float* score, int* dur, hipStream_t s) {
  if (!al_shape_ok(B, Tmax, Nmax, W)) return -2;
  if (B == 0) return 0;
  if (!lp || !t_lens || !n_lens || !plane || !score || !dur) return -2;
  const int Tpad = (Tmax + AL_BLOCK - 1) / AL_BLOCK * AL_BLOCK;
  hipLaunchKernelGGL(align_fwd_kernel<true>, dim3(B), dim3(64 * W), 0, s, lp, t_lens, n_lens, Tmax, Nmax,
                     (float*)nullptr, score, plane, Tpad);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(align_mas_path_kernel, dim3(B), dim3(64), 0, s, plane, W, Tpad, t_lens, n_lens, Tmax, Nmax, dur);
  return (int)hipGetLastError();
}

// values [B, Tmax] fp32, dur [B, Nmax] int32 -> out [B, Nmax] fp32
SSAMD_API int ssamd_segment_mean(const float* values, const int* dur, int B, int Tmax, int Nmax, float* out,
                                 hipStream_t s) {
  if (B < 0 || Tmax < 0 || Nmax < 0) return -2;
  if (B == 0 || Nmax == 0) return 0;
  if (!values && Tmax > 0) return -2;
  if (!dur || !out) return -2;
  hipLaunchKernelGGL(segment_mean_kernel, dim3(B), dim3(64), 0, s, values, dur, Tmax, Nmax, out);
  return (int)hipGetLastError();
}

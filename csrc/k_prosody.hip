// Prosody transfer (speakingstyle_amd/infer/transfer.py): a DTW path between a synthesis (frames i) and a recording
// (frames j) plus the recording's F0 / energy contours -> the per-token durations, pitch and energy the variance
// adaptor was trained on.  Semantics: ops/reference.py::prosody_transfer.
//
//   owner(j) = (i_lo + i_hi) >> 1 over the run of path cells of recorded frame j
//   token(j) = #{n : cumsum(src_dur)[n] <= min(owner(j), sum(src_dur) - 1)}          (non-decreasing in j)
//   rec_dur[n] = #{j : token(j) = n};  g = F0 with the unvoiced frames interpolated in Hz, ends held
//   relative mode: g *= exp(L_pred - L_ref), L_ref = mean_j ln g[j], L_pred = src_dur-weighted mean of
//                  ln max(pred_pitch std + mean, 1)
//   pitch[n] = (mean of g over the token's frames - mean) / std, energy[n] likewise, voiced[n] = share of f0 > 0
//
// prosody_transfer_kernel: one workgroup of 4 waves per utterance, one launch for the batch.
//   A  the duration prefix sums of up to 1024 tokens go to LDS (4 consecutive tokens per thread + a block scan);
//      the same pass collects the terms of L_pred.
//   B  every path cell is compared with its two neighbours: the first cell of a run of equal j writes i_lo[j], the
//      last one i_hi[j] (the utterance's slice of the workspace).  Then a thread per frame finds token(j) and
//      token(j - 1) by a 10-step search over the prefix sums in LDS; where they differ a token's frame range starts
//      and the previous one's ends (LDS, one writer each because token is monotone).
//   C  the nearest voiced frame at or before j: a max-scan over chunks of 256 frames with a carry; the nearest at or
//      after j: the same as a min-scan from the end.  The second scan writes g[j] to the workspace and adds ln g[j]
//      to the thread's accumulator (hardware log2).  Neither the path nor y is held in LDS: their lengths are not
//      limited by it.
//   D  a thread per token runs over the token's own frames in increasing j: one accumulator each for g, the energy
//      and the voiced count.
// L_ref / L_pred: per-thread partial sums in a fixed order, a butterfly inside the wave, the 4 wave sums added in
// order.  fp32, no atomics, no scratch; an utterance reads nothing but its own rows: bitwise what it is alone.
#include "common.h"
#include "wg_scan.h"

namespace {

constexpr int PROS_THREADS = WG_SCAN_THREADS;  // block_scan / block_sum (wg_scan.h) are written for this size
constexpr int PROS_WAVES = WG_SCAN_WAVES;
constexpr int PROS_MAX_N = 1024;             // tokens per utterance: PROS_PER_THREAD per thread
constexpr int PROS_PER_THREAD = PROS_MAX_N / PROS_THREADS;
constexpr int PROS_WS_WORDS = 3;             // workspace words per recorded frame: i_lo, i_hi, g
constexpr int PROS_NONE = WG_SCAN_NONE;
constexpr float PROS_LN2 = 0.6931471805599453f;
constexpr float PROS_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float ln_hw(float x) { return __builtin_amdgcn_logf(x) * PROS_LN2; }  // v_log_f32

// #{n : ends[n] <= key} over the PROS_MAX_N prefix sums (entries past the last token hold the total); key < total
__device__ __forceinline__ int count_le(const int* ends, int key) {
  int pos = 0;
#pragma unroll
  for (int s = PROS_MAX_N / 2; s > 0; s >>= 1)
    if (ends[pos + s - 1] <= key) pos += s;
  return pos;
}

__global__ __launch_bounds__(PROS_THREADS) void prosody_transfer_kernel(
    const int2* __restrict__ path, const int* __restrict__ path_len, int Lmax, const int* __restrict__ src_dur,
    const int* __restrict__ src_lens, const float* __restrict__ pred_pitch, int Nmax, const int* __restrict__ cu_y,
    const float* __restrict__ f0, const float* __restrict__ energy, float p_mean, float p_std, float e_mean,
    float e_std, int relative, int* ws, int* __restrict__ rec_dur, float* __restrict__ pitch,
    float* __restrict__ energy_out, float* __restrict__ voiced, uint8_t* __restrict__ pitch_ok) {
  __shared__ int ends[PROS_MAX_N];    // inclusive prefix sums of the durations
  __shared__ int tstart[PROS_MAX_N];  // first recorded frame of a token
  __shared__ int tend[PROS_MAX_N];    // one past its last
  __shared__ int wtot[PROS_WAVES];
  __shared__ float ftot[PROS_WAVES];
  const int p = blockIdx.x, t = threadIdx.x;
  const int y0 = cu_y[p], Ty = cu_y[p + 1] - y0;
  int N = src_lens[p];
  N = N < 0 ? 0 : (N > Nmax ? Nmax : N);
  int L = path_len[p];
  L = L < 0 ? 0 : (L > Lmax ? Lmax : L);
  const int2* cells = path + (long)p * Lmax;
  const int* dur = src_dur + (long)p * Nmax;
  const float* pred = pred_pitch + (long)p * Nmax;
  const float* fy = f0 + y0;
  const float* ey = energy + y0;
  int* lo = ws + (long)PROS_WS_WORDS * y0;  // the utterance's slice: [Ty] i_lo, [Ty] i_hi, [Ty] g
  int* hi = lo + Ty;
  int* gi = hi + Ty;                        // the forward scan's indices, then g as floats
  float* g = reinterpret_cast<float*>(gi);

  // ---- A: prefix sums of the durations, the terms of L_pred
  int d[PROS_PER_THREAD], local = 0;
  float lw = 0.f;
#pragma unroll
  for (int q = 0; q < PROS_PER_THREAD; ++q) {
    const int n = PROS_PER_THREAD * t + q;
    int v = n < N ? dur[n] : 0;
    v = v < 0 ? 0 : v;
    d[q] = v;
    local += v;
    if (v > 0) lw += (float)v * ln_hw(fmaxf(pred[n] * p_std + p_mean, 1.f));
  }
  int total;
  int run = block_scan(local, OpAdd(), wtot, total) - local;
#pragma unroll
  for (int q = 0; q < PROS_PER_THREAD; ++q) {
    const int n = PROS_PER_THREAD * t + q;
    run += d[q];
    ends[n] = run;
    tstart[n] = 0;
    tend[n] = 0;
  }
  const float sum_pred = block_sum(lw, ftot);

  // ---- B: runs of equal j -> i_lo / i_hi; then the frame range of every token
  for (int k = t; k < L; k += PROS_THREADS) {
    const int2 c = cells[k];
    if (c.y < 0 || c.y >= Ty) continue;  // not a cell of this utterance: never written by ops.dtw
    const int jp = k > 0 ? cells[k - 1].y : -1;
    const int jn = k + 1 < L ? cells[k + 1].y : -1;
    if (c.y != jp) lo[c.y] = c.x;
    if (c.y != jn) hi[c.y] = c.x;
  }
  __syncthreads();  // ends / tstart / tend and the workgroup's i_lo / i_hi are complete
  if (total > 0) {
    for (int j = t; j < Ty; j += PROS_THREADS) {
      const int oj = (lo[j] + hi[j]) >> 1;
      const int tj = count_le(ends, oj < 0 ? 0 : (oj < total ? oj : total - 1));
      int tp = -1;
      if (j > 0) {
        const int op = (lo[j - 1] + hi[j - 1]) >> 1;
        tp = count_le(ends, op < 0 ? 0 : (op < total ? op : total - 1));
      }
      if (tj != tp) {
        tstart[tj] = j;
        if (tp >= 0) tend[tp] = j;
      }
      if (j == Ty - 1) tend[tj] = Ty;
    }
  }

  // ---- C: nearest voiced frame on either side, g and sum ln g
  int carry = -1;
  for (int c0 = 0; c0 < Ty; c0 += PROS_THREADS) {
    const int j = c0 + t;
    int all;
    int s = block_scan((j < Ty && fy[j] > 0.f) ? j : -1, OpMax(), wtot, all);
    s = s > carry ? s : carry;
    if (j < Ty) gi[j] = s;
    carry = all > carry ? all : carry;
  }
  const bool any_voiced = carry >= 0;
  __syncthreads();  // the backward scan reads indices other threads wrote
  carry = PROS_NONE;
  float lsum = 0.f;
  for (int c0 = 0; c0 < Ty; c0 += PROS_THREADS) {
    const int j = Ty - 1 - (c0 + t);
    int all;
    int b = block_scan((j >= 0 && fy[j] > 0.f) ? j : PROS_NONE, OpMin(), wtot, all);
    b = b < carry ? b : carry;
    carry = all < carry ? all : carry;
    if (j >= 0) {
      const int a = gi[j];
      float gv = fy[j];
      if (!(gv > 0.f) && any_voiced) {
        if (a < 0) gv = fy[b];
        else if (b == PROS_NONE) gv = fy[a];
        else gv = (fy[b] - fy[a]) / (float)(b - a) * (float)(j - a) + fy[a];
      }
      g[j] = gv;
      if (gv > 0.f) lsum += ln_hw(gv);
    }
  }
  const float sum_ref = block_sum(lsum, ftot);  // its barriers also publish g, tstart and tend
  float scale = 1.f;
  if (relative && any_voiced && total > 0 && Ty > 0)
    scale = __builtin_amdgcn_exp2f((sum_pred / (float)total - sum_ref / (float)Ty) * PROS_LOG2E);  // v_exp_f32

  // ---- D: every token's sums over its own frames, in increasing j
  for (int n = t; n < Nmax; n += PROS_THREADS) {
    const int a = tstart[n], b = tend[n];
    const int cnt = b > a ? b - a : 0;
    float sp = 0.f, se = 0.f;
    int nv = 0;
    for (int j = a; j < b; ++j) {
      sp += g[j] * scale;
      se += ey[j];
      nv += fy[j] > 0.f ? 1 : 0;
    }
    const long o = (long)p * Nmax + n;
    const float c = (float)(cnt > 0 ? cnt : 1);
    rec_dur[o] = cnt;
    pitch[o] = cnt > 0 ? (sp / c - p_mean) / p_std : 0.f;
    energy_out[o] = cnt > 0 ? (se / c - e_mean) / e_std : 0.f;
    voiced[o] = cnt > 0 ? (float)nv / c : 0.f;
  }
  if (t == 0) pitch_ok[p] = any_voiced ? 1 : 0;
}

}  // namespace

// workspace words (4 bytes) of a batch whose recordings have Ry frames in all
SSAMD_API long ssamd_prosody_ws_words(long Ry) { return Ry > 0 ? (long)PROS_WS_WORDS * Ry : 0; }

// path [P, Lmax, 2] / path_len [P] as dtw writes them; src_dur / pred_pitch [P, Nmax], src_lens [P]; cu_y [P + 1]
// offsets of the utterances in the packed f0 / energy [Ry]; ws: ssamd_prosody_ws_words(Ry) words.
// Writes rec_dur int32 / pitch / energy_out / voiced fp32 [P, Nmax] and pitch_ok [P] bytes.
SSAMD_API int ssamd_prosody_transfer(const int* path, const int* path_len, int Lmax, const int* src_dur,
                                     const int* src_lens, const float* pred_pitch, int Nmax, const int* cu_y,
                                     const float* f0, const float* energy, int P, float p_mean, float p_std,
                                     float e_mean, float e_std, int relative, int* ws, int* rec_dur, float* pitch,
                                     float* energy_out, float* voiced, uint8_t* pitch_ok, hipStream_t s) {
  if (P <= 0) return 0;
  if (Nmax < 1 || Nmax > PROS_MAX_N || Lmax < 1) return -2;
  if (!path || !path_len || !src_dur || !src_lens || !pred_pitch || !cu_y || !f0 || !energy || !ws || !rec_dur ||
      !pitch || !energy_out || !voiced || !pitch_ok)
    return -2;
  hipLaunchKernelGGL(prosody_transfer_kernel, dim3(P), dim3(PROS_THREADS), 0, s, reinterpret_cast<const int2*>(path),
                     path_len, Lmax, src_dur, src_lens, pred_pitch, Nmax, cu_y, f0, energy, p_mean, p_std, e_mean,
                     e_std, relative, ws, rec_dur, pitch, energy_out, voiced, pitch_ok);
  return (int)hipGetLastError();
}

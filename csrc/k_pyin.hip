// Probabilistic YIN (Mauch & Dixon 2014) on the cmnd plane of k_pitch.hip (semantics: ops.reference.pyin_obs /
// ops.reference.pyin_decode).
//
// pyin_obs_kernel: a wave per packed frame row, four rows per workgroup.  The row sits in LDS; a lane owns 16
// consecutive lags, flags its troughs (cmnd[t] < cmnd[t - 1], cmnd[t] <= cmnd[t + 1], t in [tau_min, tau_max - 1]) and
// takes the smallest cmnd among them; an exclusive prefix minimum over the lanes (lag order, 2 at the start) gives the
// lowest earlier trough m.  A trough below m is YIN's pick for every threshold in (cmnd[t], m]: with the threshold
// distributed as Beta(2, 18) it weighs S(cmnd[t]) - S(m), S(x) = (1 - x)^18 (1 + 18 x) the tail of the distribution
// (the difference of two CDF values, taken where it does not cancel).  The lanes that own such troughs interpolate
// them as YIN does and append {bin, weight} to a list in LDS at positions from a prefix sum of their counts, i.e. in
// lag order; one lane adds the list into the row's bins in that order (the lowest trough, the last of the list, also
// takes no_trough_prob * (1 - S)), and the wave writes the whole row, zeros included.
//
// pyin_viterbi_kernel: a workgroup per utterance decodes the HMM of 2 NB states (voiced bin b, unvoiced bin b).  The
// two score vectors live in LDS with 64 cells of -inf on both sides, double-buffered.  A thread owns B (2 or 4)
// consecutive bins in both chains and walks the band of 2 h + 1 predecessors in steps of B cells: one aligned vector
// read per chain and one broadcast read of the log-triangle table per B^2 candidates of each chain, the table entries
// on a sliding register window (entry o - 1 of bin k + 1 is entry o of bin k).  Candidates are visited in increasing bin
// order and replace the best only when greater, so the lowest predecessor wins ties; staying in the voicing wins over
// switching.  The maximum of frame t - 1 is subtracted as frame t reads the scores (the wave maxima travel with the
// frame's one barrier), so the scores are exactly those of a per-frame renormalisation.  One byte per state and frame
// (band offset 0 .. 2 h, bit 7 = the voicing switched) goes to the utterance's plane in the workspace, B bytes per
// thread and store.  After the last frame the workgroup takes the best final state (voiced first, then the lowest bin)
// and one lane walks the plane back and writes f0.  fp32, no atomics, no scratch; an utterance's result depends on
// its own rows alone.
#include "common.h"

namespace {

constexpr int PO_WAVES = 4;      // rows per workgroup of pyin_obs_kernel
constexpr int PO_LAGS = 16;      // consecutive lags per lane: 64 * 16 = 1024 >= tau_max
constexpr int PO_ROW = 1028;     // tau_max + 1 <= 1025 cmnd values
constexpr int PO_LIST = 512;     // two neighbouring lags are never both troughs
constexpr float PYIN_LOG_FLOOR = 1e-30f;

__device__ __forceinline__ float beta_tail(float x) {
  x = fminf(fmaxf(x, 0.f), 1.f);
  const float y = 1.f - x, y2 = y * y, y4 = y2 * y2, y8 = y4 * y4;
  return (y8 * y8 * y2) * (1.f + 18.f * x);
}

__global__ __launch_bounds__(PO_WAVES * 64) void pyin_obs_kernel(const float* __restrict__ cm, int R, int tau_min,
                                                                 int tau_max, float sr, float fmin, float bins12,
                                                                 int NB, float no_trough, float* __restrict__ obs,
                                                                 float* __restrict__ vp) {
  __shared__ float row_s[PO_WAVES][PO_ROW];
  __shared__ float out_s[PO_WAVES][1024];
  __shared__ float lw_s[PO_WAVES][PO_LIST], lx_s[PO_WAVES][PO_LIST];
  __shared__ int lb_s[PO_WAVES][PO_LIST];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r = (long long)blockIdx.x * PO_WAVES + wave;
  const bool live = r < R;  // wave-uniform
  float* row = row_s[wave];
  float* out = out_s[wave];
  if (live) {
    const float* src = cm + r * (tau_max + 1);
    for (int i = lane; i <= tau_max; i += 64) row[i] = src[i];
  }
  for (int i = lane; i < 1024; i += 64) out[i] = 0.f;
  __syncthreads();

  // the lane's troughs among the lags 16 lane .. 16 lane + 15, and the smallest cmnd among them
  const int t0 = lane * PO_LAGS;
  unsigned trough = 0;
  float low = 2.f;
  if (live) {
#pragma unroll
    for (int q = 0; q < PO_LAGS; ++q) {
      const int t = t0 + q;
      if (t >= tau_min && t < tau_max) {  // tau_min >= 2, tau_max <= 1024: row[t - 1] and row[t + 1] exist
        const float b = row[t];
        if (b < row[t - 1] && b <= row[t + 1]) {
          trough |= 1u << q;
          low = fminf(low, b);
        }
      }
    }
  }
  float m = low;  // inclusive prefix minimum over the lanes, then the lanes below
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_up(m, o, 64);
    if (lane >= o) m = fminf(m, v);
  }
  m = __shfl_up(m, 1, 64);
  if (lane == 0) m = 2.f;

  // troughs below every earlier one
  unsigned rec = 0;
  {
    float mm = m;
    unsigned left = trough;
    while (left) {
      const int q = __builtin_ctz(left);
      left &= left - 1;
      const float b = row[t0 + q];
      if (b < mm) {
        rec |= 1u << q;
        mm = b;
      }
    }
  }
  const int own = __popc(rec);
  int pos = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(pos, o, 64);
    if (lane >= o) pos += v;
  }
  const int n = min(__shfl(pos, 63, 64), PO_LIST);  // never more: see PO_LIST
  pos -= own;
  while (rec) {
    const int q = __builtin_ctz(rec);
    rec &= rec - 1;
    const int t = t0 + q;
    const float a = row[t - 1], b = row[t], c = row[t + 1];
    const float sb = beta_tail(b);
    const float den = a - 2.f * b + c;
    float lag = (float)t;
    if (fabsf(den) > 1e-12f) lag += 0.5f * (a - c) / den;
    const float bin = rintf(bins12 * __log2f(sr / lag / fmin));
    if (pos < PO_LIST) {
      lw_s[wave][pos] = sb - beta_tail(m);
      lx_s[wave][pos] = no_trough * (1.f - sb);
      lb_s[wave][pos] = (int)fminf(fmaxf(bin, 0.f), (float)(NB - 1));
    }
    ++pos;
    m = b;
  }
  __syncthreads();

  if (live && lane == 0) {
    float sum = 0.f;
    for (int i = 0; i < n; ++i) {
      float w = lw_s[wave][i];
      if (i == n - 1) w += lx_s[wave][i];
      out[lb_s[wave][i]] += w;
      sum += w;
    }
    vp[r] = fminf(fmaxf(sum, 0.f), 1.f);
  }
  __syncthreads();
  if (live) {
    float* dst = obs + r * NB;
    for (int i = lane; i < NB; i += 64) dst[i] = out[i];
  }
}

// ------------------------------------------------------------------------------------------------ decoder
constexpr int PV_PAD = 64;  // >= h rounded up to the bins per thread, a multiple of 4
constexpr int PV_ROW = PV_PAD + 1024 + PV_PAD;

template <int B>
struct Cells;
template <>
struct Cells<2> {
  typedef float2 vec;
  typedef unsigned short bytes;
  static __device__ __forceinline__ void get(const float* p, float* v) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    v[0] = t.x, v[1] = t.y;
  }
  static __device__ __forceinline__ void put(float* p, const float* v) { *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]); }
};
template <>
struct Cells<4> {
  typedef float4 vec;
  typedef unsigned int bytes;
  static __device__ __forceinline__ void get(const float* p, float* v) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  }
  static __device__ __forceinline__ void put(float* p, const float* v) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};

// B bins per thread, 1024 / B threads.  meta: per utterance {first packed row, frames, plane byte offset (low, high)};
// tab: B * (steps + 1) floats, entry i = log-triangle weight of band offset o = i - (B - 1) - (hA - h), -inf outside
// 0 .. 2 h (hA = h rounded up to B, steps = (2 hA + B) / B); NBs = the plane's row stride, NB rounded up to 4.
template <int B>
__global__ __launch_bounds__(1024 / B) void pyin_viterbi_kernel(const float* __restrict__ obs,
                                                                  const float* __restrict__ vp,
                                                                  const int* __restrict__ meta, int NB, int NBs, int h,
                                                                  const float* __restrict__ tabg, float lstay,
                                                                  float lswap, float fmin, float bins12,
                                                                  unsigned char* planes, float* __restrict__ f0) {
  constexpr int PV_THREADS = 1024 / B, PV_WAVES = PV_THREADS / 64;
  constexpr int PV_TAB = 2 * PV_PAD + 2 * B;  // B * (steps + 1) table entries at the widest band
  typedef Cells<B> C;
  __shared__ __align__(16) float dl[2][2][PV_ROW];  // [buffer][voiced, unvoiced]
  __shared__ __align__(16) float tab[PV_TAB];
  __shared__ float red[2][PV_WAVES];
  __shared__ float fval[PV_WAVES];
  __shared__ int fkey[PV_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int u = blockIdx.x;
  const int row0 = meta[4 * u], T = meta[4 * u + 1];
  if (T <= 0) return;  // workgroup-uniform
  unsigned char* bp = planes + (((long long)meta[4 * u + 3] << 32) | (unsigned int)meta[4 * u + 2]);
  const float NINF = -INFINITY;
  const int hA = (h + B - 1) / B * B, shift = hA - h, steps = (2 * hA + B) / B;
  const int b0 = B * tid;
  const bool active = b0 < NB;

  for (int i = tid; i < 4 * PV_ROW; i += PV_THREADS) (&dl[0][0][0])[i] = NINF;
  for (int i = tid; i < B * (steps + 1); i += PV_THREADS) tab[i] = tabg[i];

  float nv[B], nu[B], on[B], vpn = 0.f;
#pragma unroll
  for (int k = 0; k < B; ++k) on[k] = 0.f;
  auto fetch = [&](int t) {  // the observations of frame t, ahead of their use
    const float* src = obs + (long long)(row0 + t) * NB;
#pragma unroll
    for (int k = 0; k < B; ++k)
      if (b0 + k < NB) on[k] = src[b0 + k];
    vpn = vp[row0 + t];
  };
  fetch(0);
  __syncthreads();  // the -inf fill is over
  {
    const float lu = __logf(fmaxf((1.f - vpn) / (float)NB, PYIN_LOG_FLOOR));
    float mx = NINF;
#pragma unroll
    for (int k = 0; k < B; ++k) {
      const bool in = b0 + k < NB;
      nv[k] = in ? __logf(fmaxf(on[k], PYIN_LOG_FLOOR)) : NINF;
      nu[k] = in ? lu : NINF;
      mx = fmaxf(mx, fmaxf(nv[k], nu[k]));
    }
    if (active) {
      C::put(&dl[0][0][PV_PAD + b0], nv);
      C::put(&dl[0][1][PV_PAD + b0], nu);
    }
    mx = wave_max(mx);
    if (lane == 0) red[0][wave] = mx;
  }
  if (T > 1) fetch(1);

  for (int t = 1; t < T; ++t) {
    __syncthreads();  // frame t - 1 is in dl[prv] / red[prv]; everyone is done reading dl[cur]
    const int cur = t & 1, prv = cur ^ 1;
    float M = red[prv][0];
#pragma unroll
    for (int w = 1; w < PV_WAVES; ++w) M = fmaxf(M, red[prv][w]);
    float oc[B];
#pragma unroll
    for (int k = 0; k < B; ++k) oc[k] = on[k];
    const float vpc = vpn;
    if (t + 1 < T) fetch(t + 1);
    float mx = NINF;
    if (active) {
      // band position j is bin b0 - hA + j; for the thread's bin k its offset is o = j - k - shift
      const float* pv = &dl[prv][0][PV_PAD + b0 - hA];
      const float* pu = &dl[prv][1][PV_PAD + b0 - hA];
      float bv[B], bu[B], tlo[B];
      int jv[B], ju[B];
#pragma unroll
      for (int k = 0; k < B; ++k) bv[k] = NINF, bu[k] = NINF, jv[k] = 0, ju[k] = 0;
      C::get(tab, tlo);
      for (int q = 0; q < steps; ++q) {
        float thi[B], xv[B], xu[B];
        C::get(tab + B * (q + 1), thi);
        C::get(pv + B * q, xv);
        C::get(pu + B * q, xu);
#pragma unroll
        for (int jj = 0; jj < B; ++jj) {
          const float sv = xv[jj] - M, su = xu[jj] - M;
          const int j = B * q + jj;
#pragma unroll
          for (int k = 0; k < B; ++k) {
            const int ii = jj - k + B - 1;
            const float tw = ii < B ? tlo[ii] : thi[ii - B];
            const float cv = sv + tw, cu = su + tw;
            if (cv > bv[k]) bv[k] = cv, jv[k] = j;
            if (cu > bu[k]) bu[k] = cu, ju[k] = j;
          }
        }
#pragma unroll
        for (int k = 0; k < B; ++k) tlo[k] = thi[k];
      }
      const float lu = __logf(fmaxf((1.f - vpc) / (float)NB, PYIN_LOG_FLOOR));
      unsigned int bytes_v = 0, bytes_u = 0;
#pragma unroll
      for (int k = 0; k < B; ++k) {
        const bool in = b0 + k < NB;
        const int ov = jv[k] - k - shift, ou = ju[k] - k - shift;
        const float keep_v = bv[k] + lstay, move_v = bu[k] + lswap;
        const float keep_u = bu[k] + lstay, move_u = bv[k] + lswap;
        const bool sw_v = move_v > keep_v, sw_u = move_u > keep_u;
        const float v = (sw_v ? move_v : keep_v) + __logf(fmaxf(oc[k], PYIN_LOG_FLOOR));
        const float w = (sw_u ? move_u : keep_u) + lu;
        nv[k] = in ? v : NINF;
        nu[k] = in ? w : NINF;
        if (in) {
          bytes_v |= (unsigned int)((sw_v ? (ou | 0x80) : ov) & 0xff) << (8 * k);
          bytes_u |= (unsigned int)((sw_u ? (ov | 0x80) : ou) & 0xff) << (8 * k);
          mx = fmaxf(mx, fmaxf(v, w));
        }
      }
      C::put(&dl[cur][0][PV_PAD + b0], nv);
      C::put(&dl[cur][1][PV_PAD + b0], nu);
      unsigned char* dst = bp + (size_t)t * 2 * NBs + b0;  // b0 + B <= NBs: both multiples of B, b0 < NB <= NBs
      *reinterpret_cast<typename C::bytes*>(dst) = (typename C::bytes)bytes_v;
      *reinterpret_cast<typename C::bytes*>(dst + NBs) = (typename C::bytes)bytes_u;
    }
    mx = wave_max(mx);
    if (lane == 0) red[cur][wave] = mx;
  }
  __syncthreads();  // the last frame's maxima and every back-pointer of the workgroup are visible

  // the best final state: voiced before unvoiced, then the lowest bin (key = voicing * 1024 + bin)
  const int last = (T - 1) & 1;
  float M = red[last][0];
#pragma unroll
  for (int w = 1; w < PV_WAVES; ++w) M = fmaxf(M, red[last][w]);
  float best = NINF;
  int key = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < B; ++k) {
    const float v = nv[k] - M;
    if (b0 + k < NB && v > best) best = v, key = b0 + k;
  }
#pragma unroll
  for (int k = 0; k < B; ++k) {
    const float v = nu[k] - M;
    if (b0 + k < NB && v > best) best = v, key = 1024 + b0 + k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v = __shfl_xor(best, o, 64);
    const int kk = __shfl_xor(key, o, 64);
    if (v > best || (v == best && kk < key)) best = v, key = kk;
  }
  if (lane == 0) fval[wave] = best, fkey[wave] = key;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PV_WAVES; ++w)
      if (fval[w] > best || (fval[w] == best && fkey[w] < key)) best = fval[w], key = fkey[w];
    int s = (key >> 10) & 1, b = min(key & 1023, NB - 1);
    for (int t = T - 1; t >= 0; --t) {
      f0[row0 + t] = s ? 0.f : fmin * exp2f((float)b / bins12);
      if (t > 0) {
        const unsigned int byte = bp[((size_t)t * 2 + s) * NBs + b];
        b = min(max(b + (int)(byte & 127u) - h, 0), NB - 1);  // a state's predecessor is on the grid; the clamp only
        s ^= (int)(byte >> 7);                                // keeps a read inside the plane whatever the bytes are
      }
    }
  }
}

}  // namespace

// cm [R, tau_max + 1]: the cmnd plane of ssamd_yin.  Writes obs [R, NB] whole and voiced_prob [R].
SSAMD_API int ssamd_pyin_obs(const float* cm, int R, int tau_min, int tau_max, float sr, float fmin, float bins12, int NB,
                             float no_trough, float* obs, float* vp, hipStream_t s) {
  if (tau_min < 2 || tau_max > 1024 || tau_min >= tau_max || NB < 1 || NB > 1024 || !(fmin > 0.f) || !(sr > 0.f)) return -2;
  if (R <= 0) return 0;
  if (!cm || !obs || !vp) return -2;
  hipLaunchKernelGGL(pyin_obs_kernel, dim3((R + PO_WAVES - 1) / PO_WAVES), dim3(PO_WAVES * 64), 0, s, cm, R, tau_min,
                     tau_max, sr, fmin, bins12, NB, no_trough, obs, vp);
  return (int)hipGetLastError();
}

// obs [R, NB] / vp [R] packed rows; meta [n, 4] int32 (see the kernel); bins: 2 or 4 bins per thread; tab: the padded
// log-triangle table for that many; planes: n planes of frames * 2 * NBs bytes at meta's offsets (frame 0's rows are
// not written); f0 [R].
SSAMD_API int ssamd_pyin_viterbi(const float* obs, const float* vp, const int* meta, int n, int NB, int h, int bins,
                                 const float* tab, float lstay, float lswap, float fmin, float bins12, void* planes,
                                 float* f0, hipStream_t s) {
  if (NB < 1 || NB > 1024 || h < 0 || h > 63 || !(bins12 > 0.f) || (bins != 2 && bins != 4)) return -2;
  if (n <= 0) return 0;
  if (!obs || !vp || !meta || !tab || !planes || !f0) return -2;
  unsigned char* bp = static_cast<unsigned char*>(planes);
  const int NBs = (NB + 3) & ~3;
  if (bins == 2)
    hipLaunchKernelGGL(pyin_viterbi_kernel<2>, dim3(n), dim3(512), 0, s, obs, vp, meta, NB, NBs, h, tab, lstay, lswap, fmin,
                       bins12, bp, f0);
  else
    hipLaunchKernelGGL(pyin_viterbi_kernel<4>, dim3(n), dim3(256), 0, s, obs, vp, meta, NB, NBs, h, tab, lstay, lswap, fmin,
                       bins12, bp, f0);
  return (int)hipGetLastError();
}

// Workgroup scans and sums in thread order, shared by the kernels that fill the unvoiced frames of an F0 contour
// (k_prosody.hip stages A and C, k_features.hip interp_unvoiced_kernel), and the latter's interpolation.
// A workgroup of WG_SCAN_THREADS threads (4 waves); every thread calls a scan (two barriers each).
#pragma once
#include "common.h"

constexpr int WG_SCAN_THREADS = 256;
constexpr int WG_SCAN_WAVES = WG_SCAN_THREADS / 64;
constexpr int WG_SCAN_NONE = 0x7fffffff;  // "no voiced frame at or after": the identity of the min-scan

struct OpAdd { __device__ __forceinline__ int operator()(int a, int b) const { return a + b; } };
struct OpMax { __device__ __forceinline__ int operator()(int a, int b) const { return a > b ? a : b; } };
struct OpMin { __device__ __forceinline__ int operator()(int a, int b) const { return a < b ? a : b; } };

// inclusive scan over the workgroup's threads in thread order; `all` = the value over all of them.  Every thread
// calls it (two barriers); `wtot` [WG_SCAN_WAVES] is free again on return.
template <class Op>
__device__ __forceinline__ int block_scan(int v, Op op, int* wtot, int& all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v = op(o, v);
  }
  if (lane == 63) wtot[wave] = v;
  __syncthreads();
  all = wtot[0];
#pragma unroll
  for (int w = 1; w < WG_SCAN_WAVES; ++w) all = op(all, wtot[w]);
  for (int w = wave - 1; w >= 0; --w) v = op(wtot[w], v);
  __syncthreads();
  return v;
}

// sum over the workgroup in a fixed order, to every thread (two barriers); `ftot` [WG_SCAN_WAVES]
__device__ __forceinline__ float block_sum(float v, float* ftot) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) ftot[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = ftot[0];
#pragma unroll
  for (int w = 1; w < WG_SCAN_WAVES; ++w) s += ftot[w];
  __syncthreads();
  return s;
}

// Frame j of the contour fy between its nearest voiced frames a <= j (a < 0: none) and b >= j (WG_SCAN_NONE: none),
// at least one of which exists: linear in Hz between them (np.interp's slope * (x - xa) + fa), the ends held.  Every
// operation is rounded on its own (no fused multiply-add): bit for bit what float32 host arithmetic gives
// (ops/reference.py::interp_unvoiced on a float32 tensor).  k_prosody.hip keeps its own, contracted expression.
__device__ __forceinline__ float interp_voiced_rn(const float* __restrict__ fy, int j, int a, int b) {
#pragma clang fp contract(off)
  if (a < 0) return fy[b];
  if (b == WG_SCAN_NONE) return fy[a];
  const float slope = (fy[b] - fy[a]) / (float)(b - a);
  const float rise = slope * (float)(j - a);
  return rise + fy[a];
}

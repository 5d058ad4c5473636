// Batched dynamic time warping (objective synthesis metrics: speakingstyle_amd/analysis/objective.py).
//
//   c(i, j) = sqrt(sum_d (x[i, d] - y[j, d])^2)            (from the differences, d in index order)
//   A(i, j) = c(i, j) + min(A(i-1, j-1), A(i-1, j), A(i, j-1)),   A(0, 0) = c(0, 0), missing = +inf
//   tie rule: diagonal, then (i-1, j), then (i, j-1); a later candidate wins only on strict <
//
// dtw_fwd: one workgroup of 8 waves per pair.  The pair is swept in strips of 64 rows and blocks of 64 wavefront
// steps.  Wave 0 runs the recurrence: lane l owns row 64 s + l and visits column j = t - l at step t; "up" is the
// previous step's value of lane l - 1 (one DPP shift), "diagonal" is the "up" of the step before, "left" is the
// lane's own previous value.  The local costs do not depend on the recurrence, so the other 7 waves compute them
// one block ahead into a double-buffered 64 x 64 LDS tile: each holds the strip's x rows in registers and reads y
// rows from an LDS ring of 2 x 64 rows (row stride odd: 64 lanes read 64 consecutive rows without a bank
// conflict); one of them keeps the next 64 y rows in flight in registers.  Two barriers per block.  The last row
// of a strip is handed to the next strip through an LDS array of Ty floats (read 64 ahead, written 64 behind).
// The direction bytes go to the pair's plane in the layout of dtw_index.h (4 steps per dword, 256 B per wave
// store).  No atomics, no scratch; a pair's result depends on nothing but its own rows: bitwise what it is alone.
//
// dtw_path: one wave per pair walks the plane back from (Tx-1, Ty-1).  The wave loads the 4 KiB tile the walk is
// in into LDS with one coalesced read; lane 0 walks inside it and writes the path backwards from the end of the
// pair's row of `path`; the wave then moves it to the front and fills the rest with -1.
#include "common.h"
#include "dtw_index.h"

namespace {

constexpr int DTW_MAX_D = 80;
constexpr int DTW_RING = 2 * DTW_BLOCK;  // y rows resident in LDS
constexpr int DTW_TILE_CELLS = DTW_STRIP * DTW_BLOCK;  // local costs of one (strip, block) tile
constexpr int DTW_WAVES = 8;             // 1 recurrence wave + 7 local-cost producers (one of them also loads y)

// value of lane l - 1 (lane 0 keeps `self`): v_mov_b32 with DPP wave_shr:1
__device__ __forceinline__ float lane_shr1(float v, float self) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(self), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float read_lane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// rows [row0, row0 + 64) of y (zeros past Ty and past D): lane m fetches row row0 + m
template <int DP>
__device__ __forceinline__ void fetch_y(const float* __restrict__ y, int row0, int Ty, int D, int lane, float* r) {
  const int j = row0 + lane;
  const float* src = y + (long)(j < Ty ? j : 0) * D;
#pragma unroll
  for (int d = 0; d < DP; ++d) r[d] = (j < Ty && d < D) ? src[d] : 0.f;
}
template <int DP>
__device__ __forceinline__ void put_y(float* ring, int slot, int lane, const float* r) {
  float* dst = ring + (slot * DTW_BLOCK + lane) * (DP + 1);
#pragma unroll
  for (int d = 0; d < DP; ++d) dst[d] = r[d];
}

// Local costs of the 64 x 64 tile of block b of the current strip: c(i, t - lane) for the in-block steps
// u = first, first + stride, ... (one producer wave's share) -> tile[u * 64 + lane].  Cells outside the matrix get
// whatever the ring holds there; the recurrence never uses them.
template <int DP>
__device__ __forceinline__ void produce_tile(const float* ring, const float* xr, int t0, int lane, int first,
                                             int stride, float* tile) {
#pragma unroll 2
  for (int u = first; u < DTW_BLOCK; u += stride) {
    const int j = t0 + u - lane;
    const float* yr = ring + (j & (DTW_RING - 1)) * (DP + 1);
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < DP; ++d) {
      const float df = xr[d] - yr[d];
      acc = fmaf(df, df, acc);
    }
    tile[u * DTW_STRIP + lane] = __fsqrt_rn(acc);
  }
}

template <int DP>
__global__ __launch_bounds__(DTW_WAVES * 64) void dtw_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                const int* __restrict__ cu_x, const int* __restrict__ cu_y,
                                                                const long long* __restrict__ plane_off, int D,
                                                                uint8_t* __restrict__ plane, float* __restrict__ cost) {
  extern __shared__ __align__(16) float smem[];
  float* ring = smem;                              // [DTW_RING][DP + 1]: y rows of two consecutive blocks
  float* ctile = ring + DTW_RING * (DP + 1);       // [2][64 steps][64 lanes]: local costs, double-buffered
  float* hand = ctile + 2 * DTW_TILE_CELLS;        // [Ty]: last row of the previous strip
  const int p = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = cu_x[p], Tx = cu_x[p + 1] - x0;
  const int y0 = cu_y[p], Ty = cu_y[p + 1] - y0;
  if (Tx <= 0 || Ty <= 0) return;  // rejected on the host; never reached
  const float* x = X + (long)x0 * D;
  const float* y = Y + (long)y0 * D;
  uint32_t* tiles = reinterpret_cast<uint32_t*>(plane + plane_off[p]);
  const int nstrip = dtw_num_strips(Tx), nblk = dtw_num_blocks(Ty);
  const float INF = __builtin_inff();
  float total = INF;  // A(Tx - 1, Ty - 1), in the recurrence lane that owns row Tx - 1

  for (int s = 0; s < nstrip; ++s) {
    const int i = s * DTW_STRIP + lane;
    const bool row_ok = i < Tx;
    float xr[DP];  // the producers' x row
    if (wave != 0) {
      const float* src = x + (long)(row_ok ? i : 0) * D;
#pragma unroll
      for (int d = 0; d < DP; ++d) xr[d] = (row_ok && d < D) ? src[d] : 0.f;
    } else {
#pragma unroll
      for (int d = 0; d < DP; ++d) xr[d] = 0.f;
    }
    float nxt[DP];  // the loader wave's y rows in flight
    if (wave == 1) fetch_y<DP>(y, 0, Ty, D, lane, nxt);
    __syncthreads();  // the previous strip is done with the ring and the cost tiles
    if (wave == 1) put_y<DP>(ring, 0, lane, nxt);
    float a = INF;                                  // A(i, j - 1): the lane's previous value
    float up = (s == 0 && lane == 0) ? 0.f : INF;   // becomes "diagonal" at the first step: A(-1, -1) = 0 for (0, 0)
    // tick b: wave 0 runs the recurrence over block b while the producers fill the cost tile of block b + 1 from
    // the y blocks b and b + 1 in the ring; the loader wave has block b + 2 in flight and stores it after the tick
    for (int b = -1; b < nblk; ++b) {
      const int t0 = b * DTW_BLOCK;
      const bool more = b + 2 < nblk;
      if (wave == 1 && more) fetch_y<DP>(y, t0 + 2 * DTW_BLOCK, Ty, D, lane, nxt);
      __syncthreads();  // the ring holds blocks b and b + 1, cost tile b is complete
      if (wave != 0) {
        if (b + 1 < nblk)
          produce_tile<DP>(ring, xr, t0 + DTW_BLOCK, lane, wave - 1, DTW_WAVES - 1, ctile + ((b + 1) & 1) * DTW_TILE_CELLS);
      } else if (b >= 0) {
        const float* ct = ctile + (b & 1) * DTW_TILE_CELLS;
        // A(i0 - 1, t0 + m) for lane 0's "up" at in-block step m (strip 0 has no row above)
        const float hin = (s > 0 && t0 + lane < Ty) ? hand[t0 + lane] : INF;
        float hout = INF;  // lane m: A(i63, t0 + m - 63), collected from lane 63
#pragma unroll 1
        for (int q = 0; q < DTW_BLOCK / 16; ++q) {
          float cr[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) cr[k] = ct[(q * 16 + k) * DTW_STRIP + lane];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            uint32_t dirs = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              const int u = q * 16 + g * 4 + k;
              const int j = t0 + u - lane;
              const float diag = up;
              up = lane_shr1(a, read_lane(hin, u));
              float best = diag;
              uint32_t dir = DTW_DIAG;
              if (up < best) { best = up; dir = DTW_UP; }
              if (a < best) { best = a; dir = DTW_LEFT; }
              const bool ok = row_ok && j >= 0 && j < Ty;
              a = ok ? cr[g * 4 + k] + best : INF;
              if (i == Tx - 1 && j == Ty - 1) total = a;
              dirs |= (ok ? dir : 0u) << (8 * k);
              const float last = read_lane(a, DTW_STRIP - 1);
              if (lane == u) hout = last;
            }
            tiles[((long)(s * nblk + b) * (DTW_BLOCK / 4) + q * 4 + g) * DTW_STRIP + lane] = dirs;
          }
        }
        const int jw = t0 + lane - (DTW_STRIP - 1);  // only wave 0 touches the hand-over row: program order
        if (jw >= 0 && jw < Ty) hand[jw] = hout;
      }
      __syncthreads();  // every read of ring block b and of cost tile b is done
      if (wave == 1 && more) put_y<DP>(ring, b & 1, lane, nxt);
    }
  }
  if (wave == 0 && lane == (Tx - 1) % DTW_STRIP) cost[p] = total;
}

// one wave per pair: walk back through the direction plane
__global__ __launch_bounds__(64) void dtw_path_kernel(const uint8_t* __restrict__ plane,
                                                      const long long* __restrict__ plane_off,
                                                      const int* __restrict__ cu_x, const int* __restrict__ cu_y,
                                                      int Lmax, int* __restrict__ path, int* __restrict__ path_len) {
  __shared__ __align__(16) uint8_t tile[DTW_TILE_BYTES];
  __shared__ int state[3];
  const int p = blockIdx.x, lane = threadIdx.x;
  const int Tx = cu_x[p + 1] - cu_x[p], Ty = cu_y[p + 1] - cu_y[p];
  int2* out = reinterpret_cast<int2*>(path) + (long)p * Lmax;
  if (Tx <= 0 || Ty <= 0 || Tx + Ty - 1 > Lmax) {  // rejected on the host; never reached
    for (int k = lane; k < Lmax; k += 64) out[k] = make_int2(-1, -1);
    if (lane == 0) path_len[p] = 0;
    return;
  }
  const uint8_t* pl = plane + plane_off[p];
  int i = Tx - 1, j = Ty - 1, n = 0;  // n cells written so far, at out[Lmax - 1 - k]
  while (true) {
    const long long tl = dtw_tile(i, j, Ty);
    {
      const uint4* src = reinterpret_cast<const uint4*>(pl + tl * DTW_TILE_BYTES);
#pragma unroll
      for (int q = 0; q < DTW_TILE_BYTES / 16 / 64; ++q) reinterpret_cast<uint4*>(tile)[q * 64 + lane] = src[q * 64 + lane];
    }
    __syncthreads();
    if (lane == 0) {
      // at most Tx + Ty - 1 <= Lmax cells in all: i + j falls by at least 1 per step and the edges force the move
      while (dtw_tile(i, j, Ty) == tl) {
        out[Lmax - 1 - n] = make_int2(i, j);
        ++n;
        if (i == 0 && j == 0) { i = -1; break; }
        int dir = tile[dtw_cell_byte(i, j)];
        if (i == 0) dir = DTW_LEFT;
        else if (j == 0) dir = DTW_UP;
        dtw_step_back(dir, i, j);
      }
      state[0] = i; state[1] = j; state[2] = n;
    }
    __syncthreads();
    i = state[0]; j = state[1]; n = state[2];
    __syncthreads();
    if (i < 0) break;
  }
  __threadfence();  // lane 0's cells are visible to the whole wave
  // move the n cells from the end of the row to its front (ascending: a chunk's sources lie at or past its
  // destinations and past every earlier chunk's), then pad with -1
  const int shift = Lmax - n;
  for (int k0 = 0; k0 < n; k0 += 64) {
    const int k = k0 + lane;
    int2 v = make_int2(-1, -1);
    if (k < n) v = out[shift + k];
    __syncthreads();
    if (k < n && shift > 0) out[k] = v;
    __threadfence();
    __syncthreads();
  }
  for (int k = n + lane; k < Lmax; k += 64) out[k] = make_int2(-1, -1);
  if (lane == 0) path_len[p] = n;
}

template <int DP>
size_t fwd_lds_bytes(int max_ty) {
  return ((size_t)DTW_RING * (DP + 1) + 2 * DTW_TILE_CELLS + (size_t)max_ty) * sizeof(float);
}

template <int DP>
int launch_fwd(const float* x, const float* y, const int* cu_x, const int* cu_y, const long long* plane_off, int P,
               int D, int max_ty, uint8_t* plane, float* cost, hipStream_t s) {
  const size_t lds = fwd_lds_bytes<DP>(max_ty);
  if (lds > 160 * 1024) return -3;
  allow_lds(dtw_fwd_kernel<DP>, lds);
  hipLaunchKernelGGL(dtw_fwd_kernel<DP>, dim3(P), dim3(DTW_WAVES * 64), lds, s, x, y, cu_x, cu_y, plane_off, D, plane, cost);
  return (int)hipGetLastError();
}

}  // namespace

// bytes of the direction plane of a Tx x Ty pair (csrc/dtw_index.h)
SSAMD_API long ssamd_dtw_plane_bytes(int Tx, int Ty) { return Tx > 0 && Ty > 0 ? (long)dtw_plane_bytes(Tx, Ty) : 0; }

// longest y the forward kernel takes at feature size D (the hand-over row lives in LDS); 0: D not covered
SSAMD_API long ssamd_dtw_max_ty(int D) {
  if (D < 1 || D > DTW_MAX_D) return 0;
  const int DP = (D + 15) / 16 * 16;
  return (long)(160 * 1024 / sizeof(float)) - (long)DTW_RING * (DP + 1) - 2 * DTW_TILE_CELLS;
}

// x [Rx, D] / y [Ry, D] fp32 packed by cu_x / cu_y [P + 1]; plane_off [P] int64 byte offsets into `plane`
// (dtw_plane_bytes each); max_ty >= every pair's Ty.  Writes the planes and cost [P].
SSAMD_API int ssamd_dtw_fwd(const float* x, const float* y, const int* cu_x, const int* cu_y,
                            const long long* plane_off, int P, int D, int max_ty, uint8_t* plane, float* cost,
                            hipStream_t s) {
  if (D < 1 || D > DTW_MAX_D || max_ty < 1) return -2;
  if (P <= 0) return 0;
  if (!x || !y || !cu_x || !cu_y || !plane_off || !plane || !cost) return -2;
  switch ((D + 15) / 16) {
    case 1: return launch_fwd<16>(x, y, cu_x, cu_y, plane_off, P, D, max_ty, plane, cost, s);
    case 2: return launch_fwd<32>(x, y, cu_x, cu_y, plane_off, P, D, max_ty, plane, cost, s);
    case 3: return launch_fwd<48>(x, y, cu_x, cu_y, plane_off, P, D, max_ty, plane, cost, s);
    case 4: return launch_fwd<64>(x, y, cu_x, cu_y, plane_off, P, D, max_ty, plane, cost, s);
    default: return launch_fwd<80>(x, y, cu_x, cu_y, plane_off, P, D, max_ty, plane, cost, s);
  }
}

// path [P, Lmax, 2] int32 in increasing order (-1 past path_len [P]); Lmax >= every pair's Tx + Ty - 1
SSAMD_API int ssamd_dtw_path(const uint8_t* plane, const long long* plane_off, const int* cu_x, const int* cu_y, int P,
                             int Lmax, int* path, int* path_len, hipStream_t s) {
  if (P <= 0) return 0;
  if (Lmax < 1 || !plane || !plane_off || !cu_x || !cu_y || !path || !path_len) return -2;
  hipLaunchKernelGGL(dtw_path_kernel, dim3(P), dim3(64), 0, s, plane, plane_off, cu_x, cu_y, Lmax, path, path_len);
  return (int)hipGetLastError();
}

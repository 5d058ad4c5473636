// Style map (speakingstyle_amd/analysis/style_map.py): exact t-SNE and k-means of a corpus's style embeddings.
// Semantics: ops/reference.py::tsne_affinities / tsne_gradient / tsne_kl / tsne_step / kmeans.
//
// fp32 throughout, no atomics, no scratch.  Every sum has a fixed order that depends on the problem size alone: a
// thread's terms in increasing index, the lanes of a wave by one butterfly, the waves of a workgroup in wave order,
// workgroups by per-block partials that ssamd_seg_colsum (k_reduce.hip) adds in order.  Two runs are bitwise equal
// wherever the blocks land.
//
//   tsne_pairdist_kernel     d_ij = sum_d (x_id - x_jd)^2 from the differences, the columns in a fixed order (16 in
//                            sequence, 8 such sums, then those): 64 x 64 tile per workgroup, 4 x 4 per thread, 16
//                            columns of x at a time through LDS.  Writes the plane that becomes P.
//   tsne_perplexity_kernel   a workgroup per row, the row in LDS (N <= 16384: 64 KiB).  Row minimum (off the diagonal)
//                            subtracted, then scikit-learn's bisection on beta: beta = 1, <= 100 steps, stop at
//                            |H - log perplexity| <= 1e-5, double / halve while a bound is infinite.  v_exp_f32 /
//                            v_log_f32.  The conditional row of the last evaluation replaces the distances.
//   tsne_planesum_kernel     2 * (sum of a 64 x 64 tile) per workgroup: the partials of sum (C + C^T).
//   tsne_symmetrise_kernel   in place, a workgroup per tile pair (I, J), I <= J: both tiles to LDS, then
//                            P_ij = P_ji = (C_ij + C_ji) / sum, zero diagonal.
//   tsne_grad_kernel         lane = row i; j runs over the workgroup's share of the columns (blockIdx.y), the 4 waves
//                            take alternate 128-wide slices of it.  P is symmetric, so P[j][i] is read: coalesced over
//                            the lanes; y_j is wave-uniform from LDS.  No cross-lane sum; the waves meet in LDS in wave
//                            order.  attr / rep / zrow and, on request, the row's KL part, as planes [6][N].
//   tsne_update_kernel       Z (every workgroup sums zrow in the same order), gradient, gains, momentum, update; the
//                            KL into its slot of the trace.
//   kmeans_far_kernel / kmeans_pick_kernel   farthest-point start, one centre per launch pair.
//   kmeans_assign_kernel     128 points per workgroup, a thread per point, 16 columns of the centroids at a time in
//                            LDS; then each thread owns a column and adds the workgroup's points to their clusters'
//                            sums in point order (LDS, one writer per word).  Partials: sums, counts, labels changed.
//   kmeans_finish_kernel     centroid = sum / count (IEEE), an empty cluster keeps its centroid.
// The k-means distances round every product and every sum on its own (no fused multiply-add): bit for bit what
// ops/reference.py computes on a float32 tensor.
#include "common.h"
#include "wg_scan.h"

namespace {

constexpr int SM_MAX_N = 16384;  // reference.TSNE_MAX_N
constexpr int SM_BISECT_STEPS = 100;
constexpr float SM_ENTROPY_TOL = 1e-5f;
constexpr float SM_LN2 = 0.6931471805599453f;
constexpr float SM_LOG2E = 1.4426950408889634f;
constexpr int SM_TILE = 64;
constexpr int SM_PLANES = 6;  // attr x, attr y, rep x, rep y, zrow, KL part (in bits: times ln 2 at the end)

// ---------------------------------------------------------------- pairwise distances
constexpr int PD_K = 16, PD_LD = SM_TILE + 4;

__global__ __launch_bounds__(256) void tsne_pairdist_kernel(const float* __restrict__ x, int N, int D,
                                                            float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xi[PD_K][PD_LD];
  __shared__ __attribute__((aligned(16))) float xj[PD_K][PD_LD];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int i0 = blockIdx.y * SM_TILE, j0 = blockIdx.x * SM_TILE;
  // three levels, each in sequence: 16 columns, 8 such sums, then those.  One chain over D = 512 loses 4 to 5 times
  // the bits of torch's pairwise sum, which the bisection at perplexity 2 (large beta) magnifies.
  float acc[4][4], mid[4][4], cur[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = mid[r][c] = 0.f;
  for (int d0 = 0; d0 < D; d0 += PD_K) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) cur[r][c] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = t + 256 * q, k = e & (PD_K - 1), r = e >> 4;
      const bool dk = d0 + k < D;
      xi[k][r] = (dk && i0 + r < N) ? x[(long)(i0 + r) * D + d0 + k] : 0.f;
      xj[k][r] = (dk && j0 + r < N) ? x[(long)(j0 + r) * D + d0 + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PD_K; ++k) {  // columns past D hold zeros on both sides: they add nothing
      const float4 a = *reinterpret_cast<const float4*>(&xi[k][ty * 4]);
      const float4 b = *reinterpret_cast<const float4*>(&xj[k][tx * 4]);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float df = av[r] - bv[c];
          cur[r][c] = fmaf(df, df, cur[r][c]);
        }
    }
    const bool close = ((d0 / PD_K) & 7) == 7 || d0 + PD_K >= D;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        mid[r][c] += cur[r][c];
        if (close) {
          acc[r][c] += mid[r][c];
          mid[r][c] = 0.f;
        }
      }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + ty * 4 + r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = j0 + tx * 4 + c;
      if (i < N && j < N) out[(long)i * N + j] = acc[r][c];
    }
  }
}

// ---------------------------------------------------------------- conditional rows
constexpr int PX_RED = 16;  // floats ahead of the row: two buffers of {sum p, sum d p} x 4 waves

__global__ __launch_bounds__(256) void tsne_perplexity_kernel(float* __restrict__ plane, int N, float log_perp) {
  extern __shared__ float px_lds[];
  float* red = px_lds;
  float* row = px_lds + PX_RED;
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float* g = plane + (long)i * N;
  float mn = INFINITY;
  for (int j = t; j < N; j += 256) {
    const float v = g[j];
    row[j] = v;
    if (j != i) mn = fminf(mn, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, 64));
  if (lane == 0) red[wave] = mn;
  __syncthreads();
  mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  __syncthreads();
  for (int j = t; j < N; j += 256) row[j] -= mn;  // a thread's own words
  float beta = 1.f, lo = -INFINITY, hi = INFINITY, nb_used = -SM_LOG2E, s_used = 1.f;
  for (int step = 0; step < SM_BISECT_STEPS; ++step) {
    const float nb = -beta * SM_LOG2E;
    float s = 0.f, sd = 0.f;
    for (int j = t; j < N; j += 256) {
      if (j == i) continue;
      const float d = row[j];
      const float p = __builtin_amdgcn_exp2f(d * nb);
      s += p;
      sd = fmaf(d, p, sd);
    }
    s = wave_sum(s);
    sd = wave_sum(sd);
    float* buf = red + (step & 1) * 8;  // alternate buffers: one barrier per step
    if (lane == 0) {
      buf[wave] = s;
      buf[4 + wave] = sd;
    }
    __syncthreads();
    s = ((buf[0] + buf[1]) + buf[2]) + buf[3];
    sd = ((buf[4] + buf[5]) + buf[6]) + buf[7];
    nb_used = nb;
    s_used = s;
    const float diff = __builtin_amdgcn_logf(s) * SM_LN2 + beta * sd / s - log_perp;  // the same in every thread
    if (fabsf(diff) <= SM_ENTROPY_TOL) break;
    if (diff > 0.f) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.f : (beta + hi) * 0.5f;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta * 0.5f : (beta + lo) * 0.5f;
    }
  }
  for (int j = t; j < N; j += 256) g[j] = j == i ? 0.f : __builtin_amdgcn_exp2f(row[j] * nb_used) / s_used;
}

// ---------------------------------------------------------------- joint P
__global__ __launch_bounds__(256) void tsne_planesum_kernel(const float* __restrict__ plane, int N,
                                                            float* __restrict__ part) {
  __shared__ float ftot[WG_SCAN_WAVES];
  const int t = threadIdx.x, c = t & 63, r0 = t >> 6;
  const int i0 = blockIdx.y * SM_TILE, j = blockIdx.x * SM_TILE + c;
  float s = 0.f;
  for (int r = r0; r < SM_TILE; r += 4) {
    const int i = i0 + r;
    if (i < N && j < N) s += plane[(long)i * N + j];
  }
  s = block_sum(s, ftot);
  if (t == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = 2.f * s;
}

__global__ __launch_bounds__(256) void tsne_symmetrise_kernel(float* __restrict__ plane, int N,
                                                              const float* __restrict__ total) {
  __shared__ float a[SM_TILE][SM_TILE + 1];
  __shared__ float b[SM_TILE][SM_TILE + 1];
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj < ti) return;  // the pair (tj, ti) does both tiles
  const int t = threadIdx.x, c = t & 63, r0 = t >> 6;
  const int i0 = ti * SM_TILE, j0 = tj * SM_TILE;
  for (int r = r0; r < SM_TILE; r += 4) {
    a[r][c] = (i0 + r < N && j0 + c < N) ? plane[(long)(i0 + r) * N + j0 + c] : 0.f;
    b[r][c] = (j0 + r < N && i0 + c < N) ? plane[(long)(j0 + r) * N + i0 + c] : 0.f;
  }
  __syncthreads();
  const float tot = total[0];
  for (int r = r0; r < SM_TILE; r += 4) {
    if (i0 + r < N && j0 + c < N)
      plane[(long)(i0 + r) * N + j0 + c] = (i0 + r == j0 + c) ? 0.f : (a[r][c] + b[c][r]) / tot;
    if (ti != tj && j0 + r < N && i0 + c < N) plane[(long)(j0 + r) * N + i0 + c] = (a[c][r] + b[r][c]) / tot;
  }
}

// ---------------------------------------------------------------- gradient sums
constexpr int GR_SLICE = 128;               // columns a wave walks per tile
constexpr int GR_TILE = 4 * GR_SLICE;       // columns of y staged per pass

__global__ __launch_bounds__(256) void tsne_grad_kernel(const float* __restrict__ P, const float* __restrict__ y, int N,
                                                        int jchunk, float* __restrict__ part, int want_kl) {
  __shared__ float2 ys[GR_TILE];
  __shared__ float meet[4][SM_PLANES][64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int i = blockIdx.x * 64 + lane;
  const int ic = i < N ? i : N - 1;  // a lane past the last row reads row N - 1 and writes nothing
  const int j0 = blockIdx.y * jchunk;
  const int j1 = min(N, j0 + jchunk);
  const float yix = y[2 * ic], yiy = y[2 * ic + 1];
  float ax = 0.f, ay = 0.f, rx = 0.f, ry = 0.f, z = 0.f, kl = 0.f;
  for (int jt = j0; jt < j1; jt += GR_TILE) {
    for (int q = t; q < GR_TILE; q += 256) {
      const int j = jt + q;
      ys[q] = j < j1 ? make_float2(y[2 * j], y[2 * j + 1]) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const int a = jt + wave * GR_SLICE;
    const int b = min(j1, a + GR_SLICE);
    const float* col = P + (long)a * N + ic;
    for (int j = a; j < b; ++j, col += N) {
      const float p = *col;
      const float2 yj = ys[j - jt];
      const float dx = yix - yj.x, dy = yiy - yj.y;
      float w = 1.f / (1.f + fmaf(dx, dx, dy * dy));
      w = j == i ? 0.f : w;
      const float pw = p * w, ww = w * w;
      ax = fmaf(pw, dx, ax);
      ay = fmaf(pw, dy, ay);
      rx = fmaf(ww, dx, rx);
      ry = fmaf(ww, dy, ry);
      z += w;
      // v_log_f32 takes no subnormals; such a P adds less than 1e-35
      if (want_kl && p >= 1.17549435e-38f && j != i) kl = fmaf(p, __builtin_amdgcn_logf(p) - __builtin_amdgcn_logf(w), kl);
    }
    __syncthreads();
  }
  meet[wave][0][lane] = ax;
  meet[wave][1][lane] = ay;
  meet[wave][2][lane] = rx;
  meet[wave][3][lane] = ry;
  meet[wave][4][lane] = z;
  meet[wave][5][lane] = kl;
  __syncthreads();
  for (int q = wave; q < SM_PLANES; q += 4) {
    const float v = ((meet[0][q][lane] + meet[1][q][lane]) + meet[2][q][lane]) + meet[3][q][lane];
    if (i < N) part[((long)blockIdx.y * SM_PLANES + q) * N + i] = v;
  }
}

// ---------------------------------------------------------------- descent step
__global__ __launch_bounds__(256) void tsne_update_kernel(const float* __restrict__ red, int N, float exag,
                                                          float momentum, float lr, float* __restrict__ y,
                                                          float* __restrict__ upd, float* __restrict__ gains,
                                                          float* __restrict__ grad_out, float* __restrict__ kl_slot,
                                                          int do_update) {
  __shared__ float ftot[WG_SCAN_WAVES];
  const int t = threadIdx.x;
  float z = 0.f;
  for (int j = t; j < N; j += 256) z += red[4L * N + j];
  const float Z = block_sum(z, ftot);  // the same bits in every workgroup
  if (kl_slot && blockIdx.x == 0) {
    float k = 0.f;
    for (int j = t; j < N; j += 256) k += red[5L * N + j];
    k = block_sum(k, ftot);
    if (t == 0) kl_slot[0] = (k + __builtin_amdgcn_logf(Z)) * SM_LN2;
  }
  const int e = blockIdx.x * 256 + t;
  if (e >= 2 * N) return;
  const int i = e >> 1, c = e & 1;
  const float g = 4.f * (exag * red[(long)c * N + i] - red[(long)(2 + c) * N + i] / Z);
  if (grad_out) grad_out[e] = g;
  if (!do_update) return;
  float u = upd[e], gn = gains[e];
  gn = u * g < 0.f ? gn + 0.2f : gn * 0.8f;
  gn = fmaxf(gn, 0.01f);
  u = momentum * u - lr * (gn * g);
  upd[e] = u;
  gains[e] = gn;
  y[e] += u;
}

// ---------------------------------------------------------------- k-means
constexpr int KM_THREADS = 128, KM_MAX_K = 64, KM_MAX_D = 512, KM_DK = 16;

// squared distance with every product and sum rounded on its own, columns in increasing order
__device__ __forceinline__ float sq_acc(float acc, float a, float b) {
#pragma clang fp contract(off)
  const float df = a - b;
  const float sq = df * df;
  return acc + sq;
}

// larger value wins, the lower index on ties
__device__ __forceinline__ void far_merge(float& v, int& ix, float ov, int oi) {
  if (ov > v || (ov == v && oi < ix)) {
    v = ov;
    ix = oi;
  }
}

template <int THREADS>
__device__ __forceinline__ void far_block(float& v, int& ix, float* sv, int* si) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) far_merge(v, ix, __shfl_xor(v, o, 64), __shfl_xor(ix, o, 64));
  if (lane == 0) {
    sv[wave] = v;
    si[wave] = ix;
  }
  __syncthreads();
  v = sv[0];
  ix = si[0];
#pragma unroll
  for (int w = 1; w < THREADS / 64; ++w) far_merge(v, ix, sv[w], si[w]);
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_far_kernel(const float* __restrict__ x, int N, int D, int idx0,
                                                                const int* __restrict__ idx_ptr, int step,
                                                                float* __restrict__ cent, float* __restrict__ mind,
                                                                float* __restrict__ pval, int* __restrict__ pidx) {
  __shared__ float c[KM_MAX_D];
  __shared__ float sv[KM_THREADS / 64];
  __shared__ int si[KM_THREADS / 64];
  const int t = threadIdx.x;
  int idx = step == 0 ? idx0 : idx_ptr[0];
  idx = idx < 0 ? 0 : (idx >= N ? N - 1 : idx);
  for (int d = t; d < D; d += KM_THREADS) {
    const float v = x[(long)idx * D + d];
    c[d] = v;
    if (blockIdx.x == 0) cent[(long)step * D + d] = v;
  }
  __syncthreads();
  const int i = blockIdx.x * KM_THREADS + t;
  float best = -1.f;
  int bi = 0x7fffffff;
  if (i < N) {
    const float* xr = x + (long)i * D;
    float acc = 0.f;
    for (int d = 0; d < D; ++d) acc = sq_acc(acc, xr[d], c[d]);
    const float m = step == 0 ? acc : fminf(mind[i], acc);
    mind[i] = m;
    best = m;
    bi = i;
  }
  far_block<KM_THREADS>(best, bi, sv, si);
  if (t == 0) {
    pval[blockIdx.x] = best;
    pidx[blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(256) void kmeans_pick_kernel(const float* __restrict__ pval, const int* __restrict__ pidx,
                                                          int nblocks, int* __restrict__ idx_ptr) {
  __shared__ float sv[4];
  __shared__ int si[4];
  float best = -1.f;
  int bi = 0x7fffffff;
  for (int b = threadIdx.x; b < nblocks; b += 256) far_merge(best, bi, pval[b], pidx[b]);
  far_block<256>(best, bi, sv, si);
  if (threadIdx.x == 0) idx_ptr[0] = bi;
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const float* __restrict__ x, int N, int D, int k,
                                                                   const float* __restrict__ cent,
                                                                   int* __restrict__ labels, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float cs[KM_DK][KM_MAX_K];
  __shared__ int lab[KM_THREADS];
  __shared__ float psum[KM_MAX_K][KM_THREADS];
  const int t = threadIdx.x;
  const int i0 = blockIdx.x * KM_THREADS, i = i0 + t;
  const long W = (long)k * D + k + 1;
  float* prow = part + (long)blockIdx.x * W;
  float acc[KM_MAX_K];
#pragma unroll
  for (int c = 0; c < KM_MAX_K; ++c) acc[c] = 0.f;
  for (int d0 = 0; d0 < D; d0 += KM_DK) {
    for (int e = t; e < KM_DK * KM_MAX_K; e += KM_THREADS) {
      const int d = e & (KM_DK - 1), c = e >> 4;
      cs[d][c] = (c < k && d0 + d < D) ? cent[(long)c * D + d0 + d] : 0.f;
    }
    float xv[KM_DK];
#pragma unroll
    for (int d = 0; d < KM_DK; ++d) xv[d] = (i < N && d0 + d < D) ? x[(long)i * D + d0 + d] : 0.f;
    __syncthreads();
#pragma unroll
    for (int d = 0; d < KM_DK; ++d) {  // columns past D are zero on both sides: acc + 0 is exact
#pragma unroll
      for (int c4 = 0; c4 < KM_MAX_K; c4 += 4) {
        const float4 cv = *reinterpret_cast<const float4*>(&cs[d][c4]);
        acc[c4] = sq_acc(acc[c4], xv[d], cv.x);
        acc[c4 + 1] = sq_acc(acc[c4 + 1], xv[d], cv.y);
        acc[c4 + 2] = sq_acc(acc[c4 + 2], xv[d], cv.z);
        acc[c4 + 3] = sq_acc(acc[c4 + 3], xv[d], cv.w);
      }
    }
    __syncthreads();
  }
  float best = acc[0];
  int bl = 0;
#pragma unroll
  for (int c = 1; c < KM_MAX_K; ++c)
    if (c < k && acc[c] < best) {  // strict: the lowest index wins a tie
      best = acc[c];
      bl = c;
    }
  int moved = 0;
  if (i < N) {
    moved = labels[i] != bl;
    labels[i] = bl;
  }
  lab[t] = i < N ? bl : -1;
  const int changed = __syncthreads_count(moved);
  // sums: thread t owns column dc + t of every cluster's row, points in increasing order
  for (int dc = 0; dc < D; dc += KM_THREADS) {
    const int d = dc + t;
    for (int c = 0; c < k; ++c) psum[c][t] = 0.f;
    if (d < D) {
      const int np = min(KM_THREADS, N - i0);
      for (int p = 0; p < np; ++p) psum[lab[p]][t] += x[(long)(i0 + p) * D + d];
      for (int c = 0; c < k; ++c) prow[(long)c * D + d] = psum[c][t];
    }
  }
  if (t < k) {
    int cnt = 0;
    for (int p = 0; p < KM_THREADS; ++p) cnt += lab[p] == t;
    prow[(long)k * D + t] = (float)cnt;
  }
  if (t == 0) prow[(long)k * D + k] = (float)changed;
}

__global__ __launch_bounds__(256) void kmeans_finish_kernel(const float* __restrict__ red, int D, int k,
                                                            float* __restrict__ cent, int* __restrict__ changed) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) changed[0] = (int)red[(long)k * D + k];
  if (e >= k * D) return;
  const float cnt = red[(long)k * D + e / D];
  if (cnt > 0.f) cent[e] = red[e] / cnt;
}

inline int grad_splits(int N) {  // column shares of the gradient kernel: about 1024 workgroups, at most 16 shares
  const int rows = cdiv(N, 64);
  int js = cdiv(1024, rows);
  js = js > 16 ? 16 : js;
  const int most = cdiv(N, GR_TILE);  // a share is at least one staged tile
  return js > most ? most : (js < 1 ? 1 : js);
}

}  // namespace

// floats of workspace for ssamd_tsne_affinities: the tile partials, the two-level scratch of their sum, the sum
SSAMD_API long ssamd_tsne_aff_ws(int N) {
  const long T = cdiv(N, SM_TILE);
  return T * T + seg_colsum_ws(1, 1) + 1;
}

// x [N, D] fp32 -> P [N, N] joint affinities, in place over the distance plane; joint = 0 stops at the conditional rows
SSAMD_API int ssamd_tsne_affinities(const float* x, int N, int D, float log_perp, float* P, float* ws, int joint,
                                    hipStream_t s) {
  if (N < 2 || N > SM_MAX_N || D < 1 || !x || !P || !ws) return -2;
  const int T = cdiv(N, SM_TILE);
  hipLaunchKernelGGL(tsne_pairdist_kernel, dim3(T, T), dim3(256), 0, s, x, N, D, P);
  const size_t lds = (size_t)(N + PX_RED) * sizeof(float);
  allow_lds(tsne_perplexity_kernel, lds);
  hipLaunchKernelGGL(tsne_perplexity_kernel, dim3(N), dim3(256), lds, s, P, N, log_perp);
  if (!joint) return (int)hipGetLastError();
  float* part = ws;
  float* scratch = ws + (long)T * T;
  float* total = scratch + seg_colsum_ws(1, 1);
  hipLaunchKernelGGL(tsne_planesum_kernel, dim3(T, T), dim3(256), 0, s, P, N, part);
  const int rc = ssamd_seg_colsum(part, 1, 1, T * T, 1, total, 1, 0, 1, nullptr, scratch, seg_colsum_ws(1, 1), s);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(tsne_symmetrise_kernel, dim3(T, T), dim3(256), 0, s, P, N, total);
  return (int)hipGetLastError();
}

// floats of workspace for ssamd_tsne_iter: the reduced planes [6][N], then the shares' partials
SSAMD_API long ssamd_tsne_iter_ws(int N) {
  const int js = grad_splits(N);
  return (long)SM_PLANES * N * (1 + (js > 1 ? js : 0));
}

// One gradient evaluation at y [N, 2] and, with do_update, one descent step.  ws[0 .. 6N) receives the planes attr x,
// attr y, rep x, rep y, zrow, KL part.  grad_out [N, 2] and kl_slot (one float: KL(P || Q) at y) may be null.
SSAMD_API int ssamd_tsne_iter(const float* P, float* y, int N, float* ws, float exag, float momentum, float lr,
                              float* upd, float* gains, float* grad_out, float* kl_slot, int do_update,
                              hipStream_t s) {
  if (N < 2 || N > SM_MAX_N || !P || !y || !ws) return -2;
  if (do_update && (!upd || !gains)) return -2;
  const int js = grad_splits(N);
  const int jchunk = cdiv(cdiv(N, js), GR_TILE) * GR_TILE;
  float* red = ws;
  float* part = js > 1 ? ws + (long)SM_PLANES * N : ws;
  hipLaunchKernelGGL(tsne_grad_kernel, dim3(cdiv(N, 64), js), dim3(256), 0, s, P, y, N, jchunk, part,
                     kl_slot ? 1 : 0);
  if (js > 1) {
    const int rc = ssamd_seg_colsum(part, (long)SM_PLANES * N, 1, js, SM_PLANES * N, red, (long)SM_PLANES * N, 0,
                                    SM_PLANES * N, nullptr, nullptr, 0, s);
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(tsne_update_kernel, dim3(cdiv(2L * N, 256)), dim3(256), 0, s, red, N, exag, momentum, lr, y, upd,
                     gains, grad_out, kl_slot, do_update);
  return (int)hipGetLastError();
}

// floats of workspace for the k-means entry points: a partial row per workgroup, the reduced row, the start's
// nearest-centre distances and block maxima
SSAMD_API long ssamd_kmeans_ws(int N, int D, int k) {
  const long W = (long)k * D + k + 1, B = cdiv(N, KM_THREADS);
  return B * W + W + N + 2 * B + 4;
}

// farthest-point start: cent [k, D]
SSAMD_API int ssamd_kmeans_init(const float* x, int N, int D, int k, int idx0, float* cent, float* ws, hipStream_t s) {
  if (N < 1 || k < 1 || k > KM_MAX_K || k > N || D < 1 || D > KM_MAX_D || !x || !cent || !ws) return -2;
  const long W = (long)k * D + k + 1, B = cdiv(N, KM_THREADS);
  float* mind = ws + B * W + W;
  float* pval = mind + N;
  int* pidx = reinterpret_cast<int*>(pval + B);
  int* idx_ptr = pidx + B;
  for (int c = 0; c < k; ++c) {
    hipLaunchKernelGGL(kmeans_far_kernel, dim3(B), dim3(KM_THREADS), 0, s, x, N, D, idx0, idx_ptr, c, cent, mind, pval,
                       pidx);
    if (c + 1 < k) hipLaunchKernelGGL(kmeans_pick_kernel, dim3(1), dim3(256), 0, s, pval, pidx, (int)B, idx_ptr);
  }
  return (int)hipGetLastError();
}

// one Lloyd step: labels [N] int32 in / out, cent [k, D] in / out, changed[0] = labels that moved
SSAMD_API int ssamd_kmeans_step(const float* x, int N, int D, int k, float* cent, int* labels, int* changed, float* ws,
                                hipStream_t s) {
  if (N < 1 || k < 1 || k > KM_MAX_K || k > N || D < 1 || D > KM_MAX_D || !x || !cent || !labels || !changed || !ws)
    return -2;
  const long W = (long)k * D + k + 1, B = cdiv(N, KM_THREADS);
  float* part = ws;
  float* red = ws + B * W;
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3(B), dim3(KM_THREADS), 0, s, x, N, D, k, cent, labels, part);
  const int rc = ssamd_seg_colsum(part, W, 1, (int)B, (int)W, red, W, 0, (int)W, nullptr, nullptr, 0, s);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(kmeans_finish_kernel, dim3(cdiv((long)k * D, 256)), dim3(256), 0, s, red, D, k, cent, changed);
  return (int)hipGetLastError();
}

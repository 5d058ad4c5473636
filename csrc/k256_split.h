// Work split of the weight-stationary K = 256 GEMM (k_gemm.hip, conv_gemm_k256_kernel): plain integer
// arithmetic shared by the kernel and the host, checked on the CPU by selftest_k256_split.cpp.
//
// The grid is ng = N / 256 column groups of nb blocks each.  The M rows are cut into 64-row chunks and the
// chunks of a column group are dealt to its nb blocks as contiguous ranges, equal to within one chunk.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define K256_HD __host__ __device__
#else
#define K256_HD
#endif

constexpr int K256_ROWS = 64;  // rows per chunk

K256_HD inline int k256_chunks(int M) { return (M + K256_ROWS - 1) / K256_ROWS; }

// blocks per column group for a budget of `blocks` blocks: every group gets the same count (at least one,
// so the grid may exceed a budget smaller than ng), never more blocks than chunks
K256_HD inline int k256_blocks_per_group(int blocks, int ng, int nch) {
  int nb = blocks / ng;
  if (nb < 1) nb = 1;
  if (nb > nch) nb = nch;
  return nb < 1 ? 1 : nb;
}

// chunk range [c0, c1) of block r (0 <= r < nb) of a column group: the first nch % nb blocks hold one more
K256_HD inline void k256_chunk_range(int nch, int nb, int r, int* c0, int* c1) {
  const int q = nch / nb, rem = nch - q * nb;
  *c0 = r * q + (r < rem ? r : rem);
  *c1 = *c0 + q + (r < rem ? 1 : 0);
}

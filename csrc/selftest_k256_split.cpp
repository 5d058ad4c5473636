// Host self-test of the K = 256 GEMM work split (k256_split.h): for every row count, column-group count
// and block budget the chunk ranges of a column group's blocks must tile [0, chunks) contiguously, in
// order, without gaps or overlap, differ in length by at most one chunk, and leave no block without rows.
#include <cstdio>

#include "k256_split.h"

static int fails = 0;
#define CHECK(c, ...)                         \
  do {                                        \
    if (!(c)) {                               \
      if (++fails <= 20) {                    \
        std::printf("FAIL %s: ", #c);         \
        std::printf(__VA_ARGS__);             \
        std::printf("\n");                    \
      }                                       \
    }                                         \
  } while (0)

int main() {
  const int Ms[] = {1, 63, 64, 65, 127, 128, 255, 257, 1001, 4097, 14336, 100352, 100353, 1 << 20};
  const int budgets[] = {1, 2, 3, 4, 5, 7, 8, 64, 255, 256, 304, 1024};
  for (int M : Ms)
    for (int ng = 1; ng <= 8; ++ng)
      for (int blocks : budgets) {
        const int nch = k256_chunks(M);
        CHECK(nch >= 1 && (long)nch * K256_ROWS >= M && (long)(nch - 1) * K256_ROWS < M, "chunks %d of M %d", nch, M);
        const int nb = k256_blocks_per_group(blocks, ng, nch);
        CHECK(nb >= 1 && nb <= nch, "nb %d nch %d (M %d ng %d blocks %d)", nb, nch, M, ng, blocks);
        CHECK(nb * ng <= blocks || nb == 1, "grid %d over the budget %d (M %d ng %d)", nb * ng, blocks, M, ng);
        int next = 0, lo = nch, hi = 0;
        for (int r = 0; r < nb; ++r) {
          int c0, c1;
          k256_chunk_range(nch, nb, r, &c0, &c1);
          CHECK(c0 == next && c1 > c0 && c1 <= nch, "block %d of %d: [%d, %d) after %d (nch %d)", r, nb, c0, c1, next,
                nch);
          next = c1;
          if (c1 - c0 < lo) lo = c1 - c0;
          if (c1 - c0 > hi) hi = c1 - c0;
        }
        CHECK(next == nch, "ranges end at %d of %d (nb %d)", next, nch, nb);
        CHECK(hi - lo <= 1, "ranges of %d .. %d chunks (nch %d nb %d)", lo, hi, nch, nb);
      }
  if (fails) {
    std::printf("selftest_k256_split: %d failures\n", fails);
    return 1;
  }
  std::printf("selftest_k256_split ok\n");
  return 0;
}

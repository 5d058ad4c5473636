// Host self-test of the attention block map (attn_blockmap.h): for every gx in 1..16 and BH in
// 1..40 the map must be a bijection of the launched ids onto (bh < BH, x < gx) plus idle ids, keep
// all x-blocks of a (b, h) on one id residue mod 8 and put consecutive (b, h) on different ones.
#include <cstdio>
#include <vector>

#include "attn_blockmap.h"

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
  for (int xcd = 0; xcd <= 1; ++xcd)
    for (int gx = 1; gx <= 16; ++gx)
      for (int BH = 1; BH <= 40; ++BH) {
        const long n = attn_map_grid(gx, BH);
        CHECK(n >= (long)gx * BH && n % gx == 0 && (n / gx) % kAttnXcds == 0 && n / gx < BH + kAttnXcds,
              "grid %ld gx %d BH %d", n, gx, BH);
        std::vector<int> seen((size_t)gx * BH, 0), res(BH, -1);
        for (long id = 0; id < n; ++id) {
          const AttnBlock b = attn_block_map((int)id, gx, xcd);
          CHECK(b.bh >= 0 && b.x >= 0 && b.x < gx, "id %ld -> (%d, %d) gx %d BH %d xcd %d", id, b.bh, b.x, gx, BH, xcd);
          if (b.bh < 0 || b.bh >= BH || b.x < 0 || b.x >= gx) continue;  // idle id: the block exits
          ++seen[(size_t)b.bh * gx + b.x];
          if (xcd) {  // all x of one bh share id % 8
            const int r = (int)(id % kAttnXcds);
            CHECK(res[b.bh] < 0 || res[b.bh] == r, "bh %d on residues %d and %d (gx %d BH %d)", b.bh, res[b.bh], r, gx, BH);
            res[b.bh] = r;
          }
        }
        for (int bh = 0; bh < BH; ++bh)
          for (int x = 0; x < gx; ++x)  // exactly once; an extra id with bh < BH would show as 2
            CHECK(seen[(size_t)bh * gx + x] == 1, "(%d, %d) produced %d times (gx %d BH %d xcd %d)", bh, x,
                  seen[(size_t)bh * gx + x], gx, BH, xcd);
        if (xcd)
          for (int bh = 0; bh + 1 < BH; ++bh)
            CHECK(res[bh] != res[bh + 1], "bh %d and %d share residue %d (gx %d BH %d)", bh, bh + 1, res[bh], gx, BH);
      }
  if (fails) {
    std::printf("selftest_attn_blockmap: %d failures\n", fails);
    return 1;
  }
  std::printf("selftest_attn_blockmap ok\n");
  return 0;
}

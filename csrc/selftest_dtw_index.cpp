// Host self-test of the DTW direction-plane index arithmetic (dtw_index.h).  For a few dozen shapes (1 x 1,
// 1 x N, N x 1, strip and block edges): a scalar DTW that stores its directions through dtw_dir_index into a
// buffer of exactly dtw_plane_bytes bytes (ASan watches the bounds) and walks back through the same header gives
// the total and the path of a plain 2-D-array DTW; every cell has a byte of its own inside the plane; and the
// (strip, block, lane, step) enumeration the kernel stores by covers every byte of the plane exactly once.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <utility>
#include <vector>

#include "dtw_index.h"

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

typedef std::vector<std::pair<int, int>> Path;

// integer-valued local cost with many ties (the tie rule decides the path)
static int local_cost(int i, int j, unsigned seed) {
  unsigned h = (unsigned)i * 2654435761u ^ ((unsigned)j * 40503u + seed);
  h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
  return (int)(h % 3u);
}

static int pick(long diag, long up, long left, long* best) {
  int dir = DTW_DIAG;
  *best = diag;
  if (up < *best) { *best = up; dir = DTW_UP; }
  if (left < *best) { *best = left; dir = DTW_LEFT; }
  return dir;
}

static const long INF = std::numeric_limits<long>::max() / 4;

// plain 2-D arrays
static long dtw_plain(int Tx, int Ty, unsigned seed, Path* path) {
  std::vector<std::vector<long>> A((size_t)Tx, std::vector<long>((size_t)Ty, 0));
  std::vector<std::vector<uint8_t>> Dr((size_t)Tx, std::vector<uint8_t>((size_t)Ty, 0));
  for (int i = 0; i < Tx; ++i)
    for (int j = 0; j < Ty; ++j) {
      long best;
      const long diag = (i > 0 && j > 0) ? A[i - 1][j - 1] : (i == 0 && j == 0 ? 0 : INF);
      const int dir = pick(diag, i > 0 ? A[i - 1][j] : INF, j > 0 ? A[i][j - 1] : INF, &best);
      A[i][j] = local_cost(i, j, seed) + best;
      Dr[i][j] = (uint8_t)dir;
    }
  path->clear();
  for (int i = Tx - 1, j = Ty - 1;;) {
    path->push_back({i, j});
    if (i == 0 && j == 0) break;
    const int dir = Dr[i][j];
    if (dir != DTW_LEFT) --i;
    if (dir != DTW_UP) --j;
  }
  std::reverse(path->begin(), path->end());
  return A[Tx - 1][Ty - 1];
}

// the same recurrence with the directions stored and read back through the header
static long dtw_indexed(int Tx, int Ty, unsigned seed, Path* path) {
  const long long nbytes = dtw_plane_bytes(Tx, Ty);
  std::vector<uint8_t> plane((size_t)nbytes, 0xff);
  std::vector<long> prev((size_t)Ty, INF), cur((size_t)Ty, INF);
  for (int i = 0; i < Tx; ++i) {
    for (int j = 0; j < Ty; ++j) {
      long best;
      const long diag = (i > 0 && j > 0) ? prev[j - 1] : (i == 0 && j == 0 ? 0 : INF);
      const int dir = pick(diag, i > 0 ? prev[j] : INF, j > 0 ? cur[j - 1] : INF, &best);
      cur[j] = local_cost(i, j, seed) + best;
      const long long at = dtw_dir_index(i, j, Ty);
      CHECK(at >= 0 && at < nbytes, "%d x %d: cell (%d, %d) at %lld of %lld", Tx, Ty, i, j, at, nbytes);
      if (at < 0 || at >= nbytes) return -1;
      CHECK(plane[(size_t)at] == 0xff, "%d x %d: cell (%d, %d) shares byte %lld", Tx, Ty, i, j, at);
      plane[(size_t)at] = (uint8_t)dir;
    }
    std::swap(prev, cur);
  }
  path->clear();
  for (int i = Tx - 1, j = Ty - 1;;) {
    path->push_back({i, j});
    if (i == 0 && j == 0) break;
    CHECK(i >= 0 && j >= 0 && (int)path->size() <= Tx + Ty - 1, "%d x %d: walk left the matrix", Tx, Ty);
    if (i < 0 || j < 0 || (int)path->size() > Tx + Ty - 1) return -1;
    dtw_step_back(plane[(size_t)dtw_dir_index(i, j, Ty)], i, j);
  }
  std::reverse(path->begin(), path->end());
  return prev[Ty - 1];
}

// the kernel's store order: strip, block, 4-step group, lane -> one dword; every byte of the plane exactly once,
// and the byte of a cell inside the matrix is the one dtw_dir_index names
static void check_cover(int Tx, int Ty) {
  const long long nbytes = dtw_plane_bytes(Tx, Ty);
  std::vector<uint8_t> seen((size_t)nbytes, 0);
  const int nstrip = dtw_num_strips(Tx), nblk = dtw_num_blocks(Ty);
  CHECK(nblk * DTW_BLOCK >= dtw_num_steps(Ty) && (nblk - 1) * DTW_BLOCK < dtw_num_steps(Ty), "%d blocks for Ty %d", nblk, Ty);
  CHECK(nstrip * DTW_STRIP >= Tx && (nstrip - 1) * DTW_STRIP < Tx, "%d strips for Tx %d", nstrip, Tx);
  for (int s = 0; s < nstrip; ++s)
    for (int b = 0; b < nblk; ++b)
      for (int u4 = 0; u4 < DTW_BLOCK / 4; ++u4)
        for (int l = 0; l < DTW_STRIP; ++l) {
          const long long dword = ((long long)(s * nblk + b) * (DTW_BLOCK / 4) + u4) * DTW_STRIP + l;
          for (int k = 0; k < 4; ++k) {
            const long long at = dword * 4 + k;
            CHECK(at >= 0 && at < nbytes, "%d x %d: store at %lld of %lld", Tx, Ty, at, nbytes);
            if (at < 0 || at >= nbytes) return;
            CHECK(!seen[(size_t)at], "%d x %d: byte %lld stored twice", Tx, Ty, at);
            seen[(size_t)at] = 1;
            const int i = s * DTW_STRIP + l, j = b * DTW_BLOCK + u4 * 4 + k - l;
            if (i < Tx && j >= 0 && j < Ty)
              CHECK(dtw_dir_index(i, j, Ty) == at, "%d x %d: cell (%d, %d) stored at %lld, read at %lld", Tx, Ty, i, j,
                    at, dtw_dir_index(i, j, Ty));
          }
        }
  for (long long at = 0; at < nbytes; ++at) CHECK(seen[(size_t)at], "%d x %d: byte %lld never stored", Tx, Ty, at);
}

int main() {
  const int edge[] = {1, 2, 3, 5, 63, 64, 65, 127, 128, 129, 200};
  std::vector<std::pair<int, int>> shapes;
  for (int a : edge)
    for (int b : {1, 2, 63, 64, 65, 129}) shapes.push_back({a, b});
  for (int n : {7, 64, 300}) {
    shapes.push_back({1, n});
    shapes.push_back({n, 1});
  }
  shapes.push_back({257, 300});
  shapes.push_back({130, 67});
  long cells = 0;
  for (const auto& sh : shapes) {
    const int Tx = sh.first, Ty = sh.second;
    check_cover(Tx, Ty);
    for (unsigned seed = 0; seed < 2; ++seed) {
      Path a, b;
      const long ta = dtw_plain(Tx, Ty, seed, &a), tb = dtw_indexed(Tx, Ty, seed, &b);
      CHECK(ta == tb, "%d x %d: total %ld vs %ld", Tx, Ty, ta, tb);
      CHECK(a == b, "%d x %d: paths differ (%zu vs %zu cells)", Tx, Ty, a.size(), b.size());
      CHECK(a.front() == std::make_pair(0, 0) && a.back() == std::make_pair(Tx - 1, Ty - 1), "%d x %d: ends", Tx, Ty);
    }
    cells += (long)Tx * Ty;
  }
  // the 64-bit plane size: a pair whose plane passes 2^31 bytes
  CHECK(dtw_plane_bytes(60000, 60000) == (long long)dtw_num_strips(60000) * dtw_num_blocks(60000) * 4096LL &&
            dtw_plane_bytes(60000, 60000) > 2147483647LL, "plane bytes overflow");
  CHECK(dtw_dir_index(59999, 59999, 60000) < dtw_plane_bytes(60000, 60000) &&
            dtw_dir_index(59999, 59999, 60000) > 2147483647LL, "last cell of a large pair");
  if (fails) {
    std::printf("selftest_dtw_index: %d failures\n", fails);
    return 1;
  }
  std::printf("selftest_dtw_index ok (%zu shapes, %ld cells)\n", shapes.size(), cells);
  return 0;
}

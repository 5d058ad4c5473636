// Direction-plane index arithmetic of the DTW kernels (k_dtw.hip), shared with host code.
//
// The forward kernel runs an anti-diagonal wavefront over strips of DTW_STRIP = 64 rows: lane l of the
// wave owns row i = 64 s + l of strip s and visits column j at wavefront step t = j + l, so a strip of a
// pair with Ty columns takes steps 0 .. Ty + 62.  Steps are grouped in blocks of DTW_BLOCK = 64; a strip
// has dtw_num_blocks(Ty) of them.  One (strip, block) tile of the direction plane is 64 lanes x 64 steps
// = 4096 bytes, laid out so that a lane's 4 consecutive steps are one aligned dword and the 64 lanes'
// dwords of those 4 steps are 256 consecutive bytes (one coalesced store per 4 steps):
//
//   byte of cell (i, j) = tile * 4096 + (((t % 64) / 4) * 64 + l) * 4 + t % 4,   tile = s * blocks + t / 64
//
// Cells outside the Tx x Ty matrix that the wavefront passes over (j < 0, j >= Ty, i >= Tx) have bytes
// too (the kernel writes 0 there); every byte of the plane is written by exactly one (lane, step).
// Direction codes: 0 = from (i-1, j-1), 1 = from (i-1, j), 2 = from (i, j-1).
// A pair's plane starts at a 64-bit byte offset (the sum of the planes before it in the launch).
// Everything here is pure integer arithmetic: csrc/selftest_dtw_index.cpp proves it on the CPU.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DTW_HD __host__ __device__
#else
#define DTW_HD
#endif

#define DTW_STRIP 64
#define DTW_BLOCK 64
#define DTW_TILE_BYTES (DTW_STRIP * DTW_BLOCK)
#define DTW_DIAG 0
#define DTW_UP 1
#define DTW_LEFT 2

// strips of 64 rows of a pair with Tx >= 1 rows
DTW_HD inline int dtw_num_strips(int Tx) { return (Tx + DTW_STRIP - 1) / DTW_STRIP; }

// wavefront steps of one strip (lane 63 reaches column Ty - 1 at step Ty + 62) and the 64-step blocks holding them
DTW_HD inline int dtw_num_steps(int Ty) { return Ty + DTW_STRIP - 1; }
DTW_HD inline int dtw_num_blocks(int Ty) { return (dtw_num_steps(Ty) + DTW_BLOCK - 1) / DTW_BLOCK; }

// bytes of a pair's direction plane
DTW_HD inline long long dtw_plane_bytes(int Tx, int Ty) {
  return (long long)dtw_num_strips(Tx) * dtw_num_blocks(Ty) * DTW_TILE_BYTES;
}

// tile (strip, block) of cell (i, j) and the byte inside it; lane l at in-block step u
DTW_HD inline long long dtw_tile(int i, int j, int Ty) {
  return (long long)(i / DTW_STRIP) * dtw_num_blocks(Ty) + (j + i % DTW_STRIP) / DTW_BLOCK;
}
DTW_HD inline int dtw_tile_byte(int l, int u) { return ((u >> 2) * DTW_STRIP + l) * 4 + (u & 3); }
DTW_HD inline int dtw_cell_byte(int i, int j) { return dtw_tile_byte(i % DTW_STRIP, (j + i % DTW_STRIP) % DTW_BLOCK); }

// byte of cell (i, j), 0 <= i < Tx, 0 <= j < Ty, relative to the pair's plane
DTW_HD inline long long dtw_dir_index(int i, int j, int Ty) {
  return dtw_tile(i, j, Ty) * DTW_TILE_BYTES + dtw_cell_byte(i, j);
}

// one backward step of the path walk
DTW_HD inline void dtw_step_back(int dir, int& i, int& j) {
  if (dir != DTW_LEFT) --i;
  if (dir != DTW_UP) --j;
}

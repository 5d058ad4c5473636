// Block placement of the D = 128 attention kernels: linear block id -> ((b, h) index, x-block).
//
// Workgroups are dealt round-robin over the 8 XCDs by linear id and the XCD L2s are not
// shared, while every x-block of one (b, h) streams the same tiles of that sequence.  The
// map puts all gx x-blocks of a (b, h) on ids of one residue mod 8 (one XCD), dispatched back
// to back, and deals consecutive (b, h) round-robin over the residues (sequences come sorted
// by length in groups, so contiguous ranges per XCD would unbalance them).  It is a bijection
// of the gx * roundup(BH, 8) ids onto (bh < roundup(BH, 8), x < gx): ids whose bh >= BH have
// no work and exit.  Correctness never depends on where a block runs.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ATTN_MAP_HD __host__ __device__
#else
#define ATTN_MAP_HD
#endif

constexpr int kAttnXcds = 8;

struct AttnBlock {
  int bh;  // (b, h) index; >= BH: the block has no work
  int x;   // x-block of that (b, h), 0 .. gx-1
};

// blocks to launch for BH (b, h) pairs of gx x-blocks each (both placements)
ATTN_MAP_HD inline long attn_map_grid(int gx, int BH) {
  return (long)gx * ((BH + kAttnXcds - 1) / kAttnXcds * kAttnXcds);
}

// xcd = 0: the plain order (x fastest, as a (gx, BH) grid numbers its blocks)
ATTN_MAP_HD inline AttnBlock attn_block_map(int id, int gx, int xcd) {
  AttnBlock r;
  if (xcd) {
    const int slot = id / kAttnXcds;
    r.bh = (slot / gx) * kAttnXcds + id % kAttnXcds;
    r.x = slot % gx;
  } else {
    r.bh = id / gx;
    r.x = id % gx;
  }
  return r;
}

// The persistent work plan of the two polyphase dilation-group kernels (conv_wino_rs.hip, conv_bf16_dg.hip).  A workgroup owns one block of
// 16 output channels of one image for a whole CHUNK of items; an item is 8 rows of one row-residue class (rows ry, ry + d, ...) by 32 image
// columns of the block's group.  Chunk j of J owns items j, j + J, ...; the (image, chunk) pairs are the KEYS, dealt out so that the
// workgroups of one XCD (workgroup id % 8) walk neighbouring keys and every block of a key.
#pragma once
#include "conv_kernel.h"

namespace vspconv {

struct ItemPlan {
  int nwg;          // workgroups launched (multiple of 8)
  int J;            // chunks per (image, block): chunk j owns items j, j + J, ...
  int nblk;         // 16-channel blocks per image
  int nkeys, kx;    // keys = (image, chunk) pairs; keys per XCD
  int cbk;          // column blocks of 32 per image row
  int cbk_shift;    // log2(cbk) when it is a power of two, else -1
  int n_items[4];   // items of a block of group g: d * row blocks * cbk
};

// nblk: blocks per image; wgs: the kernel's tuning variable (workgroups to launch; <= 0: two per CU)
inline ItemPlan item_plan(const ConvK& q, int nblk, int wgs) {
  ItemPlan pl{};
  pl.nblk = nblk;
  pl.cbk = (q.W + 31) / 32;
  pl.cbk_shift = (pl.cbk & (pl.cbk - 1)) == 0 ? __builtin_ctz(pl.cbk) : -1;
  int nmax = 0;
  for (int g = 0; g < q.G; ++g) {
    const int d = q.dil[g];
    const int sh = (q.H + d - 1) / d;
    pl.n_items[g] = d * ((sh + 7) / 8) * pl.cbk;
    nmax = pl.n_items[g] > nmax ? pl.n_items[g] : nmax;
  }
  pl.nwg = wgs > 0 ? (wgs + 7) / 8 * 8 : 2 * vsp::kNumCU;
  // chunks per (image, block): about one chunk per workgroup slot, at least ~2 items per chunk, keys a multiple of 8 when they fill the XCDs
  int J = pl.nwg / (q.B * pl.nblk);
  J = J < 1 ? 1 : J;
  if (J > (nmax + 1) / 2) J = (nmax + 1) / 2;
  J = J < 1 ? 1 : J;
  pl.J = J;
  pl.nkeys = q.B * J;
  pl.kx = (pl.nkeys + 7) / 8;
  const int chunks = pl.nkeys * pl.nblk;
  if (chunks < pl.nwg) pl.nwg = (chunks + 7) / 8 * 8;
  return pl;
}

// step m of the walk of XCD xcd -> key (past nkeys: the walk is over), block; key -> image b, first item j0
struct ItemChunk {
  int key, blk, b, j0;
};
__device__ __forceinline__ ItemChunk item_chunk(const ItemPlan& pl, int xcd, int m) {
  ItemChunk c;
  c.key = xcd * pl.kx + m / pl.nblk;
  c.blk = m % pl.nblk;
  c.b = c.key / pl.J;
  c.j0 = c.key - c.b * pl.J;
  return c;
}

// item it of a group of dilation d = 1 << dl -> column block it % cbk, t = it / cbk -> row residue t % d, row block t / d
__device__ __forceinline__ void item_xy(const ItemPlan& pl, int it, int d, int dl, int& ry, int& oy0, int& X0) {
  const int t = pl.cbk_shift >= 0 ? it >> pl.cbk_shift : it / pl.cbk;
  const int cbi = it - t * pl.cbk;
  ry = t & (d - 1);
  oy0 = 8 * (t >> dl);
  X0 = 32 * cbi;
}

}  // namespace vspconv

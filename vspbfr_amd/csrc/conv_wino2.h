// What the three fp32 Winograd F(2x2, 3x3) kernels share -- the task list (conv_wino.hip), the row owner (conv_wino_ro.hip) and the row owner
// for dilation groups (conv_wino_rod.hip): tile geometry, the scalar-cache operand load, the XCD-aware work order, the epilogue (the row
// owner runs its parts around a 16-byte store form of its own), the patch / U staging of the two row-owner kernels and the host side's
// grid set-up and eligibility test.  Only those three files include this header.
// Everything device-side is __forceinline__ and takes the kernel's parameter block BY VALUE (by reference the kernarg fields are reloaded at
// every use instead of kept: three times the s_load count on the dilation-group kernel).
#pragma once
#include "conv_kernel.h"

namespace vspconv {

// Geometry every form shares: MBW 16-channel blocks x NBW 16-tile blocks per wave and position, MBW * NBW = 8 (64 accumulator registers).
// The kernels derive from it and add what is theirs (tile columns, patch and V pitches, channels per interval).
template <int MBW>
struct Wino2Tile {
  static constexpr int NBW = 8 / MBW;
  static constexpr int WCO = 16 * MBW;
  static constexpr int NTILE = 16 * NBW;
  static constexpr int ETILE = NTILE > 64 ? 64 : NTILE;  // tiles per epilogue pass
  static constexpr int EMB = (MBW >= 2 && ETILE <= 32) ? 2 : 1;  // 16-channel blocks per epilogue pass
  static constexpr int EP = ETILE + 4;                // epilogue row pitch: 4 rows (one k-slot group) = 16 banks
  static constexpr int LDS_M = 16 * 16 * EMB * EP;
  static constexpr int UF = 2 * MBW;                  // U floats per lane and chunk: [pp 2][mb MBW]
};

constexpr int WINO2_RO_IVC = 8;   // row-owner kernels: input channels per sub-stage, one channel plane per wave

// Wave-uniform operand through the scalar cache, whatever the compiler can prove about the index: the constant address space
// makes the load an s_load (lgkmcnt).  As a per-lane global load it joins vmcnt and drags the latency of every prefetch in
// flight into the interval (measured: 674 -> 802 us on 512 -> 512 at 64^2 when an unrelated edit flipped the compiler's choice).
__device__ __forceinline__ float uload(const float* base, int idx) {
  typedef const float __attribute__((address_space(4))) * cfp4;
  return ((cfp4)(uintptr_t)base)[__builtin_amdgcn_readfirstlane(idx)];
}

// ---- XCD-aware work order.  The dispatcher deals workgroups round-robin over the 8 XCDs (each with its own 4 MB L2), so in
// dispatch order every L2 sees every pixel tile and every channel tile.  Bijective remap: XCD x walks a CONTIGUOUS range of
// the work list, ordered either
//   1 = pixel-tile-major (image, pixel tile, channel tile): neighbouring tiles share their halo (40 % of a 10 x 18 patch)
//       and the channel tiles of one pixel tile read the same patch -- right when U is small (<= 64 channels), or
//   2 = channel-tile-major (channel tile, image, pixel tile): a workgroup streams its whole U slice (64 co x Cin x 16
//       positions x 4 B = 2 MB at 512 channels) and NO two waves share any of it, so U is the kernel's dominant fetch
//       (32 KB per 8-channel interval against 5.8 KB of patch: 4.3 GB per 512 -> 512 launch at 64^2, ~5 TB/s).  In
//       pixel-major order all 8 channel tiles (16.8 MB) compete for one 4 MB L2 and U streams from MALL / HBM; in
//       channel-major order an XCD works on one or two channel tiles at a time and U stays L2-resident.
//   4 = region-major (shared-input dilation groups, as in conv_bf16.hip): a region = one image band of 8 x 2 TLY rows x 4 column
//       tiles; for every dilation d | 8 exactly 8 workgroups per column tile cover it (d residues x 8/d row tiles), and the four
//       groups of a region run back to back on one XCD instead of never meeting in an L2.
// xcd_linear_id() is this workgroup's place in the remapped list; the decodes turn it into (image b, pixel block bx, channel block by).
__device__ __forceinline__ int xcd_linear_id() {
  const int GX = gridDim.x, GY = gridDim.y, GZ = gridDim.z, GT = GX * GY * GZ;
  const int wgid = blockIdx.x + GX * (blockIdx.y + GY * blockIdx.z);
  const int xcd = wgid & 7, xq = GT >> 3, xr = GT & 7;
  return (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (wgid >> 3);
}

__device__ __forceinline__ void decode_pixel_major(int lid, int& b, int& bx, int& by) {     // order 1
  const int GX = gridDim.x, GY = gridDim.y;
  const int GN = GX * GY;
  b = lid / GN;
  const int lrem = lid - b * GN;
  bx = lrem / GY;
  by = lrem - bx * GY;
}

__device__ __forceinline__ void decode_channel_major(int lid, int& b, int& bx, int& by) {   // order 2
  const int GX = gridDim.x, GZ = gridDim.z;
  const int GN = GX * GZ;
  by = lid / GN;
  const int lrem = lid - by * GN;
  b = lrem / GX;
  bx = lrem - b * GX;
}

// order 4 -> image, channel block, and the workgroup's residue class / tile row / tile column (p.tiles_y, p.tiles_x: wino2_region_major)
__device__ __forceinline__ void decode_region_major(const ConvK p, int lid, int& b, int& by, int& reg_ry, int& reg_ty, int& reg_tx) {
  constexpr int CGX = 4;
  const int GY = gridDim.y;
  const int nb = p.tiles_y, ncg = p.tiles_x;                 // (host: bands per image, column groups per band)
  const int per_region = GY * 8 * CGX;
  const int region = lid / per_region, w = lid - region * per_region;
  b = region / (nb * ncg);
  const int rr = region - b * (nb * ncg);
  const int band = rr / ncg, cg = rr - band * ncg;
  const int slot = w / (GY * CGX), w2 = w - slot * (GY * CGX);
  const int cx = w2 / GY;
  by = w2 - cx * GY;
  const int dg = p.dil[by / p.co_tiles];
  reg_ry = slot % dg;
  reg_ty = band * (8 / dg) + slot / dg;
  reg_tx = cg * CGX + cx;
}

// Row-polyphase tile of a workgroup of a group with dilation d: residue class ry (rows ry, ry + d, ...), tile row / column within it, from
// the region-major decode (reg_ry >= 0) or from the pixel block bx.  false: a spare block, the workgroup has nothing to do.
template <int TLX, int TLY>
__device__ __forceinline__ bool wino2_tile(const ConvK p, int d, int bx, int reg_ry, int reg_ty, int reg_tx, int& ry, int& ty_i, int& tx_i) {
  const int SH = (p.H + d - 1) / d;                           // rows of one residue class
  const int tiles_x = (p.W + 2 * TLX - 1) / (2 * TLX), tiles_y = (SH + 2 * TLY - 1) / (2 * TLY);
  const int per_res = tiles_x * tiles_y;
  if (reg_ry >= 0) {
    if (reg_ty >= tiles_y || reg_tx >= tiles_x) return false;  // (bands / column groups that the image does not fill)
    ry = reg_ry; ty_i = reg_ty; tx_i = reg_tx;
  } else {
    if (bx >= per_res * d) return false;                       // (row counts that d does not divide leave a few spare blocks)
    ry = bx / per_res;
    const int tile_i = bx - ry * per_res;
    tx_i = tile_i % tiles_x;
    ty_i = tile_i / tiles_x;
  }
  return true;
}

// ---- epilogue: per 16-channel block(s) and (at most) 64 tiles, all sixteen positions through LDS, one thread per (channel, tile):
//      Y = A^T M A, then the fused operand chain of the direct kernel; the pixels of a tile lie d apart, on rows (sy + i) d + ry.
struct Wino2Out {   // this image's operand planes
  const float *osp, *nzp, *r1b, *r2b;
  float* yb;
  float nw;
  int y_plane;
  bool pairs;       // (uniform) the two pixels of a tile row are neighbours in memory, in all of output, residuals and noise, and rows hold whole pairs
};

__device__ __forceinline__ Wino2Out wino2_out(const ConvK p, int b, int d) {
  Wino2Out o;
  const int Cout = p.G * p.cout_g;
  o.osp = p.osp + (int64_t)b * Cout * p.oss;
  o.nzp = p.nzp + (int64_t)b * p.OH * p.OW * p.nzs;
  o.nw = p.nwp[0];
  o.yb = p.y + ((int64_t)b * p.y_ch + p.y_coff) * p.y_h * p.y_w;
  o.r1b = p.r1p + ((int64_t)b * p.res_ch + p.res_coff) * p.y_h * p.y_w * p.r1s;
  o.r2b = p.r2p + ((int64_t)b * p.res_ch + p.res_coff) * p.y_h * p.y_w * p.r2s;
  o.y_plane = p.y_h * p.y_w;
  o.pairs = d == 1 && p.r1s <= 1 && p.r2s <= 1 && (p.OW & 1) == 0 && p.OW >= 2;
  return o;
}

// the accumulators of channel blocks mb0 .. mb0 + EMB - 1 and tile half th -> Ml [16 pos][16 EMB co][EP]: rows padded so that the four
// k-slot groups of a store land 16 banks apart
template <int MBW, int NBW, int ETILE, int EMB, int EP>
__device__ __forceinline__ void wino2_exchange(float* Ml, const f32x4 (&acc)[2][MBW][NBW], int mb0, int th, int wave, int lr, int kq) {
  constexpr int ENB = ETILE / 16, ECO = 16 * EMB;
#pragma unroll
  for (int pp = 0; pp < 2; ++pp)
#pragma unroll
    for (int m2 = 0; m2 < EMB; ++m2)
#pragma unroll
      for (int nb = 0; nb < ENB; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          Ml[((2 * wave + pp) * ECO + m2 * 16 + kq * 4 + r) * EP + nb * 16 + lr] = acc[pp][mb0 + m2][th * ENB + nb][r];
}

// one pass over Ml: output transform, operand chain and stores of 16 EMB channels (from cb0 within the group) x ETILE tiles, as 8-byte
// pairs or pixel by pixel
template <int NTHR, int TLX, int ETILE, int EMB, int EP>
__device__ __forceinline__ void wino2_store_pass(const ConvK p, const Wino2Out o, const float* Ml, int g, int cb0, int th, int oy0, int ox0, int d,
                                                 int ry, int tid) {
  constexpr int ECO = 16 * EMB;
  constexpr int EPT = ECO * ETILE / NTHR;  // (channel, tile) pairs per thread and pass
  typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
#pragma unroll
  for (int it = 0; it < EPT; ++it) {
    const int pair = tid + it * NTHR;
    const int e_co = pair / ETILE, e_t = pair - e_co * ETILE;
    const int e_tile = th * ETILE + e_t;
    const int e_tx = e_tile % TLX;
    const int sy = oy0 + 2 * (e_tile / TLX);
    const int sx = ox0 + (e_tx % d) + 2 * d * (e_tx / d);   // first output column of the tile
    float m[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) m[q] = Ml[(q * ECO + e_co) * EP + e_t];
    float t0[4], t1[4];
#pragma unroll
    for (int nu = 0; nu < 4; ++nu) {
      t0[nu] = m[nu] + m[4 + nu] + m[8 + nu];
      t1[nu] = m[4 + nu] - m[8 + nu] - m[12 + nu];
    }
    const float yv[2][2] = {{t0[0] + t0[1] + t0[2], t0[1] - t0[2] - t0[3]}, {t1[0] + t1[1] + t1[2], t1[1] - t1[2] - t1[3]}};
    // No load sits behind a divergent branch (a ragged channel tile, an edge tile): coordinates are clamped, only the STORE is
    // predicated.  With `continue` / edge tests in front of them the compiler waited for every load in flight at each join --
    // the six per-channel operands and the noise / residual pairs of a thread left one round trip after the other.
    const int cgi = cb0 + e_co;  // channel within the group
    const bool cok = cgi < p.cout_g;
    const int cg = g * p.cout_g + (cok ? cgi : p.cout_g - 1);
    const float os = o.osp[cg * p.oss], cs = p.csp[cg * p.css], cb = p.cbp[cg * p.cbs];
    const float b1 = p.b1p[cg * p.b1s], b2 = p.b2p[cg * p.b2s], sl2 = p.s2p[cg * p.s2s];
    const int cbase = cg * o.y_plane;
    auto fin = [&](float v, float nz, float r1v, float r2v) {
      v = v * os * cs + cb + b1;
      v = (v > 0.f ? v : v * p.s1) * p.g1;
      v += nz * o.nw + b2;
      v = (v > 0.f ? v : v * sl2) * p.g2;
      return v + r1v + r2v;
    };
    if (o.pairs) {   // (uniform) even output width: a tile's two pixels are a whole 8-byte pair or lie outside together
      f32x2u nz[2] = {{0.f, 0.f}, {0.f, 0.f}}, r1v[2] = {{0.f, 0.f}, {0.f, 0.f}}, r2v[2] = {{0.f, 0.f}, {0.f, 0.f}};
      int ro[2];
      bool inside[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int oy = (sy + i) * d + ry;
        inside[i] = cok && oy < p.OH && sx < p.OW;
        const int oyc = min(oy, p.OH - 1), oxc = min(sx, p.OW - 2);
        ro[i] = cbase + oyc * p.y_w + oxc;
        if (p.nzs) nz[i] = *reinterpret_cast<const f32x2u*>(o.nzp + oyc * p.OW + oxc);
        if (p.r1s) r1v[i] = *reinterpret_cast<const f32x2u*>(o.r1b + ro[i]);
        if (p.r2s) r2v[i] = *reinterpret_cast<const f32x2u*>(o.r2b + ro[i]);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x2u o2 = {fin(yv[i][0], nz[i][0], r1v[i][0], r2v[i][0]), fin(yv[i][1], nz[i][1], r1v[i][1], r2v[i][1])};
        if (inside[i]) *reinterpret_cast<f32x2u*>(o.yb + ro[i]) = o2;
      }
    } else {   // (the undilated row owner never gets here: its launches have W % 4 == 0)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int oy = (sy + i) * d + ry, ox = sx;
        if (!cok || oy >= p.OH || ox >= p.OW) continue;
        const int ro = cbase + oy * p.y_w + ox;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int oxj = ox + j * d;
          if (oxj >= p.OW) continue;
          const int rj = ro + j * d;
          o.yb[rj] = fin(yv[i][j], o.nzp[(oy * p.OW + oxj) * p.nzs], o.r1b[rj * p.r1s], o.r2b[rj * p.r2s]);
        }
      }
    }
  }
}

// The whole epilogue of a workgroup at (image b, group g, first channel co0 within the group, sub-image row oy0, image column ox0, dilation d,
// residue class ry); smem is reused for the exchange (the main loop ended on a barrier).  d = 1 as a constant folds the column arithmetic.
template <int NTHR, int MBW, int NBW, int TLX, int ETILE, int EMB, int EP>
__device__ __forceinline__ void wino2_epilogue(const ConvK p, float* smem, const f32x4 (&acc)[2][MBW][NBW], int b, int g, int co0, int oy0, int ox0,
                                               int d, int ry, int tid, int wave, int lr, int kq) {
  constexpr int NTILE = 16 * NBW;
  const Wino2Out o = wino2_out(p, b, d);
#pragma unroll
  for (int mb0 = 0; mb0 < MBW; mb0 += EMB) {
#pragma unroll
    for (int th = 0; th < NTILE / ETILE; ++th) {  // tile halves (only the 128-tile geometry has two)
      if (mb0 + th > 0) __syncthreads();           // (the chunk loop ended on a barrier)
      wino2_exchange<MBW, NBW, ETILE, EMB, EP>(smem, acc, mb0, th, wave, lr, kq);
      __syncthreads();
      wino2_store_pass<NTHR, TLX, ETILE, EMB, EP>(p, o, smem, g, co0 + mb0 * 16, th, oy0, ox0, d, ry, tid);
    }
  }
}

// ---- staging of the two row-owner kernels.  Patch rows travel as aligned 16-byte segments, one channel plane per wave and sub-stage;
//      p_voff = the lane's byte offsets in a plane (0x7ffffff0 = padding: past the resource, the load returns zeros).
typedef float f32x4v __attribute__((ext_vector_type(4)));

// this wave's plane of sub-stage j (clamped: past the end the last one is loaded again)
template <int NLD>
__device__ __forceinline__ void wino2_load_plane(__amdgpu_buffer_rsrc_t xrsrc, const int (&p_voff)[NLD], int j, int nstage, int wave, int Cin, int chw,
                                                 f32x4v (&dst)[NLD]) {
  const int jj = j < nstage ? j : nstage - 1;
  const int ci = jj * WINO2_RO_IVC + wave;
  const bool chin = ci < Cin;                                  // (a channel past the layer: every lane offset out of range -> zeros)
  const int soff = (chin ? ci : 0) * chw * 4;
#pragma unroll
  for (int i = 0; i < NLD; ++i) dst[i] = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, chin ? p_voff[i] : 0x7ffffff0, soff, 0));
}

// plane of sub-stage j -> Pdst [wave][ppitch]; the style scale and the (folded BatchNorm) affine ride on the patch.  wt_b / wc_b: this image's
// style / affine scales (per-image bases hoisted: the interval's scalar address arithmetic is part of its issue time)
template <int NLD>
__device__ __forceinline__ void wino2_commit_plane(const ConvK p, const float* wt_b, const float* wc_b, bool affine, float* Pdst, int ppitch, int j,
                                                   int wave, unsigned p_ok, const int (&p_dst)[NLD], const f32x4v (&src)[NLD]) {
  const int ci = j * WINO2_RO_IVC + wave;
  const bool chok = ci < p.Cin;
  const int cc = chok ? ci : p.Cin - 1;
  const float st = uload(wt_b, cc * p.wt_cs);
  float sc = st, sh = 0.f;
  if (affine) {   // (uniform for the launch) folded-BatchNorm input of the IR-SE body; the modulated layers skip two scalar loads and their address arithmetic
    sc = uload(wc_b, cc * p.wc_cs) * st;
    sh = uload(p.wshp, cc * p.wsh_cs) * st;
  }
  float* dst = Pdst + wave * ppitch;
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    // (These 16-byte writes start at word 1 + 4 l: NOT 16-byte aligned, served as four dword passes with the lanes four banks apart --
    //  14 conflict cycles per write, 27 % of the undilated kernel's LDS-active cycles (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.27; with
    //  the commits switched off 0.008).  Writing the ALIGNED unit (d of segment l - 1 through DPP wave_shr:1, a, b, c) takes the ratio to
    //  0.015 and the kernel from 605 to 630 us at 256 -> 256 / 128^2, 1211 to 1378 us at 32 -> 32 / 1024^2: the LDS is not what this
    //  kernel waits for, the extra VALU on the commit path is.  Kept misaligned.)
    // padding and absent channels arrive as ZEROS (out-of-range lane offset): only the affine shift still has to be masked, one select
    // per segment -- no zero FACTOR that would turn an Inf / NaN at a clamped address into a NaN border
    const float shm = (((p_ok >> i) & 1u) && chok) ? sh : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) dst[p_dst[i] + e] = fmaf(src[i][e], sc, shm);
  }
}

// U fragments: [group][co tile][chunk][wave][pp 2][lane][mb MBW] floats, one 4-channel chunk (k-step) c (clamped) and position pp per load.
// Buffer loads: resource = this channel tile's slice, scalar offset = chunk, lane offset u_voff fixed (a flat pointer costs a 64-bit VALU
// add per load and a handful of scalar instructions for the 64-bit chunk offset: 56 SALU + 60 VALU per 32 MFMAs were measured).
template <int MBW>
__device__ __forceinline__ void wino2_load_u_half(__amdgpu_buffer_rsrc_t ursrc, int u_voff, int c, int nchunk4, int pp, float (&u)[2 * MBW]) {
  constexpr int UF = 2 * MBW;
  const int cc = c < nchunk4 ? c : nchunk4 - 1;
  const int soff = cc * (8 * 64 * UF * 4);
  if constexpr (MBW == 4) {
    typedef float f32x4b __attribute__((ext_vector_type(4)));
    const f32x4b a = __builtin_bit_cast(f32x4b, __builtin_amdgcn_raw_buffer_load_b128(ursrc, u_voff + pp * 64 * MBW * 4, soff, 0));
    u[pp * 4 + 0] = a[0]; u[pp * 4 + 1] = a[1]; u[pp * 4 + 2] = a[2]; u[pp * 4 + 3] = a[3];
  } else if constexpr (MBW == 2) {
    typedef float f32x2b __attribute__((ext_vector_type(2)));
    const f32x2b a = __builtin_bit_cast(f32x2b, __builtin_amdgcn_raw_buffer_load_b64(ursrc, u_voff + pp * 64 * MBW * 4, soff, 0));
    u[pp * 2 + 0] = a[0]; u[pp * 2 + 1] = a[1];
  } else {
    u[pp] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ursrc, u_voff + pp * 64 * MBW * 4, soff, 0));
  }
}

// ---- host side
// the largest per-group block count of a launch (groups with a smaller dilation exit early)
inline int wino2_group_blocks(const ConvK& q, int TLX, int TLY) {
  int blocks = 0;
  for (int g = 0; g < q.G; ++g) {
    const int d = q.dil[g];
    const int SH = (q.H + d - 1) / d;
    const int n = ((q.W + 2 * TLX - 1) / (2 * TLX)) * ((SH + 2 * TLY - 1) / (2 * TLY)) * d;
    blocks = n > blocks ? n : blocks;
  }
  return blocks;
}

// region-major order (4) over bands of 8 x 2 TLY rows x 4 column tiles: the band / column-group counts the kernel decodes with, and the grid's x
inline void wino2_region_major(ConvK& q, int TLY, int TLX, int* blocks) {
  q.wg_order = 4;
  q.tiles_y = (q.H + 16 * TLY - 1) / (16 * TLY);
  q.tiles_x = ((q.W + 2 * TLX - 1) / (2 * TLX) + 3) / 4;
  *blocks = q.tiles_y * q.tiles_x * 32;
}

// what the row-owner staging needs of the input: rows and planes of whole, aligned 16-byte segments, and an image its buffer descriptor holds
inline bool wino2_rows_are_segments(const ConvK& q) {
  // padding = the raw-buffer range check of ONE image's descriptor (num_records = x_ch * H * W * 4 as an int; out-of-range lanes carry
  // offset 0x7ffffff0): an image of 2 GiB or more would wrap the record count and leave the padding unbacked -- refused here
  if ((int64_t)q.x_ch * q.H * q.W * 4 >= 0x7ffffff0ll) return false;
  return q.W % 4 == 0 && (reinterpret_cast<uintptr_t>(q.x) & 15) == 0 && ((int64_t)q.H * q.W) % 4 == 0;
}

}  // namespace vspconv

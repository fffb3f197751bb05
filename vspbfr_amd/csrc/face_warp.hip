// Faces inside whole photos for gfx950 (definitions: include/vspbfr_hip.h): the aligned crop of every face of a ragged
// batch of packed RGB photos, and the feathered paste-back of the restored crops into the output photos, in place.
//
// Both kernels are integer only.  The host turns each face's float64 2 x 3 matrix (destination -> source) into four int32 tables --
// ax / bx per destination column, cx / cy per destination row -- and a pixel's Q5 source coordinate is two adds and a shift; the
// bilinear weights are 5-bit fractions whose four products sum to 2^15.  tests/photo_ref.py restates it in NumPy and the bytes are equal.
//
//   crop    one workgroup per 32 x 32 tile of one face's S x S crop, a thread per 4 consecutive pixels of a row: 4 taps x 3 bytes per
//           pixel gathered from the photo (taps outside read the border colour), 12 bytes written as three dwords when S % 4 == 0 (any
//           S otherwise: byte stores), and / or the normalised fp32 NCHW values as the ingest kernel writes them.
//   paste   one workgroup per 32 x 32 tile of an output photo that at least one face's bounding box meets (the host's tile list; a
//           tile appears once, so a pixel is owned by one thread: no race, no atomics).  A thread reads its 4 pixels, walks the tile's
//           faces in list order -- distance to the crop border -> ramp weight -> value of the restored crop -> blend into the running
//           result -- and writes the pixels back if any face touched them.
//
// The source footprint of a tile is not staged in LDS: it is a variable-size parallelogram, and the 12 byte loads of a pixel hit lines
// its neighbours in the tile have just pulled into the CU's L1 (tools/bench_photo.py times both kernels).
//
// One kernel pair, two instantiations each, chosen by the item type.  vsp_face_item (the plain entries): four bilinear taps per pixel; the
// filter below is not compiled in.  vsp_face_aa_item (the *_aa entries): a face whose item carries reach > 0 is resampled by a
// tent filter one DESTINATION pixel wide, evaluated at the source lattice points of a (2 reach + 2)^2 window around the bilinear centre
// cell (forward tables source -> destination, also built by the host); a face with reach == 0 takes the four taps, bit for bit.
// tests/photo_aa_ref.py.
//
// Bounds: the entries check every item, table entry, tile and ramp value on the host against the buffer sizes they are given before
// anything is launched (one validator for the crop and one for the paste, shared by both item types; check_tables in face_tables.h is
// shared with color_fix.hip); the kernels index tables only inside [0, nx) / [0, ny) of an item and pixels only inside a tile's photo.
#include <algorithm>
#include <type_traits>

#include "face_tables.h"

namespace {

using vspface::check_tables;
using vspface::kTableLimit;
using vspface::kTwoGiB;

constexpr int kThreads = 256;
constexpr int kTile = VSP_FACE_TILE;         // 32 x 32 pixels: 8 threads x 4 pixels per row, 32 rows

// the item type of the anti-aliased entries: the one whose faces may be filtered
template <class Item>
constexpr bool kFiltered = std::is_same<Item, vsp_face_aa_item>::value;

__device__ __forceinline__ int reach_of(const vsp_face_item&) { return 0; }
__device__ __forceinline__ int reach_of(const vsp_face_aa_item& it) { return it.reach; }

// v = (sum of 32 (i ? fx : 32 - fx)(j ? fy : 32 - fy) p(ix + i, iy + j) + 16384) >> 15 for the three channels of a packed RGB image.
// CLAMP: tap indices are clamped to the last row / column (the caller guarantees ix, iy >= 0); otherwise a tap outside reads `border`.
template <bool CLAMP>
__device__ __forceinline__ void bilinear_rgb(const uint8_t* img, int w, int h, int X, int Y, const int border[3], int v[3]) {
  const int ix = X >> 5, fx = X & 31, iy = Y >> 5, fy = Y & 31;
  int acc[3] = {16384, 16384, 16384};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int wgt = 32 * (i ? fx : 32 - fx) * (j ? fy : 32 - fy);
      int xx = ix + i, yy = iy + j;
      bool in = true;
      if (CLAMP) {
        xx = min(xx, w - 1);
        yy = min(yy, h - 1);
      } else {
        in = (unsigned)xx < (unsigned)w && (unsigned)yy < (unsigned)h;
      }
      if (in) {
        const uint8_t* p = img + ((int64_t)yy * w + xx) * 3;
        acc[0] += wgt * (int)p[0];
        acc[1] += wgt * (int)p[1];
        acc[2] += wgt * (int)p[2];
      } else {
        acc[0] += wgt * border[0];
        acc[1] += wgt * border[1];
        acc[2] += wgt * border[2];
      }
    }
  }
  v[0] = acc[0] >> 15;
  v[1] = acc[1] >> 15;
  v[2] = acc[2] >> 15;
}

// anti-aliased.  // The tent filter of one destination pixel (dx, dy: absolute destination coordinates) over the window of source lattice points
// ix - R .. ix + R + 1, iy - R .. iy + R + 1 around its bilinear centre cell:
//     U = fu[qx] + gu[qy], V = fv[qx] + gv[qy], tu = max(0, 1024 - |U - 1024 dx|), tv likewise, w = (tu tv) >> 8,
//     v_c = (sum w p_c + (W >> 1)) / W, W = sum w.
// The differences are taken modulo 2^32: with |fu|, |gu| < 2^30 and 0 <= 1024 dx < 2^30 a true difference outside int32 wraps to a
// magnitude above 2^30, which is a zero weight like the true one.  fu / fv are monotone in qx (rne of a linear function), so their
// values at the two ends of the window bound a row's U and V: a row that cannot reach the pixel is culled with four compares.
// CLAMP: pixel indices are clamped to the image (table indices never are); otherwise a point outside reads `border`.
// The host entry has checked that the window of every served pixel lies inside the item's source range, so every table index is valid.
template <bool CLAMP>
__device__ __forceinline__ void filtered_rgb(const uint8_t* img, int w, int h, int X, int Y, int dx, int dy, const vsp_face_aa_item& it,
                                             const int32_t* fwd, const int border[3], int v[3]) {
  const int R = it.reach, nwin = 2 * R + 2;
  const int qx0 = (X >> 5) - R, qy0 = (Y >> 5) - R;
  const int32_t* fu = fwd + it.fwd_off + (qx0 - it.sx0);
  const int32_t* fv = fu + it.snx;
  const int32_t* gu = fwd + it.fwd_off + 2 * (int64_t)it.snx + (qy0 - it.sy0);
  const int32_t* gv = gu + it.sny;
  const unsigned tx = (unsigned)dx << 10, ty = (unsigned)dy << 10;
  const int ulo = min(fu[0], fu[nwin - 1]), uhi = max(fu[0], fu[nwin - 1]);
  const int vlo = min(fv[0], fv[nwin - 1]), vhi = max(fv[0], fv[nwin - 1]);
  int acc0 = 0, acc1 = 0, acc2 = 0, W = 0;
  for (int j = 0; j < nwin; ++j) {
    const unsigned gus = (unsigned)gu[j] - tx, gvs = (unsigned)gv[j] - ty;
    // the row's U - 1024 dx lies in [ulo + gus, uhi + gus]: no tap of it weighs anything unless that interval meets (-1024, 1024)
    if ((int)((unsigned)uhi + gus) <= -1024 || (int)((unsigned)ulo + gus) >= 1024) continue;
    if ((int)((unsigned)vhi + gvs) <= -1024 || (int)((unsigned)vlo + gvs) >= 1024) continue;
    int yy = qy0 + j;
    const bool row_in = (unsigned)yy < (unsigned)h;
    if (CLAMP) yy = min(max(yy, 0), h - 1);
    const uint8_t* rowp = img + (int64_t)yy * w * 3;
    for (int i = 0; i < nwin; ++i) {
      const unsigned du = (unsigned)fu[i] + gus, dv = (unsigned)fv[i] + gvs;
      const unsigned au = (int)du < 0 ? 0u - du : du, av = (int)dv < 0 ? 0u - dv : dv;
      if (au >= 1024u || av >= 1024u) continue;
      const int wgt = (int)(((1024u - au) * (1024u - av)) >> 8);
      if (wgt == 0) continue;
      int xx = qx0 + i;
      bool in = true;
      if (CLAMP)
        xx = min(max(xx, 0), w - 1);
      else
        in = row_in && (unsigned)xx < (unsigned)w;
      if (in) {
        const uint8_t* p = rowp + xx * 3;
        acc0 += wgt * (int)p[0];
        acc1 += wgt * (int)p[1];
        acc2 += wgt * (int)p[2];
      } else {
        acc0 += wgt * border[0];
        acc1 += wgt * border[1];
        acc2 += wgt * border[2];
      }
      W += wgt;
    }
  }
  // W > 0 for the tables of a similarity; the guard keeps a division by zero out of reach of any other table
  const unsigned Wd = (unsigned)max(W, 1), half = (unsigned)W >> 1;
  v[0] = (int)(((unsigned)acc0 + half) / Wd);
  v[1] = (int)(((unsigned)acc1 + half) / Wd);
  v[2] = (int)(((unsigned)acc2 + half) / Wd);
}

// the paste weight of a face's (S, S) uint16 mask at Q5 crop coordinates, with the four taps and the clamping of bilinear_rgb<true>:
// (sum of 32 wx wy m + 16384) >> 15 -- a mask of all 256 gives 256.  The result is clamped to 256: weights above it, which
// vsp_parse_blur_u16 never writes, act as 256 instead of wrapping the blended byte.
__device__ __forceinline__ int bilinear_mask(const uint16_t* m, int S, int X, int Y) {
  const int ix = X >> 5, fx = X & 31, iy = Y >> 5, fy = Y & 31;
  int acc = 16384;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      acc += 32 * (i ? fx : 32 - fx) * (j ? fy : 32 - fy) * (int)m[(int64_t)min(iy + j, S - 1) * S + min(ix + i, S - 1)];
  return min(acc >> 15, 256);
}

// a thread's 4 pixels x 3 channels.  A struct passed by reference: handed to store_crop as a bare array, the non-VEC crop compiled to other code
struct Quad {
  int v[4][3];
};

// the crop's store of a thread's 4 pixels of face f, row y, columns xg .. xg + 3: 12 bytes as three dwords / one float4 per channel (VEC), or
// element by element up to column S - 1
template <bool VEC>
__device__ __forceinline__ void store_crop(uint8_t* out_u8, float* out_f32, const Quad& q, int64_t f, int y, int xg, int S) {
  if (out_u8) {
    uint8_t* o = out_u8 + ((f * S + y) * S + xg) * 3;
    if (VEC) {
      uint32_t d[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int j = 4 * k + b;
          word |= (uint32_t)q.v[j / 3][j % 3] << (8 * b);
        }
        d[k] = word;
      }
      uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
      o4[0] = d[0];
      o4[1] = d[1];
      o4[2] = d[2];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (xg + e < S) {
          o[3 * e + 0] = (uint8_t)q.v[e][0];
          o[3 * e + 1] = (uint8_t)q.v[e][1];
          o[3 * e + 2] = (uint8_t)q.v[e][2];
        }
      }
    }
  }
  if (out_f32) {
    const int64_t plane = (int64_t)S * S;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = out_f32 + (f * 3 + c) * plane + (int64_t)y * S + xg;
      float n[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) n[e] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)q.v[e][c], 255.0f), 0.5f), 0.5f);
      if (VEC) {
        *reinterpret_cast<float4*>(o) = make_float4(n[0], n[1], n[2], n[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (xg + e < S) o[e] = n[e];
      }
    }
  }
}

// grid: (tiles per row, tiles per column, faces).  VEC: S % 4 == 0 and 16-byte aligned outputs -- dword / float4 stores.
// fwd: the forward tables of vsp_face_aa_item; unused (and last, so that no other argument moves) for vsp_face_item.
template <bool VEC, class Item>
__global__ __launch_bounds__(kThreads) void face_crop_kernel(uint8_t* out_u8, float* out_f32, const uint8_t* src, const int32_t* tables,
                                                              const Item* items, int S, int b0, int b1, int b2, const int32_t* fwd) {
  const Item it = items[blockIdx.z];
  const int y = (int)blockIdx.y * kTile + ((int)threadIdx.x >> 3);
  const int xg = (int)blockIdx.x * kTile + ((int)threadIdx.x & 7) * 4;
  if (y >= S || xg >= S) return;
  const int32_t* ax = tables + it.tab_off;
  const int32_t* bx = ax + S;
  const int cxv = ax[2 * S + y], cyv = ax[3 * S + y];
  const uint8_t* img = src + it.src_off;
  const int border[3] = {b0, b1, b2};
  Quad q;
  if (reach_of(it) == 0) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int x = min(xg + e, S - 1);   // (a pixel past the row repeats the last one and is not stored)
      bilinear_rgb<false>(img, it.w, it.h, (cxv + ax[x]) >> 5, (cyv + bx[x]) >> 5, border, q.v[e]);
    }
  } else if constexpr (kFiltered<Item>) {
    for (int e = 0; e < 4; ++e) {
      const int x = min(xg + e, S - 1);
      filtered_rgb<false>(img, it.w, it.h, (cxv + ax[x]) >> 5, (cyv + bx[x]) >> 5, x, y, it, fwd, border, q.v[e]);
    }
  }
  store_crop<VEC>(out_u8, out_f32, q, blockIdx.z, y, xg, S);
}

// grid: (tiles).  One thread owns 4 consecutive pixels of one tile row of the output photo.  fwd: as above.
// MASK (the *_mask entries): face i's ramp weight is scaled by its (S, S) uint16 paste weights at mask + i S S, sampled where
// the colour is; without it `mask` is not read and the instantiation is the code it was before the parameter existed.
template <class Item, bool MASK = false>
__global__ __launch_bounds__(kThreads) void face_paste_kernel(uint8_t* photos, const uint8_t* crops, const int32_t* tables, const Item* items,
                                                               const vsp_face_tile* tiles, const int32_t* tile_faces, const uint16_t* ramp,
                                                               int L, int S, const int32_t* fwd, const uint16_t* mask = nullptr) {
  const vsp_face_tile t = tiles[blockIdx.x];
  const int y = t.y0 + ((int)threadIdx.x >> 3);
  const int xg = t.x0 + ((int)threadIdx.x & 7) * 4;
  if (y >= t.h || xg >= t.w) return;
  uint8_t* row = photos + t.dst_off + ((int64_t)y * t.w + xg) * 3;
  const int npx = min(4, t.w - xg);
  int px[4][3];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < npx) {
      px[e][0] = row[3 * e + 0];
      px[e][1] = row[3 * e + 1];
      px[e][2] = row[3 * e + 2];
    } else {
      px[e][0] = px[e][1] = px[e][2] = 0;
    }
  }
  const int lim = (S - 1) * 32;
  const int none[3] = {0, 0, 0};
  bool touched = false;
  for (int k = 0; k < t.nfaces; ++k) {
    const int face = tile_faces[t.face0 + k];
    const Item it = items[face];
    const int ry = y - it.y0;
    if (ry < 0 || ry >= it.ny) continue;
    const int32_t* ax = tables + it.tab_off;
    const int32_t* bx = ax + it.nx;
    const int cxv = ax[2 * it.nx + ry], cyv = ax[2 * it.nx + it.ny + ry];
    const uint8_t* crop = crops + it.src_off;
#pragma unroll   // (the compiler unrolled the anti-aliased kernel's copy of this loop without being asked)
    for (int e = 0; e < 4; ++e) {
      const int rx = xg + e - it.x0;
      if (e >= npx || rx < 0 || rx >= it.nx) continue;
      const int X = (cxv + ax[rx]) >> 5, Y = (cyv + bx[rx]) >> 5;
      const int d = min(min(X, Y), min(lim - X, lim - Y));
      if (d < 0) continue;
      int w = ramp[min(d >> 2, L - 1)];
      if (w == 0) continue;   // (256 bg + 128) >> 8 = bg
      if constexpr (MASK) {
        w = (w * bilinear_mask(mask + (int64_t)face * S * S, S, X, Y) + 128) >> 8;
        if (w == 0) continue;
      }
      int f[3];
      if (reach_of(it) == 0)
        bilinear_rgb<true>(crop, S, S, X, Y, none, f);
      else if constexpr (kFiltered<Item>)
        filtered_rgb<true>(crop, S, S, X, Y, xg + e, y, it, fwd, none, f);
#pragma unroll
      for (int c = 0; c < 3; ++c) px[e][c] = (w * f[c] + (256 - w) * px[e][c] + 128) >> 8;
      touched = true;
    }
  }
  if (!touched) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e < npx) {
      row[3 * e + 0] = (uint8_t)px[e][0];
      row[3 * e + 1] = (uint8_t)px[e][1];
      row[3 * e + 2] = (uint8_t)px[e][2];
    }
  }
}

// The forward tables of the anti-aliased entries: host copy, device copy, entries.  The plain entries pass none, which every check on them
// below lets through.
struct Fwd {
  const int32_t* host = nullptr;
  const int32_t* dev = nullptr;
  size_t ints = 0;
};

// One anti-aliased item: its destination -> source tables as check_tables does, then reach (VSP_ENOTSUP above VSP_FACE_AA_MAX_REACH), the
// forward tables (inside the buffer, every entry below 2^30) and the source range: the centre cell of any pixel the item serves is
// ((cx[y] + ax[x]) >> 10, (cy[y] + bx[x]) >> 10), which lies between the cells of (min cx + min ax) and (max cx + max ax) -- the range
// must hold those extremes - reach .. + reach + 1.
int check_aa_item(const char* what, int i, const vsp_face_aa_item& a, const int32_t* tables, size_t table_ints, const int32_t* fwd,
                  size_t fwd_ints) {
  const int rc = check_tables(what, i, a, tables, table_ints);
  if (rc != VSP_OK) return rc;
  VSP_REQUIRE(a.reach >= 0, "%s: face %d: reach %d", what, i, a.reach);
  if (a.reach > VSP_FACE_AA_MAX_REACH)
    return vsp::fail(VSP_ENOTSUP, "%s: face %d: reach %d above %d (a minification above 16 is not served)", what, i, a.reach, VSP_FACE_AA_MAX_REACH);
  if (a.reach == 0 || a.nx == 0 || a.ny == 0) return VSP_OK;
  VSP_REQUIRE(fwd, "%s: null pointer (forward tables of face %d)", what, i);
  VSP_REQUIRE(a.snx > 0 && a.sny > 0 && a.snx <= VSP_FACE_AA_MAX_RANGE && a.sny <= VSP_FACE_AA_MAX_RANGE, "%s: face %d: source range of %d x %d", what,
              i, a.snx, a.sny);
  VSP_REQUIRE(a.sx0 > -kTableLimit && a.sx0 < kTableLimit && a.sy0 > -kTableLimit && a.sy0 < kTableLimit, "%s: face %d: source range at (%d, %d)",
              what, i, a.sx0, a.sy0);
  VSP_REQUIRE(a.x0 >= 0 && a.y0 >= 0 && (int64_t)a.x0 + a.nx <= (1 << 20) && (int64_t)a.y0 + a.ny <= (1 << 20),
              "%s: face %d: a filtered face's destination must stay below 2^20 pixels a side", what, i);
  const uint64_t n = 2ull * (uint64_t)a.snx + 2ull * (uint64_t)a.sny;
  VSP_REQUIRE(a.fwd_off >= 0 && (uint64_t)a.fwd_off + n <= (uint64_t)fwd_ints, "%s: face %d: forward tables outside the %zu entries", what, i,
              fwd_ints);
  const int32_t* f = fwd + a.fwd_off;
  for (uint64_t k = 0; k < n; ++k)
    VSP_REQUIRE(f[k] > -kTableLimit && f[k] < kTableLimit, "%s: face %d: table overflow (forward entry %llu = %d, magnitude 2^30 or more)", what, i,
                (unsigned long long)k, f[k]);
  const int32_t* t = tables + a.tab_off;
  int64_t lo[4], hi[4];   // ax, bx, cx, cy
  const int len[4] = {a.nx, a.nx, a.ny, a.ny};
  for (int q = 0; q < 4; ++q) {
    lo[q] = hi[q] = t[0];
    for (int k = 0; k < len[q]; ++k) {
      lo[q] = std::min<int64_t>(lo[q], t[k]);
      hi[q] = std::max<int64_t>(hi[q], t[k]);
    }
    t += len[q];
  }
  const int64_t ix0 = (lo[2] + lo[0]) >> 10, ix1 = (hi[2] + hi[0]) >> 10, iy0 = (lo[3] + lo[1]) >> 10, iy1 = (hi[3] + hi[1]) >> 10;
  VSP_REQUIRE(ix0 - a.reach >= a.sx0 && ix1 + a.reach + 1 < (int64_t)a.sx0 + a.snx && iy0 - a.reach >= a.sy0 &&
                  iy1 + a.reach + 1 < (int64_t)a.sy0 + a.sny,
              "%s: face %d: source range too small (columns %d + %d, rows %d + %d; windows reach columns %lld .. %lld, rows %lld .. %lld)", what, i,
              a.sx0, a.snx, a.sy0, a.sny, (long long)(ix0 - a.reach), (long long)(ix1 + a.reach + 1), (long long)(iy0 - a.reach),
              (long long)(iy1 + a.reach + 1));
  return VSP_OK;
}

// the tables of one item of either type
int check_item_tables(const char* what, int i, const vsp_face_item& it, const int32_t* tables, size_t table_ints, const Fwd&) {
  return check_tables(what, i, it, tables, table_ints);
}
int check_item_tables(const char* what, int i, const vsp_face_aa_item& it, const int32_t* tables, size_t table_ints, const Fwd& fwd) {
  return check_aa_item(what, i, it, tables, table_ints, fwd.host, fwd.ints);
}

bool misaligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// Every argument of a crop entry; `what` is the entry's name in the messages.  VSP_OK with n == 0: nothing to launch.
template <class Item>
int check_crop(const char* what, const uint8_t* out_u8, const float* out_f32, const uint8_t* src, size_t src_bytes, const int32_t* tables,
               const int32_t* tables_dev, size_t table_ints, const Fwd& fwd, const Item* items, const Item* items_dev, int n, int S, int border_r,
               int border_g, int border_b) {
  VSP_REQUIRE(n >= 0 && n <= VSP_FACE_MAX_ITEMS, "%s: 0..%d faces (got %d)", what, VSP_FACE_MAX_ITEMS, n);
  VSP_REQUIRE(S > 0 && S <= VSP_FACE_MAX_SIDE, "%s: crop side 1..%d (got %d)", what, VSP_FACE_MAX_SIDE, S);
  VSP_REQUIRE((unsigned)border_r < 256u && (unsigned)border_g < 256u && (unsigned)border_b < 256u, "%s: border colour outside 0..255", what);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(out_u8 || out_f32, "%s: null pointer (no output)", what);
  VSP_REQUIRE(src && tables && tables_dev && items && items_dev && (fwd.host == nullptr) == (fwd.dev == nullptr), "%s: null pointer", what);
  VSP_REQUIRE(!misaligned(tables_dev, 3u) && !misaligned(fwd.dev, 3u) && !misaligned(items_dev, 7u) && !misaligned(out_f32, 3u),
              "%s: misaligned tables, items or fp32 output", what);
  VSP_REQUIRE((uint64_t)src_bytes < kTwoGiB && (uint64_t)n * S * S * 3ull < kTwoGiB && (uint64_t)fwd.ints * 4ull < kTwoGiB,
              kFiltered<Item> ? "%s: the photos and the tables must stay below 2 GiB and an output below 2^31 elements (%d faces of %d x %d)"
                              : "%s: the photos must stay below 2 GiB and an output below 2^31 elements (%d faces of %d x %d)",
              what, n, S, S);
  for (int i = 0; i < n; ++i) {
    const Item& it = items[i];
    VSP_REQUIRE(it.w > 0 && it.h > 0, "%s: face %d: photo size %d x %d", what, i, it.w, it.h);
    VSP_REQUIRE(it.src_off >= 0 && (uint64_t)it.src_off + 3ull * (uint64_t)it.w * (uint64_t)it.h <= (uint64_t)src_bytes,
                "%s: face %d: photo outside the %zu source bytes", what, i, src_bytes);
    if constexpr (kFiltered<Item>)   // its destination is the crop itself: the filter takes absolute destination coordinates
      VSP_REQUIRE(it.nx == S && it.ny == S && it.x0 == 0 && it.y0 == 0, "%s: face %d: tables of %d x %d at (%d, %d) for a crop of side %d", what, i,
                  it.nx, it.ny, it.x0, it.y0, S);
    else
      VSP_REQUIRE(it.nx == S && it.ny == S, "%s: face %d: tables of %d x %d for a crop of side %d", what, i, it.nx, it.ny, S);
    const int rc = check_item_tables(what, i, it, tables, table_ints, fwd);
    if (rc != VSP_OK) return rc;
  }
  return VSP_OK;
}

// Every argument of a paste entry.  VSP_OK with n == 0 or ntiles == 0: nothing to launch.
template <class Item>
int check_paste(const char* what, const uint8_t* photos, size_t photo_bytes, const uint8_t* crops, size_t crop_bytes, const int32_t* tables,
                const int32_t* tables_dev, size_t table_ints, const Fwd& fwd, const Item* items, const Item* items_dev, int n, int S,
                const vsp_face_tile* tiles, const vsp_face_tile* tiles_dev, int ntiles, const int32_t* tile_faces, const int32_t* tile_faces_dev,
                size_t tile_face_ints, const uint16_t* ramp, const uint16_t* ramp_dev, int ramp_len) {
  VSP_REQUIRE(n >= 0 && n <= VSP_FACE_MAX_ITEMS, "%s: 0..%d faces (got %d)", what, VSP_FACE_MAX_ITEMS, n);
  VSP_REQUIRE(S > 0 && S <= VSP_FACE_MAX_SIDE, "%s: crop side 1..%d (got %d)", what, VSP_FACE_MAX_SIDE, S);
  VSP_REQUIRE(ntiles >= 0, "%s: %d tiles", what, ntiles);
  VSP_REQUIRE(ramp && ramp_dev, "%s: null pointer (ramp)", what);
  VSP_REQUIRE(ramp_len >= 1 && ramp_len <= VSP_FACE_MAX_RAMP, "%s: ramp of 1..%d entries (got %d)", what, VSP_FACE_MAX_RAMP, ramp_len);
  VSP_REQUIRE(ramp[0] == 0, "%s: ramp[0] != 0 (the crop border itself must keep the background; got %d)", what, (int)ramp[0]);
  for (int k = 0; k < ramp_len; ++k) VSP_REQUIRE(ramp[k] <= 256, "%s: ramp[%d] = %d above 256", what, k, (int)ramp[k]);
  if (n == 0 || ntiles == 0) return VSP_OK;
  VSP_REQUIRE(photos && crops && tables && tables_dev && items && items_dev && tiles && tiles_dev && tile_faces && tile_faces_dev &&
                  (fwd.host == nullptr) == (fwd.dev == nullptr),
              "%s: null pointer", what);
  VSP_REQUIRE(!misaligned(tables_dev, 3u) && !misaligned(fwd.dev, 3u) && !misaligned(items_dev, 7u) && !misaligned(tiles_dev, 7u) &&
                  !misaligned(tile_faces_dev, 3u) && !misaligned(ramp_dev, 1u),
              "%s: misaligned tables, items, tiles or ramp", what);
  VSP_REQUIRE((uint64_t)photo_bytes < kTwoGiB && (uint64_t)crop_bytes < kTwoGiB && (uint64_t)fwd.ints * 4ull < kTwoGiB,
              kFiltered<Item> ? "%s: the photos, the crops and the tables must each stay below 2 GiB"
                              : "%s: the photos and the crops must each stay below 2 GiB",
              what);
  const uint64_t one = 3ull * (uint64_t)S * (uint64_t)S;
  for (int i = 0; i < n; ++i) {
    const Item& it = items[i];
    VSP_REQUIRE(it.w == S && it.h == S, "%s: face %d: its source is the %d x %d crop (got %d x %d)", what, i, S, S, it.w, it.h);
    VSP_REQUIRE(it.src_off >= 0 && (uint64_t)it.src_off + one <= (uint64_t)crop_bytes, "%s: face %d: crop outside the %zu crop bytes", what, i,
                crop_bytes);
    VSP_REQUIRE(it.x0 >= 0 && it.y0 >= 0, "%s: face %d: bounding box at (%d, %d)", what, i, it.x0, it.y0);
    const int rc = check_item_tables(what, i, it, tables, table_ints, fwd);
    if (rc != VSP_OK) return rc;
  }
  for (int k = 0; k < ntiles; ++k) {
    const vsp_face_tile& t = tiles[k];
    VSP_REQUIRE(t.w > 0 && t.h > 0 && t.dst_off >= 0 && (uint64_t)t.dst_off + 3ull * (uint64_t)t.w * (uint64_t)t.h <= (uint64_t)photo_bytes,
                "%s: tile %d: photo outside the %zu photo bytes", what, k, photo_bytes);
    VSP_REQUIRE(t.x0 >= 0 && t.y0 >= 0 && t.x0 % kTile == 0 && t.y0 % kTile == 0 && t.x0 < t.w && t.y0 < t.h,
                "%s: tile %d at (%d, %d) of a %d x %d photo", what, k, t.x0, t.y0, t.w, t.h);
    if (k > 0) {   // strictly ascending (photo, row, column): a tile appears once, so one thread owns a pixel
      const vsp_face_tile& p = tiles[k - 1];
      const bool same = p.dst_off == t.dst_off;
      VSP_REQUIRE(same ? (p.w == t.w && p.h == t.h && (p.y0 < t.y0 || (p.y0 == t.y0 && p.x0 < t.x0)))
                       : (uint64_t)p.dst_off + 3ull * (uint64_t)p.w * (uint64_t)p.h <= (uint64_t)t.dst_off,
                  "%s: tile %d: tiles must ascend by photo, row, column without repeats or overlapping photos", what, k);
    }
    VSP_REQUIRE(t.nfaces >= 1 && t.face0 >= 0 && (uint64_t)t.face0 + (uint64_t)t.nfaces <= (uint64_t)tile_face_ints,
                "%s: tile %d: face list outside the %zu entries", what, k, tile_face_ints);
    for (int j = 0; j < t.nfaces; ++j) {
      const int f = tile_faces[t.face0 + j];
      VSP_REQUIRE(f >= 0 && f < n && (j == 0 || tile_faces[t.face0 + j - 1] < f), "%s: tile %d: faces must be 0..%d in list order", what, k, n - 1);
      const Item& it = items[f];
      VSP_REQUIRE((int64_t)it.x0 + it.nx <= t.w && (int64_t)it.y0 + it.ny <= t.h, "%s: tile %d: face %d's bounding box leaves the photo", what, k, f);
    }
  }
  return VSP_OK;
}

// the one more buffer of the masked paste entries: n faces of S x S uint16 weights on the device
int check_mask(const char* what, const uint16_t* mask_dev, size_t mask_elems, int n, int S) {
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(mask_dev, "%s: null pointer (mask)", what);
  VSP_REQUIRE(!misaligned(mask_dev, 1u), "%s: misaligned mask", what);
  VSP_REQUIRE((uint64_t)mask_elems >= (uint64_t)n * (uint64_t)S * (uint64_t)S, "%s: mask of %zu weights, %d faces of %d x %d need more", what,
              mask_elems, n, S, S);
  if ((uint64_t)mask_elems * 2ull >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "%s: a mask of 2 GiB or more", what);
  return VSP_OK;
}

// the crop's launch: grid and the choice of the store path
template <class Item>
void launch_crop(uint8_t* out_u8, float* out_f32, const uint8_t* src, const int32_t* tables_dev, const Item* items_dev, int n, int S, int border_r,
                 int border_g, int border_b, const int32_t* fwd_dev, vsp_stream_t stream) {
  const unsigned tiles = (unsigned)((S + kTile - 1) / kTile);
  const bool vec = S % 4 == 0 && !misaligned(out_u8, 3u) && !misaligned(out_f32, 15u);
  const auto kernel = vec ? face_crop_kernel<true, Item> : face_crop_kernel<false, Item>;
  kernel<<<dim3(tiles, tiles, (unsigned)n), kThreads, 0, vsp::as_stream(stream)>>>(out_u8, out_f32, src, tables_dev, items_dev, S, border_r, border_g,
                                                                                   border_b, fwd_dev);
}

}  // namespace

extern "C" {

int vsp_face_crop_u8(uint8_t* out_u8, float* out_f32, const uint8_t* src, size_t src_bytes, const int32_t* tables, const int32_t* tables_dev,
                     size_t table_ints, const vsp_face_item* items, const vsp_face_item* items_dev, int n, int S, int border_r, int border_g,
                     int border_b, vsp_stream_t stream) {
  const int rc = check_crop("face_crop", out_u8, out_f32, src, src_bytes, tables, tables_dev, table_ints, Fwd{}, items, items_dev, n, S, border_r,
                            border_g, border_b);
  if (rc != VSP_OK || n == 0) return rc;
  launch_crop(out_u8, out_f32, src, tables_dev, items_dev, n, S, border_r, border_g, border_b, nullptr, stream);
  return vsp::check_launch("face_crop");
}

int vsp_face_paste_u8(uint8_t* photos, size_t photo_bytes, const uint8_t* crops, size_t crop_bytes, const int32_t* tables,
                      const int32_t* tables_dev, size_t table_ints, const vsp_face_item* items, const vsp_face_item* items_dev, int n, int S,
                      const vsp_face_tile* tiles, const vsp_face_tile* tiles_dev, int ntiles, const int32_t* tile_faces,
                      const int32_t* tile_faces_dev, size_t tile_face_ints, const uint16_t* ramp, const uint16_t* ramp_dev, int ramp_len,
                      vsp_stream_t stream) {
  const int rc = check_paste("face_paste", photos, photo_bytes, crops, crop_bytes, tables, tables_dev, table_ints, Fwd{}, items, items_dev, n, S, tiles,
                             tiles_dev, ntiles, tile_faces, tile_faces_dev, tile_face_ints, ramp, ramp_dev, ramp_len);
  if (rc != VSP_OK || n == 0 || ntiles == 0) return rc;
  face_paste_kernel<<<dim3((unsigned)ntiles), kThreads, 0, vsp::as_stream(stream)>>>(photos, crops, tables_dev, items_dev, tiles_dev, tile_faces_dev,
                                                                                     ramp_dev, ramp_len, S, nullptr);
  return vsp::check_launch("face_paste");
}

int vsp_face_crop_aa_u8(uint8_t* out_u8, float* out_f32, const uint8_t* src, size_t src_bytes, const int32_t* tables, const int32_t* tables_dev,
                        size_t table_ints, const int32_t* fwd, const int32_t* fwd_dev, size_t fwd_ints, const vsp_face_aa_item* items,
                        const vsp_face_aa_item* items_dev, int n, int S, int border_r, int border_g, int border_b, vsp_stream_t stream) {
  const int rc = check_crop("face_crop_aa", out_u8, out_f32, src, src_bytes, tables, tables_dev, table_ints, Fwd{fwd, fwd_dev, fwd_ints}, items,
                            items_dev, n, S, border_r, border_g, border_b);
  if (rc != VSP_OK || n == 0) return rc;
  launch_crop(out_u8, out_f32, src, tables_dev, items_dev, n, S, border_r, border_g, border_b, fwd_dev, stream);
  return vsp::check_launch("face_crop_aa");
}

int vsp_face_paste_aa_u8(uint8_t* photos, size_t photo_bytes, const uint8_t* crops, size_t crop_bytes, const int32_t* tables,
                         const int32_t* tables_dev, size_t table_ints, const int32_t* fwd, const int32_t* fwd_dev, size_t fwd_ints,
                         const vsp_face_aa_item* items, const vsp_face_aa_item* items_dev, int n, int S, const vsp_face_tile* tiles,
                         const vsp_face_tile* tiles_dev, int ntiles, const int32_t* tile_faces, const int32_t* tile_faces_dev,
                         size_t tile_face_ints, const uint16_t* ramp, const uint16_t* ramp_dev, int ramp_len, vsp_stream_t stream) {
  const int rc = check_paste("face_paste_aa", photos, photo_bytes, crops, crop_bytes, tables, tables_dev, table_ints, Fwd{fwd, fwd_dev, fwd_ints}, items,
                             items_dev, n, S, tiles, tiles_dev, ntiles, tile_faces, tile_faces_dev, tile_face_ints, ramp, ramp_dev, ramp_len);
  if (rc != VSP_OK || n == 0 || ntiles == 0) return rc;
  face_paste_kernel<<<dim3((unsigned)ntiles), kThreads, 0, vsp::as_stream(stream)>>>(photos, crops, tables_dev, items_dev, tiles_dev, tile_faces_dev,
                                                                                     ramp_dev, ramp_len, S, fwd_dev);
  return vsp::check_launch("face_paste_aa");
}

// the two paste entries with a face-parsing mask: the arguments of the entries above, checked by the same validator, and
// the (n, S, S) uint16 weights
int vsp_face_paste_mask_u8(uint8_t* photos, size_t photo_bytes, const uint8_t* crops, size_t crop_bytes, const int32_t* tables,
                           const int32_t* tables_dev, size_t table_ints, const vsp_face_item* items, const vsp_face_item* items_dev, int n, int S,
                           const vsp_face_tile* tiles, const vsp_face_tile* tiles_dev, int ntiles, const int32_t* tile_faces,
                           const int32_t* tile_faces_dev, size_t tile_face_ints, const uint16_t* ramp, const uint16_t* ramp_dev, int ramp_len,
                           const uint16_t* mask_dev, size_t mask_elems, vsp_stream_t stream) {
  int rc = check_paste("face_paste_mask", photos, photo_bytes, crops, crop_bytes, tables, tables_dev, table_ints, Fwd{}, items, items_dev, n, S,
                       tiles, tiles_dev, ntiles, tile_faces, tile_faces_dev, tile_face_ints, ramp, ramp_dev, ramp_len);
  if (rc == VSP_OK) rc = check_mask("face_paste_mask", mask_dev, mask_elems, n, S);
  if (rc != VSP_OK || n == 0 || ntiles == 0) return rc;
  face_paste_kernel<vsp_face_item, true><<<dim3((unsigned)ntiles), kThreads, 0, vsp::as_stream(stream)>>>(
      photos, crops, tables_dev, items_dev, tiles_dev, tile_faces_dev, ramp_dev, ramp_len, S, nullptr, mask_dev);
  return vsp::check_launch("face_paste_mask");
}

int vsp_face_paste_mask_aa_u8(uint8_t* photos, size_t photo_bytes, const uint8_t* crops, size_t crop_bytes, const int32_t* tables,
                              const int32_t* tables_dev, size_t table_ints, const int32_t* fwd, const int32_t* fwd_dev, size_t fwd_ints,
                              const vsp_face_aa_item* items, const vsp_face_aa_item* items_dev, int n, int S, const vsp_face_tile* tiles,
                              const vsp_face_tile* tiles_dev, int ntiles, const int32_t* tile_faces, const int32_t* tile_faces_dev,
                              size_t tile_face_ints, const uint16_t* ramp, const uint16_t* ramp_dev, int ramp_len, const uint16_t* mask_dev,
                              size_t mask_elems, vsp_stream_t stream) {
  int rc = check_paste("face_paste_mask_aa", photos, photo_bytes, crops, crop_bytes, tables, tables_dev, table_ints, Fwd{fwd, fwd_dev, fwd_ints},
                       items, items_dev, n, S, tiles, tiles_dev, ntiles, tile_faces, tile_faces_dev, tile_face_ints, ramp, ramp_dev, ramp_len);
  if (rc == VSP_OK) rc = check_mask("face_paste_mask_aa", mask_dev, mask_elems, n, S);
  if (rc != VSP_OK || n == 0 || ntiles == 0) return rc;
  face_paste_kernel<vsp_face_aa_item, true><<<dim3((unsigned)ntiles), kThreads, 0, vsp::as_stream(stream)>>>(
      photos, crops, tables_dev, items_dev, tiles_dev, tile_faces_dev, ramp_dev, ramp_len, S, fwd_dev, mask_dev);
  return vsp::check_launch("face_paste_mask_aa");
}

}  // extern "C"

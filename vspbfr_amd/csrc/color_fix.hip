// Colour fix for restored faces, gfx950 (definitions: include/vspbfr_hip.h): between the crop and the paste-back of the
// whole-photo path the restored crop takes its low frequencies (wavelet) or its per-channel mean and deviation (stats) from the source
// crop.  Integer only; tests/color_fix_ref.py restates both modes in NumPy and the bytes are equal.
//
//   wavelet  one launch per level.  A level is the separable 3-tap [1 2 1] / 4 with stride s = 2^l on the Q6 difference plane, indices
//            clamped to the image.  One workgroup per 64 x 32 tile of one face: per channel it stages the tile plus a halo of s in LDS
//            (cells hold the plane at the CLAMPED image coordinate, so a halo cell equals the whole-plane value), runs the pass along x
//            over every staged row into a second LDS buffer and the pass along y from there.  The first level forms the difference from
//            the two uint8 crops and the validity test while it stages (all three channels at once: s = 1); the levels between read and
//            write planar int16 (F, 3, S, S) scratch, ping-pong; the last level keeps its three channels in registers, adds them to the
//            restored crop and writes packed uint8.  levels == 1: the first level writes the plane and a pointwise kernel applies it,
//            so that no workgroup writes `out` while another still reads a halo of `restored` (out may alias restored).
//   stats    one reduction launch (per-thread uint32 partial sums over 16 pixels, wave shuffles, LDS across the four waves, one 64-bit
//            integer atomic per sum and workgroup: integer sums, so the order does not matter) and one apply launch whose first three
//            threads finish the face's twelve constants from the sums.  No copy to the host in between.
//
// Bounds: the entry checks sizes, scratch, items and tables on the host before anything is launched; the kernels index pixels only
// inside [0, S)^2 of face blockIdx.z / blockIdx.y < F and tables only inside [0, S) of an item's four tables.
#include "face_tables.h"

namespace {

using vspface::kTwoGiB;

constexpr int kThreads = 256;
constexpr int kTW = 64, kTH = 32;          // tile: 16 threads x 4 pixels a row, 16 thread rows x 2 rows
constexpr int kChunk = kThreads * 16;      // stats: pixels of one workgroup, 4 groups of 4 per thread

struct alignas(8) short4_t {
  int16_t v[4];
};

// the centre cell of crop pixel (x, y) lies inside the photo (tab == nullptr: always)
__device__ __forceinline__ bool valid_px(const int32_t* tab, int S, int w, int h, int x, int y) {
  if (!tab) return true;
  const int ix = (tab[2 * S + y] + tab[x]) >> 10, iy = (tab[3 * S + y] + tab[S + x]) >> 10;
  return (unsigned)ix < (unsigned)w && (unsigned)iy < (unsigned)h;
}

__device__ __forceinline__ void unpack12(const uint32_t w[3], int px[4][3]) {
#pragma unroll
  for (int j = 0; j < 12; ++j) px[j / 3][j % 3] = (int)((w[j / 4] >> (8 * (j % 4))) & 255u);
}

__device__ __forceinline__ void pack12(const int px[4][3], uint32_t w[3]) {
  w[0] = w[1] = w[2] = 0;
#pragma unroll
  for (int j = 0; j < 12; ++j) w[j / 4] |= (uint32_t)px[j / 3][j % 3] << (8 * (j % 4));
}

// One wavelet level.  grid (ceil(S / 64), ceil(S / 32), F).  Dynamic LDS: A[FIRST ? 3 : 1][rows][WA] int16, B[rows][64] int16 with
// rows = 32 + 2 s, WA = 64 + 2 sp, sp = s rounded up to 4 (so that a staged group of 4 columns starts at a multiple of 4).
// FIRST: src is unused, the difference comes from crop / restored / tab; else src16 is the planar plane of the level before.
// LAST: out = clamp(restored + ((d + 32) >> 6)); else dst16 gets the plane.  VEC: S % 4 == 0 and 4-byte aligned uint8 buffers.
template <bool FIRST, bool LAST, bool VEC>
__global__ __launch_bounds__(kThreads) void wavelet_level_kernel(const uint8_t* crop, const uint8_t* restored, uint8_t* out, const int16_t* src16,
                                                                  int16_t* dst16, const int32_t* tables, const vsp_face_item* items, int S, int s) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int sp = (s + 3) & ~3, rows = kTH + 2 * s, WA = kTW + 2 * sp, GA = WA / 4;
  int16_t* A = reinterpret_cast<int16_t*>(smem);
  int16_t* B = A + (FIRST ? 3 : 1) * rows * WA;
  const int t = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * kTW, y0 = (int)blockIdx.y * kTH;
  const int64_t f = blockIdx.z, plane = (int64_t)S * S;

  if (FIRST) {
    const int32_t* tab = nullptr;
    int pw = 0, ph = 0;
    if (items) {
      const vsp_face_item it = items[f];
      tab = tables + it.tab_off;
      pw = it.w, ph = it.h;
    }
    for (int idx = t; idx < rows * GA; idx += kThreads) {
      const int ly = idx / GA, lg = idx - ly * GA;
      const int cy = min(max(y0 - s + ly, 0), S - 1), gx = x0 - sp + 4 * lg;
      int c[4][3], r[4][3], xx[4];
      if (VEC && gx >= 0 && gx + 3 < S) {
        const int64_t o = ((f * S + cy) * S + gx) * 3;
        const uint32_t* c4 = reinterpret_cast<const uint32_t*>(crop + o);
        const uint32_t* r4 = reinterpret_cast<const uint32_t*>(restored + o);
        const uint32_t cw[3] = {c4[0], c4[1], c4[2]}, rw[3] = {r4[0], r4[1], r4[2]};
        unpack12(cw, c);
        unpack12(rw, r);
#pragma unroll
        for (int e = 0; e < 4; ++e) xx[e] = gx + e;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          xx[e] = min(max(gx + e, 0), S - 1);
          const int64_t o = ((f * S + cy) * S + xx[e]) * 3;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) c[e][ch] = crop[o + ch], r[e][ch] = restored[o + ch];
        }
      }
      short4_t d[3];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool ok = valid_px(tab, S, pw, ph, xx[e], cy);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) d[ch].v[e] = (int16_t)(ok ? (c[e][ch] - r[e][ch]) * 64 : 0);
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) *reinterpret_cast<short4_t*>(A + (ch * rows + ly) * WA + 4 * lg) = d[ch];
    }
    __syncthreads();
  }

  const int g = t & 15, ry = t >> 4;   // the thread's 4 columns x0 + 4 g .. + 3 and rows y0 + ry, y0 + ry + 16
  int res[3][2][4];
  for (int ch = 0; ch < 3; ++ch) {
    const int16_t* Ac = A + (FIRST ? ch * rows * WA : 0);
    if (!FIRST) {
      const int16_t* sp16 = src16 + (f * 3 + ch) * plane;
      for (int idx = t; idx < rows * GA; idx += kThreads) {
        const int ly = idx / GA, lg = idx - ly * GA;
        const int cy = min(max(y0 - s + ly, 0), S - 1), gx = x0 - sp + 4 * lg;
        const int16_t* row = sp16 + (int64_t)cy * S;
        short4_t d;
        if (VEC && gx >= 0 && gx + 3 < S) {
          d = *reinterpret_cast<const short4_t*>(row + gx);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) d.v[e] = row[min(max(gx + e, 0), S - 1)];
        }
        *reinterpret_cast<short4_t*>(A + ly * WA + 4 * lg) = d;
      }
      __syncthreads();
    }
    // along x: every staged row, the tile's 64 columns
    for (int idx = t; idx < rows * (kTW / 4); idx += kThreads) {
      const int ly = idx >> 4, lg = idx & 15;
      const int16_t* p = Ac + ly * WA + (sp - s) + 4 * lg;   // p[e], p[e + s], p[e + 2 s]: columns x - s, x, x + s
      short4_t o;
      if ((s & 3) == 0) {
        const short4_t a = *reinterpret_cast<const short4_t*>(p), b = *reinterpret_cast<const short4_t*>(p + s),
                       c = *reinterpret_cast<const short4_t*>(p + 2 * s);
#pragma unroll
        for (int e = 0; e < 4; ++e) o.v[e] = (int16_t)(((int)a.v[e] + 2 * (int)b.v[e] + (int)c.v[e] + 2) >> 2);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o.v[e] = (int16_t)(((int)p[e] + 2 * (int)p[e + s] + (int)p[e + 2 * s] + 2) >> 2);
      }
      *reinterpret_cast<short4_t*>(B + ly * kTW + 4 * lg) = o;
    }
    __syncthreads();
    // along y: B row ly holds image row clamp(y0 - s + ly)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int16_t* p = B + (ry + 16 * k) * kTW + 4 * g;
      const short4_t a = *reinterpret_cast<const short4_t*>(p), b = *reinterpret_cast<const short4_t*>(p + s * kTW),
                     c = *reinterpret_cast<const short4_t*>(p + 2 * s * kTW);
#pragma unroll
      for (int e = 0; e < 4; ++e) res[ch][k][e] = ((int)a.v[e] + 2 * (int)b.v[e] + (int)c.v[e] + 2) >> 2;
    }
    if (!LAST) {
      int16_t* dp = dst16 + (f * 3 + ch) * plane;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int y = y0 + ry + 16 * k, x = x0 + 4 * g;
        if (y >= S || x >= S) continue;
        int16_t* o = dp + (int64_t)y * S + x;
        if (VEC) {
          short4_t v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v.v[e] = (int16_t)res[ch][k][e];
          *reinterpret_cast<short4_t*>(o) = v;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (x + e < S) o[e] = (int16_t)res[ch][k][e];
        }
      }
    }
    __syncthreads();   // A and B are free for the next channel
  }

  if (LAST) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int y = y0 + ry + 16 * k, x = x0 + 4 * g;
      if (y >= S || x >= S) continue;
      const int64_t o = ((f * S + y) * S + x) * 3;
      int px[4][3];
      if (VEC) {
        const uint32_t* r4 = reinterpret_cast<const uint32_t*>(restored + o);
        const uint32_t rw[3] = {r4[0], r4[1], r4[2]};
        unpack12(rw, px);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) px[e][ch] = min(max(px[e][ch] + ((res[ch][k][e] + 32) >> 6), 0), 255);
        uint32_t ow[3];
        pack12(px, ow);
        uint32_t* o4 = reinterpret_cast<uint32_t*>(out + o);
        o4[0] = ow[0];
        o4[1] = ow[1];
        o4[2] = ow[2];
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (x + e >= S) continue;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch)
            out[o + 3 * e + ch] = (uint8_t)min(max((int)restored[o + 3 * e + ch] + ((res[ch][k][e] + 32) >> 6), 0), 255);
        }
      }
    }
  }
}

// levels == 1: out = clamp(restored + ((d + 32) >> 6)) from the planar plane.  grid (ceil(S^2 / 1024), F), a thread per 4 pixels.
// VEC (S % 4 == 0, 4-byte aligned uint8 buffers): three dwords of `restored`, one 8-byte load per channel of the plane, three dwords out.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void wavelet_apply_kernel(const uint8_t* restored, uint8_t* out, const int16_t* d16, int S) {
  const int64_t f = blockIdx.y, plane = (int64_t)S * S;
  const int64_t p0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
  if (p0 >= plane) return;
  if (VEC) {   // plane % 4 == 0: the group lies wholly inside
    const int64_t o = (f * plane + p0) * 3;
    const uint32_t* r4 = reinterpret_cast<const uint32_t*>(restored + o);
    const uint32_t rw[3] = {r4[0], r4[1], r4[2]};
    int px[4][3];
    unpack12(rw, px);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const short4_t d = *reinterpret_cast<const short4_t*>(d16 + (f * 3 + ch) * plane + p0);
#pragma unroll
      for (int e = 0; e < 4; ++e) px[e][ch] = min(max(px[e][ch] + (((int)d.v[e] + 32) >> 6), 0), 255);
    }
    uint32_t ow[3];
    pack12(px, ow);
    uint32_t* o4 = reinterpret_cast<uint32_t*>(out + o);
    o4[0] = ow[0];
    o4[1] = ow[1];
    o4[2] = ow[2];
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t p = p0 + e;
    if (p >= plane) return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int64_t o = (f * plane + p) * 3 + ch;
      out[o] = (uint8_t)min(max((int)restored[o] + (((int)d16[(f * 3 + ch) * plane + p] + 32) >> 6), 0), 255);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- stats
// The thread's q-th group of 4 pixels of face f: flat pixel index p (pixels past the plane are not read), as c / r values.
template <bool VEC>
__device__ __forceinline__ void load_group(const uint8_t* crop, const uint8_t* restored, int64_t base, int64_t p, int64_t plane, int c[4][3],
                                           int r[4][3]) {
  if (VEC) {   // plane % 4 == 0: a group lies wholly inside
    const uint32_t* c4 = crop ? reinterpret_cast<const uint32_t*>(crop + (base + p) * 3) : nullptr;
    const uint32_t* r4 = reinterpret_cast<const uint32_t*>(restored + (base + p) * 3);
    const uint32_t rw[3] = {r4[0], r4[1], r4[2]};
    unpack12(rw, r);
    if (crop) {
      const uint32_t cw[3] = {c4[0], c4[1], c4[2]};
      unpack12(cw, c);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = p + e < plane;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        r[e][ch] = in ? restored[(base + p + e) * 3 + ch] : 0;
        if (crop) c[e][ch] = in ? crop[(base + p + e) * 3 + ch] : 0;
      }
    }
  }
}

// sums[f][16] += {N, then per channel S1c, S2c, S1r, S2r} over the valid pixels.  grid (ceil(S^2 / 4096), F).
template <bool VEC>
__global__ __launch_bounds__(kThreads) void stats_reduce_kernel(const uint8_t* crop, const uint8_t* restored, unsigned long long* sums,
                                                                 const int32_t* tables, const vsp_face_item* items, int S) {
  __shared__ uint32_t part[kThreads / 64][13];
  const int64_t f = blockIdx.y, plane = (int64_t)S * S;
  const int32_t* tab = nullptr;
  int pw = 0, ph = 0;
  if (items) {
    const vsp_face_item it = items[f];
    tab = tables + it.tab_off;
    pw = it.w, ph = it.h;
  }
  uint32_t acc[13];
#pragma unroll
  for (int k = 0; k < 13; ++k) acc[k] = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t p = ((int64_t)blockIdx.x * kChunk + q * (kThreads * 4)) + (int64_t)threadIdx.x * 4;
    if (p >= plane) break;
    int c[4][3], r[4][3];
    load_group<VEC>(crop, restored, f * plane, p, plane, c, r);
    int y = (int)(p / S), x = (int)(p - (int64_t)y * S);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (p + e < plane && valid_px(tab, S, pw, ph, x, y)) {
        acc[0] += 1;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          acc[1 + 4 * ch] += (uint32_t)c[e][ch];
          acc[2 + 4 * ch] += (uint32_t)(c[e][ch] * c[e][ch]);
          acc[3 + 4 * ch] += (uint32_t)r[e][ch];
          acc[4 + 4 * ch] += (uint32_t)(r[e][ch] * r[e][ch]);
        }
      }
      if (++x == S) x = 0, ++y;
    }
  }
  // 16 pixels x 255^2 per thread, x 256 threads: below 2^32
#pragma unroll
  for (int k = 0; k < 13; ++k) {
    uint32_t v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 13) {
    unsigned long long v = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) v += part[w][threadIdx.x];
    if (v) atomicAdd(sums + f * 16 + threadIdx.x, v);
  }
}

__device__ __forceinline__ uint64_t isqrt_u64(uint64_t x) {   // exact floor(sqrt(x))
  uint64_t r = 0, bit = 1ull << 62;
  while (bit > x) bit >>= 2;
  while (bit) {
    if (x >= r + bit) {
      x -= r + bit;
      r = (r >> 1) + bit;
    } else {
      r >>= 1;
    }
    bit >>= 2;
  }
  return r;
}

// out = clamp((g (r 256 - mr) + mc 4096 + 2^19) >> 20); threads 0..2 finish g, mr, mc of their channel first.  Same grid as the reduction.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void stats_apply_kernel(const uint8_t* restored, uint8_t* out, const unsigned long long* sums, int S) {
  __shared__ int kg[3], kmr[3], kmc[3];
  const int64_t f = blockIdx.y, plane = (int64_t)S * S;
  if (threadIdx.x < 3) {
    const unsigned long long* m = sums + f * 16;
    const uint64_t N = m[0];
    int g = 4096, mr = 0, mc = 0;   // N == 0: (4096 (256 r) + 2^19) >> 20 = r
    if (N) {
      const uint64_t S1c = m[1 + 4 * threadIdx.x], S2c = m[2 + 4 * threadIdx.x], S1r = m[3 + 4 * threadIdx.x], S2r = m[4 + 4 * threadIdx.x];
      const uint64_t vc = ((N * S2c - S1c * S1c) * 256ull) / (N * N), vr = ((N * S2r - S1r * S1r) * 256ull) / (N * N);
      const uint64_t root = isqrt_u64((vc << 24) / (vr ? vr : 1ull));
      g = (int)(root < 1024ull ? 1024ull : root > 16384ull ? 16384ull : root);
      mc = (int)((S1c * 256ull + N / 2) / N);
      mr = (int)((S1r * 256ull + N / 2) / N);
    }
    kg[threadIdx.x] = g, kmr[threadIdx.x] = mr, kmc[threadIdx.x] = mc;
  }
  __syncthreads();
  const int g[3] = {kg[0], kg[1], kg[2]}, mr[3] = {kmr[0], kmr[1], kmr[2]}, mc[3] = {kmc[0], kmc[1], kmc[2]};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t p = ((int64_t)blockIdx.x * kChunk + q * (kThreads * 4)) + (int64_t)threadIdx.x * 4;
    if (p >= plane) break;
    int c[4][3], r[4][3];
    load_group<VEC>(nullptr, restored, f * plane, p, plane, c, r);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        // clamped in Q20 BEFORE the shift, which gives the same byte: written as clamp(x >> 20, 0, 255) the compiler packs two results
        // with v_ashr_pk_u8_i32 and ORs the other two bytes onto its result as if the upper half were zero, while the MI355X keeps
        // the destination's old upper half there -- bytes 2 and 3 of every dword came out ORed with stale bits
        const int v20 = g[ch] * (r[e][ch] * 256 - mr[ch]) + mc[ch] * 4096 + (1 << 19);
        r[e][ch] = (int)((unsigned)min(max(v20, 0), (256 << 20) - 1) >> 20);
      }
    uint8_t* o = out + (f * plane + p) * 3;
    if (VEC) {
      uint32_t ow[3];
      pack12(r, ow);
      uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
      o4[0] = ow[0];
      o4[1] = ow[1];
      o4[2] = ow[2];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (p + e >= plane) break;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[3 * e + ch] = (uint8_t)r[e][ch];
      }
    }
  }
}

bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  return pa < pb + nb && pb < pa + na;
}

int lds_bytes(bool first, int s) {
  const int sp = (s + 3) & ~3, rows = kTH + 2 * s, WA = kTW + 2 * sp;
  return ((first ? 3 : 1) * rows * WA + rows * kTW) * 2;
}

template <bool FIRST, bool LAST>
void launch_level(bool vec, dim3 grid, hipStream_t st, const uint8_t* crop, const uint8_t* restored, uint8_t* out, const int16_t* src16,
                  int16_t* dst16, const int32_t* tables, const vsp_face_item* items, int S, int s) {
  const int lds = lds_bytes(FIRST, s);   // at most 36864 bytes (s = 32)
  if (vec)
    wavelet_level_kernel<FIRST, LAST, true><<<grid, kThreads, lds, st>>>(crop, restored, out, src16, dst16, tables, items, S, s);
  else
    wavelet_level_kernel<FIRST, LAST, false><<<grid, kThreads, lds, st>>>(crop, restored, out, src16, dst16, tables, items, S, s);
}

}  // namespace

extern "C" {

int vsp_color_fix_u8(const uint8_t* crop, const uint8_t* restored, uint8_t* out, int F, int S, int mode, int levels,
                     const vsp_face_item* items, const vsp_face_item* items_dev, const int32_t* tables, const int32_t* tables_dev,
                     size_t table_ints, void* scratch, size_t scratch_bytes, vsp_stream_t stream) {
  VSP_REQUIRE(mode == VSP_COLOR_FIX_STATS || mode == VSP_COLOR_FIX_WAVELET, "color_fix: unknown mode %d", mode);
  VSP_REQUIRE(levels >= 1 && levels <= VSP_COLOR_FIX_MAX_LEVELS, "color_fix: levels 1..%d (got %d)", VSP_COLOR_FIX_MAX_LEVELS, levels);
  VSP_REQUIRE(F >= 0 && F <= VSP_FACE_MAX_ITEMS, "color_fix: 0..%d faces (got %d)", VSP_FACE_MAX_ITEMS, F);
  VSP_REQUIRE(S >= 1 && S <= VSP_FACE_MAX_SIDE, "color_fix: crop side 1..%d (got %d)", VSP_FACE_MAX_SIDE, S);
  if (mode == VSP_COLOR_FIX_STATS && S > VSP_COLOR_FIX_STATS_MAX_SIDE)
    return vsp::fail(VSP_ENOTSUP, "color_fix: the statistics serve a crop side up to %d (got %d)", VSP_COLOR_FIX_STATS_MAX_SIDE, S);
  if (F == 0) return VSP_OK;
  VSP_REQUIRE(crop && restored && out && scratch, "color_fix: null pointer");
  const uint64_t px = (uint64_t)F * (uint64_t)S * (uint64_t)S, bytes = 3ull * px;
  const uint64_t need = mode == VSP_COLOR_FIX_WAVELET ? 12ull * px : 128ull * (uint64_t)F;
  VSP_REQUIRE(bytes < kTwoGiB && need < kTwoGiB, "color_fix: the crops and the scratch must each stay below 2 GiB (%d faces of %d x %d)", F, S, S);
  VSP_REQUIRE((uint64_t)scratch_bytes >= need, "color_fix: scratch too small (%zu bytes, %llu needed)", scratch_bytes, (unsigned long long)need);
  VSP_REQUIRE(vsp::aligned16(scratch), "color_fix: misaligned scratch");
  VSP_REQUIRE((out == restored || !overlap(out, bytes, restored, bytes)) && !overlap(out, bytes, crop, bytes),
              "color_fix: out overlaps an input (it may only be `restored` itself)");
  VSP_REQUIRE(!overlap(scratch, need, out, bytes) && !overlap(scratch, need, crop, bytes) && !overlap(scratch, need, restored, bytes),
              "color_fix: scratch overlaps a crop buffer");
  const bool planned = items || items_dev || tables || tables_dev;
  if (planned) {
    VSP_REQUIRE(items && items_dev && tables && tables_dev, "color_fix: null pointer (items and tables: all four or none)");
    VSP_REQUIRE((reinterpret_cast<uintptr_t>(tables_dev) & 3u) == 0 && (reinterpret_cast<uintptr_t>(items_dev) & 7u) == 0,
                "color_fix: misaligned tables or items");
    VSP_REQUIRE((uint64_t)table_ints * 4ull < kTwoGiB, "color_fix: the tables must stay below 2 GiB");
    for (int i = 0; i < F; ++i) {
      const vsp_face_item& it = items[i];
      VSP_REQUIRE(it.w > 0 && it.h > 0, "color_fix: face %d: photo size %d x %d", i, it.w, it.h);
      VSP_REQUIRE(it.nx == S && it.ny == S, "color_fix: face %d: tables of %d x %d for a crop of side %d", i, it.nx, it.ny, S);
      const int rc = vspface::check_tables("color_fix", i, it, tables, table_ints);
      if (rc != VSP_OK) return rc;
    }
  }
  hipStream_t st = vsp::as_stream(stream);
  const bool vec = S % 4 == 0 && ((reinterpret_cast<uintptr_t>(crop) | reinterpret_cast<uintptr_t>(restored) | reinterpret_cast<uintptr_t>(out)) & 3u) == 0;
  if (mode == VSP_COLOR_FIX_STATS) {
    unsigned long long* sums = static_cast<unsigned long long*>(scratch);
    if (hipMemsetAsync(sums, 0, (size_t)need, st) != hipSuccess) return vsp::check_launch("color_fix (clearing the sums)");
    const dim3 grid((unsigned)(((uint64_t)S * S + kChunk - 1) / kChunk), (unsigned)F);
    if (vec) {
      stats_reduce_kernel<true><<<grid, kThreads, 0, st>>>(crop, restored, sums, tables_dev, items_dev, S);
      stats_apply_kernel<true><<<grid, kThreads, 0, st>>>(restored, out, sums, S);
    } else {
      stats_reduce_kernel<false><<<grid, kThreads, 0, st>>>(crop, restored, sums, tables_dev, items_dev, S);
      stats_apply_kernel<false><<<grid, kThreads, 0, st>>>(restored, out, sums, S);
    }
    return vsp::check_launch("color_fix (stats)");
  }
  int16_t* buf[2] = {static_cast<int16_t*>(scratch), static_cast<int16_t*>(scratch) + 3ull * px};
  const dim3 grid((unsigned)((S + kTW - 1) / kTW), (unsigned)((S + kTH - 1) / kTH), (unsigned)F);
  launch_level<true, false>(vec, grid, st, crop, restored, out, nullptr, buf[0], tables_dev, items_dev, S, 1);
  if (levels == 1) {
    const dim3 agrid((unsigned)(((uint64_t)S * S + 4 * kThreads - 1) / (4 * kThreads)), (unsigned)F);
    if (vec)
      wavelet_apply_kernel<true><<<agrid, kThreads, 0, st>>>(restored, out, buf[0], S);
    else
      wavelet_apply_kernel<false><<<agrid, kThreads, 0, st>>>(restored, out, buf[0], S);
    return vsp::check_launch("color_fix (wavelet)");
  }
  int cur = 0;
  for (int l = 1; l < levels - 1; ++l, cur ^= 1)
    launch_level<false, false>(vec, grid, st, crop, restored, out, buf[cur], buf[cur ^ 1], tables_dev, items_dev, S, 1 << l);
  launch_level<false, true>(vec, grid, st, crop, restored, out, buf[cur], nullptr, tables_dev, items_dev, S, 1 << (levels - 1));
  return vsp::check_launch("color_fix (wavelet)");
}

}  // extern "C"

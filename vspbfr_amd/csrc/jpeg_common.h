// The JPEG codec's integer arithmetic that the training degradation (degrade.hip: a round trip in the pixel domain), the file encoder
// (jpeg.hip) and the file decoder (jpeg_decode.hip) share.  Compressor: colour transform, 4:2:0 downsampling with the compressor's edge
// rule, ISLOW forward DCT, the quality-scaled Annex K quantisation tables.  Decompressor: ISLOW inverse DCT with its range limit, fancy
// h2v2 upsampling, YCbCr -> RGB.  Bit-exact against libjpeg / libjpeg-turbo; tests/degrade_ref.py, tests/jpeg_ref.py and
// tests/jpeg_dec_ref.py restate it in NumPy.
#pragma once
#include "vsp_common.h"

namespace vsp_jpeg {

// Integer arithmetic of the Independent JPEG Group's baseline codec as libjpeg / libjpeg-turbo run it by default (ISLOW DCTs,
// 13-bit constants, 2 extra bits between the passes), written from the algorithm descriptions.
constexpr int kConstBits = 13, kPass1Bits = 2;
constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137,
              F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;

__host__ __device__ inline int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// ISLOW forward DCT of 8 values at stride `s`; pass 1 (rows) keeps PASS1_BITS extra bits, pass 2 (columns) removes them
// (jfdctint.c).  The outputs are 8x the orthonormal DCT, which the quantiser's divisor absorbs.
template <bool kPass2>
__host__ __device__ inline void fdct8(int* d, int s) {
  const int tmp0 = d[0] + d[7 * s], tmp7 = d[0] - d[7 * s], tmp1 = d[s] + d[6 * s], tmp6 = d[s] - d[6 * s];
  const int tmp2 = d[2 * s] + d[5 * s], tmp5 = d[2 * s] - d[5 * s], tmp3 = d[3 * s] + d[4 * s], tmp4 = d[3 * s] - d[4 * s];
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  const int sh = kPass2 ? kConstBits + kPass1Bits : kConstBits - kPass1Bits;
  if (kPass2) {
    d[0] = descale(tmp10 + tmp11, kPass1Bits);
    d[4 * s] = descale(tmp10 - tmp11, kPass1Bits);
  } else {
    d[0] = (tmp10 + tmp11) << kPass1Bits;
    d[4 * s] = (tmp10 - tmp11) << kPass1Bits;
  }
  const int z1 = (tmp12 + tmp13) * F0541;
  d[2 * s] = descale(z1 + tmp13 * F0765, sh);
  d[6 * s] = descale(z1 - tmp12 * F1847, sh);
  const int z5 = (tmp4 + tmp5 + tmp6 + tmp7) * F1175;
  const int a1 = -(tmp4 + tmp7) * F0899, a2 = -(tmp5 + tmp6) * F2562;
  const int a3 = -(tmp4 + tmp6) * F1961 + z5, a4 = -(tmp5 + tmp7) * F0390 + z5;
  d[7 * s] = descale(tmp4 * F0298 + a1 + a3, sh);
  d[5 * s] = descale(tmp5 * F2053 + a2 + a4, sh);
  d[3 * s] = descale(tmp6 * F3072 + a2 + a3, sh);
  d[s] = descale(tmp7 * F1501 + a1 + a4, sh);
}

// Annex K tables (ITU-T T.81), natural order, scaled like jpeg_set_quality(q, force_baseline = TRUE): 5000 / q below 50, else 200 - 2q
// percent, (base * scale + 50) / 100 clamped to [1, 255].
__host__ __device__ inline int jpeg_quant(int q, int chroma, int i) {
  const unsigned char luma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
  const unsigned char chrom[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                   99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                   99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
  q = q < 1 ? 1 : q > 100 ? 100 : q;
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
  const int v = ((chroma ? chrom[i] : luma[i]) * scale + 50) / 100;
  return v < 1 ? 1 : v > 255 ? 255 : v;
}

// quantise: round half away from zero of c / (8 q) (jcdctmgr.c; the DCT's outputs carry a factor 8)
__host__ __device__ inline int jpeg_quantise(int c, int q) {
  const int d = q << 3;
  return c < 0 ? -((-c + (d >> 1)) / d) : (c + (d >> 1)) / d;
}

// jccolor.c: 16-bit fixed point, FIX(x) = round(x * 65536); Cb / Cr carry +128 and round with ONE_HALF - 1
__host__ __device__ inline int rgb_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__host__ __device__ inline int rgb_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__host__ __device__ inline int rgb_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

struct JpegGeom {
  int dh, dw, mw, mh, pw, ph, ch, cw;  // image, MCUs across / down, padded size (multiples of 16), real chroma size
};

__host__ __device__ inline JpegGeom jpeg_geom(int dh, int dw) {
  JpegGeom g;
  g.dh = dh, g.dw = dw;
  g.mw = (dw + 15) / 16, g.mh = (dh + 15) / 16;
  g.pw = g.mw * 16, g.ph = g.mh * 16;
  g.cw = (dw + 1) / 2, g.ch = (dh + 1) / 2;
  return g;
}

// Edge rule of the compressor: columns and rows past the image repeat the last one (jcsample.c expand_right_edge, jcprepct.c
// expand_bottom_edge); a chroma row past the last real one repeats the last DOWNSAMPLED row (the pre-processor pads each component to
// a full iMCU after downsampling).  rgb(y, x, R, G, B) reads a pixel inside the image.
template <typename Rgb>
__host__ __device__ inline int jpeg_luma(const JpegGeom& g, int y, int x, const Rgb& rgb) {
  int R, G, B;
  rgb(y < g.dh - 1 ? y : g.dh - 1, x < g.dw - 1 ? x : g.dw - 1, R, G, B);
  return rgb_y(R, G, B);
}

// h2v2 downsampling (jcsample.c h2v2_downsample): the sum of the 2 x 2 cell + the bias 1, 2, 1, 2 ... along the row, >> 2; chroma
// sample (cy, cx) of the padded plane, cy counted in chroma rows
template <typename Rgb>
__host__ __device__ inline void jpeg_chroma_h2v2(const JpegGeom& g, int cy, int cx, const Rgb& rgb, int& cb, int& cr) {
  const int gcy = cy < g.ch - 1 ? cy : g.ch - 1;
  int sb = 0, sr = 0;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      const int y = 2 * gcy + a < g.dh - 1 ? 2 * gcy + a : g.dh - 1, x = 2 * cx + b < g.dw - 1 ? 2 * cx + b : g.dw - 1;
      int R, G, B;
      rgb(y, x, R, G, B);
      sb += rgb_cb(R, G, B), sr += rgb_cr(R, G, B);
    }
  const int bias = (cx & 1) ? 2 : 1;
  cb = (sb + bias) >> 2;
  cr = (sr + bias) >> 2;
}

// ---- the decompressor's half (degrade.hip's round trip and the file decoder jpeg_decode.hip)
// ISLOW inverse DCT of 8 values at stride `s` (jidctint.c).  Pass 1 (columns) leaves PASS1_BITS extra bits; pass 2 (rows) descales by
// CONST_BITS + PASS1_BITS + 3 and applies the post-IDCT range limit: index (x & 1023) of a table that clamps x + 128 to [0, 255] for
// |x| < 512 and wraps beyond, exactly as the library's table does.
__host__ __device__ inline int idct_range_limit(int x) {
  const int i = x & 1023;
  return i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896;
}

template <bool kPass2>
__host__ __device__ inline void idct8(int* d, int s) {
  const int z2e = d[2 * s], z3e = d[6 * s];
  const int z1 = (z2e + z3e) * F0541;
  const int t2 = z1 - z3e * F1847, t3 = z1 + z2e * F0765;
  const int t0 = (d[0] + d[4 * s]) * (1 << kConstBits), t1 = (d[0] - d[4 * s]) * (1 << kConstBits);
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int o0 = d[7 * s], o1 = d[5 * s], o2 = d[3 * s], o3 = d[s];
  const int z5 = (o0 + o1 + o2 + o3) * F1175;
  const int y1 = -(o0 + o3) * F0899, y2 = -(o1 + o2) * F2562;
  const int y3 = -(o0 + o2) * F1961 + z5, y4 = -(o1 + o3) * F0390 + z5;
  o0 = o0 * F0298 + y1 + y3;
  o1 = o1 * F2053 + y2 + y4;
  o2 = o2 * F3072 + y2 + y3;
  o3 = o3 * F1501 + y1 + y4;
  const int sh = kPass2 ? kConstBits + kPass1Bits + 3 : kConstBits - kPass1Bits;
  int r[8] = {descale(t10 + o3, sh), descale(t11 + o2, sh), descale(t12 + o1, sh), descale(t13 + o0, sh),
              descale(t13 - o0, sh), descale(t12 - o1, sh), descale(t11 - o2, sh), descale(t10 - o3, sh)};
  for (int i = 0; i < 8; ++i) d[i * s] = kPass2 ? idct_range_limit(r[i]) : r[i];
}

// jdcolor.c: R = Y + round(1.402 (Cr - 128)), B = Y + round(1.772 (Cb - 128)), G = Y + ((-0.34414 (Cb - 128) - 0.71414 (Cr - 128)) in
// 16-bit fixed point, + ONE_HALF, arithmetic shift), each clamped to [0, 255]
__host__ __device__ inline int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
__host__ __device__ inline void ycc_rgb(int y, int cb, int cr, int& r, int& g, int& b) {
  cb -= 128, cr -= 128;
  r = clamp255(y + ((91881 * cr + 32768) >> 16));
  g = clamp255(y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  b = clamp255(y + ((116130 * cb + 32768) >> 16));
}

// h2v2 fancy upsampling (jdsample.c): each output takes 9/16, 3/16, 3/16, 1/16 of the four nearest chroma samples; column sums
// 3 * nearer row + farther row, then (3 * this + neighbour + 8) >> 4 for even and + 7 for odd output columns.  Rows and columns past
// the real chroma size repeat the last real one (jdmainct.c set_bottom_pointers, the first / last column cases).
template <typename Cs>
__host__ __device__ inline int fancy_h2v2(const JpegGeom& g, int y, int x, const Cs& cs) {
  const int cy = y >> 1, cx = x >> 1;
  const int cn = (y & 1) ? min(cy + 1, g.ch - 1) : max(cy - 1, 0);
  const int nx = (x & 1) ? min(cx + 1, g.cw - 1) : max(cx - 1, 0);
  const int this_sum = 3 * cs(cy, cx) + cs(cn, cx), next_sum = 3 * cs(cy, nx) + cs(cn, nx);
  return (3 * this_sum + next_sum + ((x & 1) ? 7 : 8)) >> 4;
}

}  // namespace vsp_jpeg

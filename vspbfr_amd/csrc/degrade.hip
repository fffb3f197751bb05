// Training degradations for gfx950: the low-quality (LQ) synthesis of the reference's training datasets on the device.
//
// The reference builds each LQ face on the host with cv2 / numpy (dataset.py:327-373 degrade_img, :83-127 without the haze step):
//   blur (cv2.filter2D, 39x39 / 41x41 Gaussian) -> haze -> cv2.resize INTER_LINEAR down -> + Gaussian noise, clip -> JPEG round trip
//   (cv2.imencode / imdecode) -> cv2.resize INTER_LINEAR back up -> round to 8 bits -> (rarely) cv2.cvtColor BGR2GRAY.
// Here one launch per stage serves a whole ragged batch: every item (one LQ image) has its own taps, sizes, noise and JPEG quality in a
// vsp_degrade_item table in device memory, and no stage talks to the host.
//
//   degrade_gt_kernel     uint8 HWC -> fp32 NCHW / 255 (the reference's np.array(img) / 255), optional grey
//   degrade_blur_kernel   K x K correlation (not convolution: cv2.filter2D does not flip), reflect-101 border, haze fused; LDS tile
//                         of 64 x 64 outputs + the (K-1) halo, each thread 16 outputs of one row held in registers
//                         (the only stage with real arithmetic: 2 K^2 flops per output)
//   degrade_down_kernel   cv2 INTER_LINEAR (half-pixel centres, no antialiasing, edge clamp) + sigma * N(0,1) noise (Philox4x32-10 /
//                         Box-Muller, or an injected tensor) + clip + round-half-even to uint8: a planar uint8 image per item
//   degrade_jpeg_mcu_kernel / degrade_jpeg_color_kernel
//                         the pixel domain of a libjpeg baseline round trip at the cv2 / libjpeg defaults, bit-exact in int32:
//                         RGB -> YCbCr (jccolor fixed point), 4:2:0 box downsampling with alternating 1 / 2 bias, ISLOW forward DCT,
//                         quantisation by the quality-scaled Annex K tables, dequantisation, ISLOW inverse DCT with the post-IDCT range
//                         limit; then h2v2 "fancy" triangle upsampling of the chroma and YCbCr -> RGB (jdcolor fixed point).  Huffman
//                         coding is lossless and skipped.  cv2 reads the array as BGR, so channel 0 enters the colour transform as blue.
//   degrade_up_kernel     cv2 INTER_LINEAR back to the training size from the uint8 image / 255, round-half-even(x * 255) / 255,
//                         optional grey (cv2 BGR2GRAY weights on channels 0, 1, 2 = 0.114, 0.587, 0.299)
//
// Bounds: the Python front end (vspbfr_amd/degrade.py) validates every table entry against the buffers it allocates before the upload;
// the kernels clamp every index they derive from a table entry as well, so a bad entry can produce wrong pixels but no stray access.
#include "vsp_common.h"
#include "jpeg_common.h"

namespace {

using namespace vsp_jpeg;

constexpr int kBlurTile = 64;                        // output tile edge
constexpr int kBlurRow = 16;                         // outputs per thread (one row)
constexpr int kBlurLds = kBlurTile + VSP_DEGRADE_MAX_KSIZE - 1;   // 104: tile + halo of the largest kernel
constexpr int kBlurPitch = kBlurLds + 1;             // odd: conflict-free LDS reads

__host__ __device__ inline int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

// ---------------------------------------------------------------------------------------------------------------------- gt / grey
__global__ __launch_bounds__(256) void degrade_gt_kernel(float* __restrict__ out, const uint8_t* __restrict__ hwc, const float* in,
                                                          const int32_t* __restrict__ grey, int B, int H, int W) {
  const int64_t hw = (int64_t)H * W, total = (int64_t)B * hw;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / hw, p = i - b * hw;
    float v[3];
    if (hwc) {
      for (int c = 0; c < 3; ++c) v[c] = (float)hwc[i * 3 + c] / 255.0f;
    } else {
      for (int c = 0; c < 3; ++c) v[c] = in[(b * 3 + c) * hw + p];
    }
    if (grey && grey[b]) {
      const float g = v[0] * 0.114f + v[1] * 0.587f + v[2] * 0.299f;
      v[0] = v[1] = v[2] = g;
    }
    for (int c = 0; c < 3; ++c) out[(b * 3 + c) * hw + p] = v[c];
  }
}

// ---------------------------------------------------------------------------------------------------------------------- blur
// grid (ceil(W / 64), ceil(H / 64), n * 3), 256 threads: thread t computes row t / 4 of the tile, columns 16 (t % 4) .. + 15.
// Per tap row, chunks of 8 / 4 / 2 / 1 taps read a register window of 15 + C values from LDS once (16 C FMAs per 15 + C reads; the
// compiler pairs neighbouring columns into v_pk_fma_f32 and builds the odd-offset pairs with v_pk_mov); the taps are uniform across the
// workgroup (scalar loads).  Each tap row accumulates into its own partial sums, added to the totals once per row (float32 error over
// 41 x 41 taps: two sums of 41 terms instead of one of 1681).  The LDS pitch is odd, so the 64 lanes of a read (16 rows x 4 column
// groups 16 apart) hit 64 different banks.
template <int C>
__device__ __forceinline__ void blur_chunk(float (&part)[kBlurRow], const float* row, const float* tr) {
  float w[kBlurRow + C - 1];
#pragma unroll
  for (int j = 0; j < kBlurRow + C - 1; ++j) w[j] = row[j];
#pragma unroll
  for (int q = 0; q < C; ++q) {
    const float t = tr[q];
#pragma unroll
    for (int j = 0; j < kBlurRow; ++j) part[j] = fmaf(t, w[j + q], part[j]);
  }
}

__global__ __launch_bounds__(256) void degrade_blur_kernel(float* __restrict__ out, const float* __restrict__ gt,
                                                            const float* __restrict__ taps, const vsp_degrade_item* __restrict__ items,
                                                            int B, int H, int W) {
  __shared__ float tile[kBlurLds * kBlurPitch];
  const int n = blockIdx.z / 3, c = blockIdx.z - n * 3;
  const vsp_degrade_item it = items[n];
  const int K = min(max(it.ksize | 1, 1), VSP_DEGRADE_MAX_KSIZE), r = K / 2;
  const int src = min(max(it.src, 0), B - 1);
  const float* plane = gt + ((int64_t)src * 3 + c) * H * W;
  const int x0 = blockIdx.x * kBlurTile, y0 = blockIdx.y * kBlurTile;
  const int lw = kBlurTile + K - 1;
  for (int i = threadIdx.x; i < lw * lw; i += 256) {
    const int ly = i / lw, lx = i - ly * lw;
    tile[ly * kBlurPitch + lx] = plane[(int64_t)reflect101(y0 + ly - r, H) * W + reflect101(x0 + lx - r, W)];
  }
  __syncthreads();
  const int ty = threadIdx.x >> 2, tx = (threadIdx.x & 3) * kBlurRow;
  float acc[kBlurRow];
#pragma unroll
  for (int j = 0; j < kBlurRow; ++j) acc[j] = 0.0f;
  const float* tk = taps + it.tap_off;
  for (int ky = 0; ky < K; ++ky) {
    const float* row = tile + (ty + ky) * kBlurPitch + tx;
    const float* tr = tk + ky * K;
    float part[kBlurRow];
#pragma unroll
    for (int j = 0; j < kBlurRow; ++j) part[j] = 0.0f;
    int kx = 0;
    for (; kx + 8 <= K; kx += 8) blur_chunk<8>(part, row + kx, tr + kx);
    if (kx + 4 <= K) blur_chunk<4>(part, row + kx, tr + kx), kx += 4;
    if (kx + 2 <= K) blur_chunk<2>(part, row + kx, tr + kx), kx += 2;
    if (kx < K) blur_chunk<1>(part, row + kx, tr + kx);
#pragma unroll
    for (int j = 0; j < kBlurRow; ++j) acc[j] += part[j];
  }
  const int y = y0 + ty;
  if (y >= H) return;
  const bool haze = it.flags & VSP_DEGRADE_HAZE;
  const float a = it.alpha, a1 = 1.0f - it.alpha;
  float* o = out + (((int64_t)n * 3 + c) * H + y) * W;
#pragma unroll
  for (int j = 0; j < kBlurRow; ++j) {
    const int x = x0 + tx + j;
    if (x < W) o[x] = haze ? acc[j] * a + a1 : acc[j];
  }
}

// ---------------------------------------------------------------------------------------------------------------------- resize rule
// cv2.resize INTER_LINEAR for float images (imgproc resize.cpp, generic path): scale = 1 / (dst / src) in double,
// f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s.  Columns: s < 0 -> (s, f) = (0, 0); s >= src - 1 -> (src - 1, 0).
// Rows keep their fraction and clamp both source rows into [0, src - 1].  The value is s0 * w0 + s1 * w1 as separately rounded float32
// products and sum, horizontally then vertically (HResizeLinear / VResizeLinear), never contracted to an FMA.
struct Lin {
  int i0, i1;
  float w0, w1;
};

__device__ inline Lin lin_col(int d, double scale, int src) {
#pragma clang fp contract(off)
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) s = 0, f = 0.0f;
  if (s >= src - 1) s = src - 1, f = 0.0f;
  return {s, min(s + 1, src - 1), 1.0f - f, f};
}

__device__ __forceinline__ float lerp2(float s0, float s1, float w0, float w1) {
#pragma clang fp contract(off)
  return s0 * w0 + s1 * w1;
}

__device__ inline Lin lin_row(int d, double scale, int src) {
#pragma clang fp contract(off)
  float f = (float)((d + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f -= (float)s;
  return {min(max(s, 0), src - 1), min(max(s + 1, 0), src - 1), 1.0f - f, f};
}

// ---------------------------------------------------------------------------------------------------------------------- noise
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&r)[4]) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

__device__ __forceinline__ float u01(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-08f; }

// the four normals of one Philox call: Box-Muller on (w0, w1) and (w2, w3), as vsp_keyed_fill_f32 draws them
__device__ inline void normal4(uint32_t q, uint32_t c1, uint64_t sample, uint32_t k0, uint32_t k1, float (&v)[4]) {
  uint32_t w[4];
  philox4x32_10(q, c1, (uint32_t)sample, (uint32_t)(sample >> 32), k0, k1, w);
  const float r0 = sqrtf(-2.0f * logf(u01(w[0]))), r1 = sqrtf(-2.0f * logf(u01(w[2])));
  float s0, cs0, s1, cs1;
  sincosf(6.283185307179586f * u01(w[1]), &s0, &cs0);
  sincosf(6.283185307179586f * u01(w[3]), &s1, &cs1);
  v[0] = r0 * cs0; v[1] = r0 * s0; v[2] = r1 * cs1; v[3] = r1 * s1;
}

// ---------------------------------------------------------------------------------------------------------------------- down
// grid (ceil(max_pixels / 256), n): one thread per output pixel of an item, three channels.  Noise element e = 3 p + c of the item's
// (dh, dw, 3) draw (numpy's randn(h, w, 3) order).
__global__ __launch_bounds__(256) void degrade_down_kernel(uint8_t* __restrict__ lq, float* __restrict__ pre,
                                                            const float* __restrict__ blurred, const float* __restrict__ noise,
                                                            const vsp_degrade_item* __restrict__ items, int H, int W, uint32_t k0,
                                                            uint32_t k1, uint64_t step) {
  const int n = blockIdx.y;
  const vsp_degrade_item it = items[n];
  const int dh = min(max(it.dh, 1), VSP_DEGRADE_MAX_SIZE), dw = min(max(it.dw, 1), VSP_DEGRADE_MAX_SIZE);
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= dh * dw) return;
  const int dy = p / dw, dx = p - dy * dw;
  const Lin cx = lin_col(dx, 1.0 / ((double)dw / W), W), ry = lin_row(dy, 1.0 / ((double)dh / H), H);
  const int64_t plane = (int64_t)H * W;
  const uint32_t c1 = (uint32_t)(step << 2) | ((uint32_t)it.slot & 3u);
  const uint32_t e0 = (uint32_t)p * 3u;
  float nz[8];
  if (!noise && it.sigma != 0.0f) {
    float a[4], b[4];
    normal4(e0 >> 2, c1, (uint64_t)it.sample, k0, k1, a);
    normal4((e0 >> 2) + 1, c1, (uint64_t)it.sample, k0, k1, b);
#pragma unroll
    for (int i = 0; i < 4; ++i) nz[i] = a[i], nz[4 + i] = b[i];
  }
  const float sig = it.sigma / 255.0f;
  const int64_t hw = (int64_t)dh * dw;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* s = blurred + ((int64_t)n * 3 + c) * plane;
    const float* s0 = s + (int64_t)ry.i0 * W;
    const float* s1 = s + (int64_t)ry.i1 * W;
    const float h0 = lerp2(s0[cx.i0], s0[cx.i1], cx.w0, cx.w1);
    const float h1 = lerp2(s1[cx.i0], s1[cx.i1], cx.w0, cx.w1);
    float v = lerp2(h0, h1, ry.w0, ry.w1);
    if (pre) pre[it.pix_off + (int64_t)p * 3 + c] = v;
    const float z = noise ? noise[it.pix_off + (int64_t)p * 3 + c] : (it.sigma != 0.0f ? nz[(e0 & 3u) + c] : 0.0f);
    v = fminf(fmaxf(v + z * sig, 0.0f), 1.0f);
    lq[it.pix_off + c * hw + p] = (uint8_t)rintf(v * 255.0f);
  }
}

// ---------------------------------------------------------------------------------------------------------------------- JPEG
// Integer arithmetic of the Independent JPEG Group's baseline codec as libjpeg / libjpeg-turbo run it by default (ISLOW DCTs,
// 13-bit constants, 2 extra bits between the passes), written from the algorithm descriptions.  The compressor's half is in
// jpeg_common.h, shared with the file encoder (jpeg.hip), and so is the decoder's half, shared with the file decoder (jpeg_decode.hip).
// quantise (jpeg_common.h) and dequantise (jddctmgr.c): what the decoder's IDCT sees
__host__ __device__ inline int jpeg_requant(int c, int q) { return jpeg_quantise(c, q) * q; }

// grid (total MCUs), 64 threads, one 16x16 MCU of a 4:2:0 image (4 Y blocks + Cb + Cr) each.  Edge rule of the compressor: columns and
// rows past the image repeat the last one (jcsample.c expand_right_edge, jcprepct.c expand_bottom_edge); a chroma row past the last
// real one repeats the last DOWNSAMPLED row (the pre-processor pads each component to a full iMCU after downsampling).  The decoded
// samples go to the item's work planes: Y (ph x pw), then Cb and Cr (ph/2 x pw/2).  Thread t owns coefficient / sample t of each of the six blocks in the transform passes (48 threads
// for the 8-vector DCT passes: block t / 8, vector t % 8).
__global__ __launch_bounds__(64) void degrade_jpeg_mcu_kernel(uint8_t* __restrict__ work, const uint8_t* __restrict__ lq,
                                                               const vsp_degrade_item* __restrict__ items, int n) {
  __shared__ int blk[6][64];
  __shared__ int qt[2][64];
  const int m = blockIdx.x, t = threadIdx.x;
  int k = 0;
  for (int i = 1; i < n; ++i)
    if (items[i].mcu0 <= m) k = i;
  const vsp_degrade_item it = items[k];
  const JpegGeom g = jpeg_geom(min(max(it.dh, 1), VSP_DEGRADE_MAX_SIZE), min(max(it.dw, 1), VSP_DEGRADE_MAX_SIZE));
  const int local = m - it.mcu0;
  if (local < 0 || local >= g.mw * g.mh) return;
  const int my = local / g.mw, mx = local - my * g.mw;
  const int64_t hw = (int64_t)g.dh * g.dw;
  const uint8_t* img = lq + it.pix_off;
  qt[0][t] = jpeg_quant(it.quality, 0, t);
  qt[1][t] = jpeg_quant(it.quality, 1, t);
  auto px = [&](int c, int y, int x) -> int { return img[c * hw + (int64_t)y * g.dw + x]; };
  auto rgb = [&](int y, int x, int& R, int& G, int& B) { R = px(2, y, x), G = px(1, y, x), B = px(0, y, x); };
  {  // luma: thread t -> 4 samples of row t / 4
    const int yy = t >> 2;
    for (int j = 0; j < 4; ++j) {
      const int xx = (t & 3) * 4 + j;
      blk[(yy >> 3) * 2 + (xx >> 3)][(yy & 7) * 8 + (xx & 7)] = jpeg_luma(g, my * 16 + yy, mx * 16 + xx, rgb) - 128;
    }
  }
  {  // chroma: thread t -> sample t of the 8x8 Cb and Cr blocks
    int cb, cr;
    jpeg_chroma_h2v2(g, my * 8 + (t >> 3), mx * 8 + (t & 7), rgb, cb, cr);
    blk[4][t] = cb - 128;
    blk[5][t] = cr - 128;
  }
  __syncthreads();
  const int b8 = t >> 3, v8 = t & 7;
  if (t < 48) fdct8<false>(&blk[b8][v8 * 8], 1);
  __syncthreads();
  if (t < 48) fdct8<true>(&blk[b8][v8], 8);
  __syncthreads();
  for (int b = 0; b < 6; ++b) blk[b][t] = jpeg_requant(blk[b][t], qt[b >= 4][t]);
  __syncthreads();
  if (t < 48) idct8<false>(&blk[b8][v8], 8);
  __syncthreads();
  if (t < 48) idct8<true>(&blk[b8][v8 * 8], 1);
  __syncthreads();
  uint8_t* yp = work + it.jpg_off;
  uint8_t* cp = yp + (int64_t)g.ph * g.pw;
  const int64_t chw = (int64_t)(g.ph / 2) * (g.pw / 2);
  for (int b = 0; b < 4; ++b) {
    const int yy = (b >> 1) * 8 + (t >> 3), xx = (b & 1) * 8 + (t & 7);
    yp[(int64_t)(my * 16 + yy) * g.pw + mx * 16 + xx] = (uint8_t)blk[b][t];
  }
  const int64_t co = (int64_t)(my * 8 + (t >> 3)) * (g.pw / 2) + mx * 8 + (t & 7);
  cp[co] = (uint8_t)blk[4][t];
  cp[chw + co] = (uint8_t)blk[5][t];
}

// grid (ceil(max_pixels / 256), n): fancy upsampling + YCbCr -> RGB of one pixel, written back over the item's planar uint8 image
__global__ __launch_bounds__(256) void degrade_jpeg_color_kernel(uint8_t* __restrict__ lq, const uint8_t* __restrict__ work,
                                                                  const vsp_degrade_item* __restrict__ items) {
  const vsp_degrade_item it = items[blockIdx.y];
  const JpegGeom g = jpeg_geom(min(max(it.dh, 1), VSP_DEGRADE_MAX_SIZE), min(max(it.dw, 1), VSP_DEGRADE_MAX_SIZE));
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= g.dh * g.dw) return;
  const int y = p / g.dw, x = p - y * g.dw;
  const uint8_t* yp = work + it.jpg_off;
  const uint8_t* cb = yp + (int64_t)g.ph * g.pw;
  const int cpw = g.pw / 2;
  const uint8_t* cr = cb + (int64_t)(g.ph / 2) * cpw;
  const int Y = yp[(int64_t)y * g.pw + x];
  const int Cb = fancy_h2v2(g, y, x, [&](int r, int c) -> int { return cb[(int64_t)r * cpw + c]; });
  const int Cr = fancy_h2v2(g, y, x, [&](int r, int c) -> int { return cr[(int64_t)r * cpw + c]; });
  int R, G, B;
  ycc_rgb(Y, Cb, Cr, R, G, B);
  uint8_t* o = lq + it.pix_off;
  const int64_t hw = (int64_t)g.dh * g.dw;
  o[p] = (uint8_t)B;
  o[hw + p] = (uint8_t)G;
  o[2 * hw + p] = (uint8_t)R;
}

// ---------------------------------------------------------------------------------------------------------------------- up
// grid (ceil(H * W / 256), n): np.float32(u8) / 255 -> cv2 INTER_LINEAR to (H, W) -> np.clip(round(x * 255), 0, 255) / 255
__global__ __launch_bounds__(256) void degrade_up_kernel(float* __restrict__ out, const uint8_t* __restrict__ lq,
                                                          const vsp_degrade_item* __restrict__ items, int H, int W) {
  const int n = blockIdx.y;
  const vsp_degrade_item it = items[n];
  const int dh = min(max(it.dh, 1), VSP_DEGRADE_MAX_SIZE), dw = min(max(it.dw, 1), VSP_DEGRADE_MAX_SIZE);
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= H * W) return;
  const int y = p / W, x = p - y * W;
  const Lin cx = lin_col(x, 1.0 / ((double)W / dw), dw), ry = lin_row(y, 1.0 / ((double)H / dh), dh);
  const uint8_t* img = lq + it.pix_off;
  const int64_t hw = (int64_t)dh * dw;
  float o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint8_t* s0 = img + c * hw + (int64_t)ry.i0 * dw;
    const uint8_t* s1 = img + c * hw + (int64_t)ry.i1 * dw;
    const float h0 = lerp2((float)s0[cx.i0] / 255.0f, (float)s0[cx.i1] / 255.0f, cx.w0, cx.w1);
    const float h1 = lerp2((float)s1[cx.i0] / 255.0f, (float)s1[cx.i1] / 255.0f, cx.w0, cx.w1);
    const float v = lerp2(h0, h1, ry.w0, ry.w1);
    o[c] = fminf(fmaxf(rintf(v * 255.0f), 0.0f), 255.0f) / 255.0f;
  }
  if (it.flags & VSP_DEGRADE_GREY) o[0] = o[1] = o[2] = o[0] * 0.114f + o[1] * 0.587f + o[2] * 0.299f;
  const int64_t plane = (int64_t)H * W;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[((int64_t)n * 3 + c) * plane + p] = o[c];
}

int grid_stream(int64_t work) {
  int64_t b = (work + 255) / 256;
  return (int)(b < 1 ? 1 : b > vsp::kMaxStreamBlocks ? vsp::kMaxStreamBlocks : b);
}

}  // namespace

extern "C" {

int vsp_degrade_gt_f32(float* out, const uint8_t* hwc, const float* in, const int32_t* grey, int B, int H, int W, vsp_stream_t stream) {
  VSP_REQUIRE(B >= 0 && H > 0 && W > 0 && H <= VSP_DEGRADE_MAX_SIZE && W <= VSP_DEGRADE_MAX_SIZE, "degrade_gt: bad shape B=%d H=%d W=%d", B,
              H, W);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(out && (hwc != nullptr) != (in != nullptr), "degrade_gt: need out and exactly one of hwc / in");
  degrade_gt_kernel<<<grid_stream((int64_t)B * H * W), 256, 0, vsp::as_stream(stream)>>>(out, hwc, in, grey, B, H, W);
  return vsp::check_launch("degrade_gt");
}

int vsp_degrade_blur_f32(float* out, const float* gt, const float* taps, const vsp_degrade_item* items, int n, int B, int H, int W,
                         vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && n <= VSP_DEGRADE_MAX_ITEMS, "degrade_blur: %d items (max %d)", n, VSP_DEGRADE_MAX_ITEMS);
  VSP_REQUIRE(B > 0 && H > 0 && W > 0 && H <= VSP_DEGRADE_MAX_SIZE && W <= VSP_DEGRADE_MAX_SIZE, "degrade_blur: bad shape B=%d H=%d W=%d", B,
              H, W);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(out && gt && taps && items, "degrade_blur: null pointer");
  dim3 grid((W + kBlurTile - 1) / kBlurTile, (H + kBlurTile - 1) / kBlurTile, n * 3);
  degrade_blur_kernel<<<grid, 256, 0, vsp::as_stream(stream)>>>(out, gt, taps, items, B, H, W);
  return vsp::check_launch("degrade_blur");
}

int vsp_degrade_down_u8(uint8_t* lq, float* pre, const float* blurred, const float* noise, const vsp_degrade_item* items, int n, int H,
                        int W, int max_pixels, uint64_t seed, int64_t step, vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && n <= VSP_DEGRADE_MAX_ITEMS, "degrade_down: %d items (max %d)", n, VSP_DEGRADE_MAX_ITEMS);
  VSP_REQUIRE(H > 0 && W > 0 && H <= VSP_DEGRADE_MAX_SIZE && W <= VSP_DEGRADE_MAX_SIZE, "degrade_down: bad source size %dx%d", H, W);
  VSP_REQUIRE(max_pixels > 0 && max_pixels <= VSP_DEGRADE_MAX_SIZE * VSP_DEGRADE_MAX_SIZE, "degrade_down: bad max_pixels %d", max_pixels);
  VSP_REQUIRE(step >= 0, "degrade_down: negative step");
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(lq && blurred && items, "degrade_down: null pointer");
  dim3 grid((max_pixels + 255) / 256, n);
  degrade_down_kernel<<<grid, 256, 0, vsp::as_stream(stream)>>>(lq, pre, blurred, noise, items, H, W,
                                                                (uint32_t)seed ^ VSP_DEGRADE_NOISE_KEY, (uint32_t)(seed >> 32),
                                                                (uint64_t)step);
  return vsp::check_launch("degrade_down");
}

int vsp_degrade_jpeg_u8(uint8_t* lq, uint8_t* work, const vsp_degrade_item* items, int n, int total_mcus, int max_pixels,
                        vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && n <= VSP_DEGRADE_MAX_ITEMS, "degrade_jpeg: %d items (max %d)", n, VSP_DEGRADE_MAX_ITEMS);
  VSP_REQUIRE(total_mcus >= 0 && max_pixels > 0 && max_pixels <= VSP_DEGRADE_MAX_SIZE * VSP_DEGRADE_MAX_SIZE,
              "degrade_jpeg: bad sizes (total_mcus %d, max_pixels %d)", total_mcus, max_pixels);
  if (n == 0 || total_mcus == 0) return VSP_OK;
  VSP_REQUIRE(lq && work && items, "degrade_jpeg: null pointer");
  degrade_jpeg_mcu_kernel<<<total_mcus, 64, 0, vsp::as_stream(stream)>>>(work, lq, items, n);
  int rc = vsp::check_launch("degrade_jpeg_mcu");
  if (rc != VSP_OK) return rc;
  dim3 grid((max_pixels + 255) / 256, n);
  degrade_jpeg_color_kernel<<<grid, 256, 0, vsp::as_stream(stream)>>>(lq, work, items);
  return vsp::check_launch("degrade_jpeg_color");
}

int vsp_degrade_up_f32(float* out, const uint8_t* lq, const vsp_degrade_item* items, int n, int H, int W, vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && n <= VSP_DEGRADE_MAX_ITEMS, "degrade_up: %d items (max %d)", n, VSP_DEGRADE_MAX_ITEMS);
  VSP_REQUIRE(H > 0 && W > 0 && H <= VSP_DEGRADE_MAX_SIZE && W <= VSP_DEGRADE_MAX_SIZE, "degrade_up: bad output size %dx%d", H, W);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(out && lq && items, "degrade_up: null pointer");
  dim3 grid((H * W + 255) / 256, n);
  degrade_up_kernel<<<grid, 256, 0, vsp::as_stream(stream)>>>(out, lq, items, H, W);
  return vsp::check_launch("degrade_up");
}

}  // extern "C"

// Face detection for whole photos with the ResNet-50 backbone: RetinaFace's `Resnet50` network on f16 operands.
//   r50_stem_kernel   u8 RGB photos where they lie -> BGR minus the mean, zero outside the photo (the canvas is never stored), 7x7 / 2 / pad 3,
//                     3 -> 64, + bias, ReLU; fp32 fmaf, f16 NHWC out
//   r50_pool_kernel   3x3 / 2 / pad 1 max pool on f16 NHWC; a tap outside the map does not take part
//   r50_conv_kernel   everything between stem and heads as one implicit GEMM on v_mfma_f32_16x16x32_f16: 1x1 and 3x3 (pad 1), stride 1 or 2,
//                     Cin and Cout multiples of 64 up to 2048, + fp32 bias, [+ residual] [ReLU] [+ the coarser level at (y >> 1, x >> 1)],
//                     one rounding to f16, written into a channel window of the output tensor
//   r50_heads_kernel  the three 1x1 heads of one level, 256 -> 32 in fp32 fmaf, written as priors p0 + 2 cell + anchor
// Activations are (B, H, W, pitch) _Float16; a tensor is a pointer, a channel pitch and a channel offset.
//
// r50_conv_kernel: 256 threads, one workgroup per 128 output pixels x 64 output channels.  The GEMM's M dimension is the flat output pixel
// index b OH OW + oy OW + ox across the batch, so the small maps of the coarse levels still fill tiles and a pixel's sum does not depend
// on where in a batch (or a tile) it lies: K = taps x Cin is walked tap by tap in steps of 32 channels, always in that order, by the one
// wave that owns the pixel.  There is no split of K and no atomic.  Wave v owns pixels 32 v .. 32 v + 31 of the tile and all 64 channels:
// 2 x 4 accumulator blocks.  The WEIGHTS are the MFMA's A operand and the pixels its B operand, so a lane holds four consecutive output
// channels of one pixel (column = lane & 15 = pixel, row = 4 (lane >> 4) + r = channel of the block) and stores 8 bytes per block.  Both
// operands come straight from memory, 16 bytes per lane: a pixel fragment is 64 consecutive bytes of each of 16 pixels, a weight
// fragment 1 KiB of consecutive bytes of the packed image (as parse.hip and rrdb.hip read theirs); the next step's fragments are fetched
// before the current step's MFMAs.  Padding and the tile's tail are resolved in the address (clamped, so every load is in bounds and
// unconditional) and a select.
#include "vsp_common.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int64_t kTwoGiB = (int64_t)1 << 31;
constexpr int kTilePx = 128, kTileCo = 64;

// ---------------------------------------------------------------------------------------------------------------------------- stem
// w: (147, 64) fp32, row (7 ky + kx) 3 + network channel (B, G, R).
__global__ __launch_bounds__(256) void r50_stem_kernel(_Float16* __restrict__ y, const uint8_t* __restrict__ src,
                                                       const vsp_det_src* __restrict__ items, const float* __restrict__ wt,
                                                       const float* __restrict__ bias, int OH, int OW) {
  __shared__ __attribute__((aligned(16))) float sw[147 * 64];
  __shared__ __attribute__((aligned(16))) float sb[64];
  for (int i = threadIdx.x; i < 147 * 64; i += 256) sw[i] = wt[i];
  if (threadIdx.x < 64) sb[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const vsp_det_src it = items[blockIdx.y];
  const int P = OH * OW, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int oy = p / OW, ox = p - oy * OW;
  float acc[64];
#pragma unroll
  for (int co = 0; co < 64; ++co) acc[co] = sb[co];
  const uint8_t* ph = src + it.off;
  const float mean[3] = {104.f, 117.f, 123.f};
  for (int ky = 0; ky < 7; ++ky) {
    const int iy = 2 * oy - 3 + ky;
    if (iy < 0 || iy >= it.h) continue;
    for (int kx = 0; kx < 7; ++kx) {
      const int ix = 2 * ox - 3 + kx;
      if (ix < 0 || ix >= it.w) continue;
      const uint8_t* px = ph + ((int64_t)iy * it.w + ix) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = (float)px[2 - c] - mean[c];          // network channel c is B, G, R
        const float4* wr = reinterpret_cast<const float4*>(sw + ((ky * 7 + kx) * 3 + c) * 64);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float4 w4 = wr[q];
          acc[4 * q] = fmaf(w4.x, v, acc[4 * q]);
          acc[4 * q + 1] = fmaf(w4.y, v, acc[4 * q + 1]);
          acc[4 * q + 2] = fmaf(w4.z, v, acc[4 * q + 2]);
          acc[4 * q + 3] = fmaf(w4.w, v, acc[4 * q + 3]);
        }
      }
    }
  }
  half4* yo = reinterpret_cast<half4*>(y + ((int64_t)it.slot * P + p) * 64);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    half4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (_Float16)fmaxf(acc[4 * q + j], 0.f);
    yo[q] = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------- pool
// One thread per output pixel and group of 8 channels.  A tap outside the map is clamped onto the border row / column, which lies in
// the window already: the maximum is that of the taps inside.
__global__ __launch_bounds__(256) void r50_pool_kernel(_Float16* __restrict__ y, const _Float16* __restrict__ x, int64_t n, int C8, int H,
                                                       int W, int OH, int OW) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int g = (int)(i % C8);
  int64_t m = i / C8;
  const int ox = (int)(m % OW);
  m /= OW;
  const int oy = (int)(m % OH), b = (int)(m / OH);
  half8 best;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = min(max(2 * oy - 1 + ky, 0), H - 1);
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = min(max(2 * ox - 1 + kx, 0), W - 1);
      const half8 v = *reinterpret_cast<const half8*>(x + (((int64_t)b * H + iy) * W + ix) * (C8 * 8) + g * 8);
      if (ky == 0 && kx == 0) best = v;
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) best[j] = v[j] > best[j] ? v[j] : best[j];
      }
    }
  }
  *reinterpret_cast<half8*>(y + i * 8) = best;
}

// ------------------------------------------------------------------------------------------------------------------- convolution
struct ConvArgs {
  _Float16* y;              // + y_off
  const _Float16* x;        // + x_off
  const _Float16* res;      // + res_off, added before the activation, at the output pixel
  const _Float16* up;       // + up_off, added behind the activation, at (oy >> 1, ox >> 1) of an (OH / 2, OW / 2) map
  const uint4* wimg;
  const float* bias;
  int y_pitch, x_pitch, res_pitch, up_pitch;
  int H, W, OH, OW;
  int M;                    // B OH OW
  int nkc;                  // Cin / 32
  int nbt;                  // Cout / 16
  int stride, relu;
};

// KS: filter extent, 1 or 3 (padding KS / 2)
template <int KS>
__global__ __launch_bounds__(256) void r50_conv_kernel(const ConvArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lp = lane & 15, lg = lane >> 4;
  const int m0 = blockIdx.x * kTilePx + wv * 32, nb0 = blockIdx.y * (kTileCo / 16);
  const int OHW = a.OH * a.OW;

  // the lane's two pixels (clamped into the batch: the tail's loads are in bounds, its results are not stored)
  int pb[2], py[2], px[2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const int m = min(m0 + mb * 16 + lp, a.M - 1);
    pb[mb] = m / OHW;
    const int r = m - pb[mb] * OHW;
    py[mb] = r / a.OW;
    px[mb] = r - py[mb] * a.OW;
  }

  f32x4 acc[2][4];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const unsigned char* xb = reinterpret_cast<const unsigned char*>(a.x) + lg * 16;
  const unsigned char* wb = reinterpret_cast<const unsigned char*>(a.wimg) + (int64_t)nb0 * 1024 + lane * 16;
  const int64_t wstep = (int64_t)a.nbt * 1024;                // bytes of one K-step of all output channels
  const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

  for (int tap = 0; tap < KS * KS; ++tap) {
    const int ky = tap / KS, kx = tap - ky * KS;
    uint32_t off[2];
    bool in[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int iy = py[mb] * a.stride - KS / 2 + ky, ix = px[mb] * a.stride - KS / 2 + kx;
      in[mb] = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      const int cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);
      off[mb] = (uint32_t)((((int64_t)pb[mb] * a.H + cy) * a.W + cx) * a.x_pitch * 2);
    }
    const unsigned char* pw = wb + (int64_t)tap * a.nkc * wstep;
    half8 pxn[2], wtn[4];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) pxn[mb] = *reinterpret_cast<const half8*>(xb + off[mb]);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) wtn[nb] = *reinterpret_cast<const half8*>(pw + nb * 1024);
    for (int kc = 0; kc < a.nkc; ++kc) {
      half8 pxc[2], wtc[4];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) pxc[mb] = in[mb] ? pxn[mb] : zero;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) wtc[nb] = wtn[nb];
      const int kn = min(kc + 1, a.nkc - 1);                  // the last step fetches itself again: no branch around a load
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) pxn[mb] = *reinterpret_cast<const half8*>(xb + off[mb] + kn * 64);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) wtn[nb] = *reinterpret_cast<const half8*>(pw + kn * wstep + nb * 1024);
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wtc[nb], pxc[mb], acc[mb][nb], 0, 0, 0);
    }
  }

  // epilogue: the lane holds channels 16 (nb0 + nb) + 4 lg + r, r = 0 .. 3, of its pixel of block mb
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const bool inside = m0 + mb * 16 + lp < a.M;
    const int64_t p = ((int64_t)pb[mb] * a.OH + py[mb]) * a.OW + px[mb];
    const int64_t pu = ((int64_t)pb[mb] * (a.OH >> 1) + (py[mb] >> 1)) * (a.OW >> 1) + (px[mb] >> 1);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const int ch = (nb0 + nb) * 16 + lg * 4;
      const float4 b4 = *reinterpret_cast<const float4*>(a.bias + ch);
      float v[4] = {acc[mb][nb][0] + b4.x, acc[mb][nb][1] + b4.y, acc[mb][nb][2] + b4.z, acc[mb][nb][3] + b4.w};
      if (a.res) {
        const half4 q = *reinterpret_cast<const half4*>(a.res + p * a.res_pitch + ch);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)q[r];
      }
      if (a.relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      if (a.up) {
        const half4 q = *reinterpret_cast<const half4*>(a.up + pu * a.up_pitch + ch);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)q[r];
      }
      half4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = (_Float16)v[r];
      if (inside) *reinterpret_cast<half4*>(a.y + p * a.y_pitch + ch) = o;
    }
  }
}

// --------------------------------------------------------------------------------------------------------------------------- heads
// One thread per cell of the flat index b H W + cell.  w: (256, 32) fp32, class (4) | box (8) | landmarks (20) side by side.
__global__ __launch_bounds__(256) void r50_heads_kernel(float* __restrict__ conf, float* __restrict__ loc, float* __restrict__ lm,
                                                        const _Float16* __restrict__ x, int x_pitch, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int HW, int M, int P, int p0) {
  __shared__ __attribute__((aligned(16))) float sw[256 * 32];
  for (int i = threadIdx.x; i < 256 * 32; i += 256) sw[i] = w[i];
  __syncthreads();
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float acc[32];
#pragma unroll
  for (int co = 0; co < 32; ++co) acc[co] = bias[co];
  const half8* xp = reinterpret_cast<const half8*>(x + (int64_t)m * x_pitch);
  for (int c8 = 0; c8 < 32; ++c8) {
    const half8 v8 = xp[c8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = (float)v8[j];
      const float4* wr = reinterpret_cast<const float4*>(sw + (c8 * 8 + j) * 32);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const float4 w4 = wr[q];
        acc[4 * q] = fmaf(w4.x, v, acc[4 * q]);
        acc[4 * q + 1] = fmaf(w4.y, v, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(w4.z, v, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(w4.w, v, acc[4 * q + 3]);
      }
    }
  }
  const int b = m / HW, cell = m - b * HW;
  const int64_t q = (int64_t)b * P + p0 + 2 * cell;          // the cell's first prior: anchors are adjacent
  float* c = conf + q * 2;
  float* l = loc + q * 4;
  float* k = lm + q * 10;
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = acc[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) l[i] = acc[4 + i];
#pragma unroll
  for (int i = 0; i < 20; ++i) k[i] = acc[12 + i];
}

inline bool dims_ok(int B, int H, int W) { return B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= VSP_DET_MAX_SIDE && W <= VSP_DET_MAX_SIDE; }
inline int64_t act_bytes(int B, int H, int W, int pitch) { return (int64_t)B * H * W * pitch * 2; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool overlap(const void* p, int64_t pn, const void* q, int64_t qn) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}

}  // namespace

extern "C" {

int vsp_det50_stem_u8(void* y, const uint8_t* src, size_t src_bytes, const vsp_det_src* items, const vsp_det_src* items_dev, int n,
                      const float* w, const float* b, int B, int Hc, int Wc, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, Hc, Wc), "det50_stem: batch %d, canvas %d x %d (sides 1..%d)", B, Hc, Wc, VSP_DET_MAX_SIDE);
  VSP_REQUIRE(n >= 0 && n <= B, "det50_stem: %d items for a batch of %d", n, B);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(y && src && items && items_dev && w && b, "det50_stem: null pointer");
  VSP_REQUIRE(aligned8(y) && vsp::aligned16(w) && vsp::aligned16(b) && aligned8(items_dev),
              "det50_stem: buffers must be aligned (y and the item table to 8 bytes, weights to 16)");
  const int OH = (Hc + 1) / 2, OW = (Wc + 1) / 2;
  if ((int64_t)src_bytes >= kTwoGiB || act_bytes(B, OH, OW, 64) >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "det50_stem: a buffer of 2 GiB or more");
  for (int i = 0; i < n; ++i) {
    const vsp_det_src& it = items[i];
    VSP_REQUIRE(it.h >= 1 && it.w >= 1 && it.h <= Hc && it.w <= Wc, "det50_stem: item %d: photo %d x %d does not fit the %d x %d canvas", i,
                it.h, it.w, Hc, Wc);
    VSP_REQUIRE(it.off >= 0 && it.off + (int64_t)3 * it.h * it.w <= (int64_t)src_bytes, "det50_stem: item %d: bytes outside src", i);
    VSP_REQUIRE(it.slot >= 0 && it.slot < B, "det50_stem: item %d: slot %d outside 0..%d", i, it.slot, B - 1);
  }
  r50_stem_kernel<<<dim3((OH * OW + 255) / 256, n), 256, 0, vsp::as_stream(stream)>>>(static_cast<_Float16*>(y), src, items_dev, w, b, OH, OW);
  return vsp::check_launch("det50_stem");
}

int vsp_det50_pool_f16(void* y, const void* x, int B, int H, int W, int C, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, H, W), "det50_pool: batch %d, map %d x %d", B, H, W);
  VSP_REQUIRE(C >= 8 && C <= 2048 && C % 8 == 0, "det50_pool: %d channels (a multiple of 8 up to 2048)", C);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(y && x, "det50_pool: null pointer");
  VSP_REQUIRE(vsp::aligned16(y) && vsp::aligned16(x), "det50_pool: buffers must be 16-byte aligned");
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  if (act_bytes(B, H, W, C) >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "det50_pool: a tensor of 2 GiB or more");
  VSP_REQUIRE(!overlap(y, act_bytes(B, OH, OW, C), x, act_bytes(B, H, W, C)), "det50_pool: the output overlaps the input");
  const int64_t n = (int64_t)B * OH * OW * (C / 8);
  r50_pool_kernel<<<(unsigned)((n + 255) / 256), 256, 0, vsp::as_stream(stream)>>>(static_cast<_Float16*>(y), static_cast<const _Float16*>(x), n,
                                                                                    C / 8, H, W, OH, OW);
  return vsp::check_launch("det50_pool");
}

int vsp_det50_conv_f16(void* y, int y_pitch, int y_off, const void* x, int x_pitch, int x_off, int B, int H, int W, int Cin, int Cout,
                       int ksize, int stride, int flags, const void* w_img, const float* b, const void* res, int res_pitch, int res_off,
                       const void* up, int up_pitch, int up_off, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, H, W), "det50_conv: batch %d, map %d x %d", B, H, W);
  VSP_REQUIRE(Cin >= 64 && Cin <= 2048 && Cin % 64 == 0 && Cout >= 64 && Cout <= 2048 && Cout % 64 == 0,
              "det50_conv: %d -> %d channels; multiples of 64 up to 2048 are served", Cin, Cout);
  VSP_REQUIRE(ksize == 1 || ksize == 3, "det50_conv: filter %d x %d (1 x 1 or 3 x 3)", ksize, ksize);
  VSP_REQUIRE(stride == 1 || stride == 2, "det50_conv: stride %d (1 or 2)", stride);
  VSP_REQUIRE((flags & ~VSP_DET50_RELU) == 0, "det50_conv: unknown flags %d", flags);
  VSP_REQUIRE(x_off >= 0 && x_off % 8 == 0 && x_pitch % 8 == 0 && x_pitch <= 4096 && x_off + Cin <= x_pitch,
              "det50_conv: input channels %d..%d of a pitch of %d (offset and pitch multiples of 8)", x_off, x_off + Cin - 1, x_pitch);
  VSP_REQUIRE(y_off >= 0 && y_off % 4 == 0 && y_pitch % 4 == 0 && y_pitch <= 4096 && y_off + Cout <= y_pitch,
              "det50_conv: output channels %d..%d of a pitch of %d (offset and pitch multiples of 4)", y_off, y_off + Cout - 1, y_pitch);
  VSP_REQUIRE(!res || (res_off >= 0 && res_off % 4 == 0 && res_pitch % 4 == 0 && res_pitch <= 4096 && res_off + Cout <= res_pitch),
              "det50_conv: residual channels %d..%d of a pitch of %d (offset and pitch multiples of 4)", res_off, res_off + Cout - 1, res_pitch);
  VSP_REQUIRE(!up || (up_off >= 0 && up_off % 4 == 0 && up_pitch % 4 == 0 && up_pitch <= 4096 && up_off + Cout <= up_pitch),
              "det50_conv: coarser-level channels %d..%d of a pitch of %d (offset and pitch multiples of 4)", up_off, up_off + Cout - 1, up_pitch);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(y && x && w_img && b, "det50_conv: null pointer");
  VSP_REQUIRE(vsp::aligned16(x) && vsp::aligned16(w_img) && vsp::aligned16(b) && aligned8(y) && aligned8(res) && aligned8(up),
              "det50_conv: buffers must be aligned (input, weights, bias to 16 bytes; output, residuals to 8)");
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  VSP_REQUIRE(!up || (OH % 2 == 0 && OW % 2 == 0), "det50_conv: the coarser level needs an even output map, not %d x %d", OH, OW);
  const int64_t xb = act_bytes(B, H, W, x_pitch), yb = act_bytes(B, OH, OW, y_pitch);
  const int64_t rb = res ? act_bytes(B, OH, OW, res_pitch) : 0, ub = up ? act_bytes(B, OH / 2, OW / 2, up_pitch) : 0;
  if (xb >= kTwoGiB || yb >= kTwoGiB || rb >= kTwoGiB || ub >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "det50_conv: a tensor of 2 GiB or more");
  VSP_REQUIRE(!overlap(y, yb, x, xb), "det50_conv: the output overlaps the input");
  // the residual may be the very window the launch writes (each value is read by the lane that then writes it) and nothing else of it
  if (res && overlap(y, yb, res, rb))
    VSP_REQUIRE(res == y && res_pitch == y_pitch && res_off == y_off, "det50_conv: the residual overlaps the output without being its window");
  VSP_REQUIRE(!up || !overlap(y, yb, up, ub), "det50_conv: the coarser level overlaps the output");
  ConvArgs a = {};
  a.y = static_cast<_Float16*>(y) + y_off, a.x = static_cast<const _Float16*>(x) + x_off;
  a.res = res ? static_cast<const _Float16*>(res) + res_off : nullptr, a.up = up ? static_cast<const _Float16*>(up) + up_off : nullptr;
  a.wimg = static_cast<const uint4*>(w_img), a.bias = b;
  a.y_pitch = y_pitch, a.x_pitch = x_pitch, a.res_pitch = res_pitch, a.up_pitch = up_pitch;
  a.H = H, a.W = W, a.OH = OH, a.OW = OW, a.M = B * OH * OW, a.nkc = Cin / 32, a.nbt = Cout / 16;
  a.stride = stride, a.relu = (flags & VSP_DET50_RELU) != 0;
  const dim3 grid((unsigned)((a.M + kTilePx - 1) / kTilePx), (unsigned)(Cout / kTileCo));
  if (ksize == 1)
    r50_conv_kernel<1><<<grid, 256, 0, vsp::as_stream(stream)>>>(a);
  else
    r50_conv_kernel<3><<<grid, 256, 0, vsp::as_stream(stream)>>>(a);
  return vsp::check_launch("det50_conv");
}

int vsp_det50_heads_f32(float* conf, float* loc, float* lm, const void* x, int x_pitch, const float* w, const float* b, int B, int H, int W,
                        int P, int p0, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, H, W), "det50_heads: batch %d, map %d x %d", B, H, W);
  VSP_REQUIRE(p0 >= 0 && P >= 1 && (int64_t)p0 + (int64_t)2 * H * W <= P, "det50_heads: priors %d..%lld of %d", p0,
              (long long)p0 + (long long)2 * H * W - 1, P);
  VSP_REQUIRE(x_pitch >= 256 && x_pitch <= 4096 && x_pitch % 8 == 0, "det50_heads: input pitch %d (at least 256, a multiple of 8)", x_pitch);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(conf && loc && lm && x && w && b, "det50_heads: null pointer");
  VSP_REQUIRE(vsp::aligned16(x) && vsp::aligned16(w), "det50_heads: input and weights must be 16-byte aligned");
  if (act_bytes(B, H, W, x_pitch) >= kTwoGiB || (int64_t)B * P * 40 >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "det50_heads: a tensor of 2 GiB or more");
  const int M = B * H * W;
  r50_heads_kernel<<<(M + 255) / 256, 256, 0, vsp::as_stream(stream)>>>(conf, loc, lm, static_cast<const _Float16*>(x), x_pitch, w, b, H * W, M, P,
                                                                        p0);
  return vsp::check_launch("det50_heads");
}

}  // extern "C"

// Facial landmarks for the LMD column: face_alignment's 2D-FAN (stacked hourglasses, pre-activated blocks) on f16 operands.
//   fan_stem_kernel    u8 RGB photo + box (x0, y0, s) -> bilinear sample to side x side at half-pixel centres, zero outside the photo, / 255
//                      (never stored), 7x7 / 2 / pad 3, 3 -> 64 with the folded BatchNorm, ReLU; fp32 fmaf, f16 NHWC out
//   fan_conv_kernel    every other convolution as one implicit GEMM on v_mfma_f32_16x16x32_f16: 1x1 and 3x3 (pad 1), stride 1, Cin a
//                      multiple of 32 up to 256, Cout a multiple of 32 up to 256 or 68 (the image is padded to 96, the padding is never
//                      stored).  Optional input affine: the operand is f16(max(fmaf(a_c, x, b_c), 0)), a rounding point; a tap outside
//                      the map is zero BEHIND the affine.  v = acc [+ bias] [ReLU]; `raw` takes f16(v), the output takes
//                      v [+ res1] [+ res2] [+ the coarser level at (y >> 1, x >> 1)] rounded once to f16, or as fp32.
//   fan_pool_kernel    2x2 mean of f16 values: ((a + b) + (c + d)) / 4 in fp32, one rounding
//   fan_decode_kernel  one wave per (image, landmark): argmax of the fp32 map (lowest flat index among equals, a non-finite value never
//                      wins), quarter-pixel offset, the point in the box, the peak value, a non-finite flag
// Activations are (B, H, W, pitch) _Float16; a tensor is a pointer, a channel pitch and a channel offset, so a ConvBlock's cat is three
// channel windows of one tensor.
//
// fan_conv_kernel is the arrangement of detect_r50.hip: 256 threads, one workgroup per 128 pixels of the flat index b H W + y W + x and
// 16 NB output channels (NB = 4, or 2 where the padded channel count is no multiple of 64); wave v owns pixels 32 v .. 32 v + 31 and all
// the tile's channels.  The weights are the MFMA's A operand, the pixels its B operand, both read straight from memory 16 bytes per lane;
// the next step's fragments are fetched before the current step's MFMAs.  K = taps x Cin is walked tap by tap in steps of 32 channels by
// the one wave that owns the pixel: no split of K, no atomic, so an image has the same bits at any batch size and position.  Padding and
// the tile's tail are resolved in the address (clamped: every load is in bounds and unconditional) and a select.
#include "vsp_common.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int64_t kTwoGiB = (int64_t)1 << 31;
constexpr int kTilePx = 128;
constexpr int kMaxSide = 4096;
constexpr int kDeepGroups = 512;

// ---------------------------------------------------------------------------------------------------------------------------- stem
// w: (147, 64) fp32, row (7 ky + kx) 3 + channel (R, G, B).  box: (B, 3) fp32 x0, y0, s.  One thread per output pixel.
__global__ __launch_bounds__(256) void fan_stem_kernel(_Float16* __restrict__ y, const uint8_t* __restrict__ src, const float* __restrict__ box,
                                                       const float* __restrict__ wt, const float* __restrict__ bias, int H, int W, int side) {
  __shared__ __attribute__((aligned(16))) float sw[147 * 64];
  __shared__ __attribute__((aligned(16))) float sb[64];
  for (int i = threadIdx.x; i < 147 * 64; i += 256) sw[i] = wt[i];
  if (threadIdx.x < 64) sb[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.y, O = side >> 1, P = O * O, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int oy = p / O, ox = p - oy * O;
  const float x0 = box[3 * b], y0 = box[3 * b + 1], sc = box[3 * b + 2] / (float)side;
  const uint8_t* ph = src + (int64_t)b * H * W * 3;
  float acc[64];
#pragma unroll
  for (int co = 0; co < 64; ++co) acc[co] = sb[co];
  for (int ky = 0; ky < 7; ++ky) {
    const int sy = 2 * oy - 3 + ky;
    if (sy < 0 || sy >= side) continue;
    const float fy = y0 + ((float)sy + 0.5f) * sc - 0.5f;
    const float yf = floorf(fy);
    const float wy1 = fy - yf, wy0 = 1.f - wy1;
    const int iy0 = (int)fminf(fmaxf(yf, -2.f), (float)H), iy1 = iy0 + 1;   // a row outside the photo stays outside after the clamp
    const bool vy0 = iy0 >= 0 && iy0 < H, vy1 = iy1 >= 0 && iy1 < H;
    const int cy0 = min(max(iy0, 0), H - 1), cy1 = min(max(iy1, 0), H - 1);
    for (int kx = 0; kx < 7; ++kx) {
      const int sx = 2 * ox - 3 + kx;
      if (sx < 0 || sx >= side) continue;
      const float fx = x0 + ((float)sx + 0.5f) * sc - 0.5f;
      const float xf = floorf(fx);
      const float wx1 = fx - xf, wx0 = 1.f - wx1;
      const int ix0 = (int)fminf(fmaxf(xf, -2.f), (float)W), ix1 = ix0 + 1;
      const bool vx0 = ix0 >= 0 && ix0 < W, vx1 = ix1 >= 0 && ix1 < W;
      const int cx0 = min(max(ix0, 0), W - 1), cx1 = min(max(ix1, 0), W - 1);
      const uint8_t* p00 = ph + ((int64_t)cy0 * W + cx0) * 3;
      const uint8_t* p01 = ph + ((int64_t)cy0 * W + cx1) * 3;
      const uint8_t* p10 = ph + ((int64_t)cy1 * W + cx0) * 3;
      const uint8_t* p11 = ph + ((int64_t)cy1 * W + cx1) * 3;
      const float w00 = (vy0 && vx0) ? wy0 * wx0 : 0.f, w01 = (vy0 && vx1) ? wy0 * wx1 : 0.f;
      const float w10 = (vy1 && vx0) ? wy1 * wx0 : 0.f, w11 = (vy1 && vx1) ? wy1 * wx1 : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = (w00 * (float)p00[c] + w01 * (float)p01[c] + w10 * (float)p10[c] + w11 * (float)p11[c]) / 255.f;
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
  half4* yo = reinterpret_cast<half4*>(y + ((int64_t)b * P + p) * 64);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    half4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (_Float16)fmaxf(acc[4 * q + j], 0.f);
    yo[q] = o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------- pool
// One thread per output pixel and group of 8 channels.
__global__ __launch_bounds__(256) void fan_pool_kernel(_Float16* __restrict__ y, int y_pitch, const _Float16* __restrict__ x, int x_pitch, int64_t n,
                                                       int C8, int H, int W) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int OH = H >> 1, OW = W >> 1;
  const int g = (int)(i % C8);
  int64_t m = i / C8;
  const int ox = (int)(m % OW);
  m /= OW;
  const int oy = (int)(m % OH), b = (int)(m / OH);
  const _Float16* xp = x + (((int64_t)b * H + 2 * oy) * W + 2 * ox) * x_pitch + g * 8;
  const half8 v00 = *reinterpret_cast<const half8*>(xp), v01 = *reinterpret_cast<const half8*>(xp + x_pitch);
  const half8 v10 = *reinterpret_cast<const half8*>(xp + (int64_t)W * x_pitch), v11 = *reinterpret_cast<const half8*>(xp + (int64_t)(W + 1) * x_pitch);
  half8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (_Float16)(__fmul_rn(__fadd_rn(__fadd_rn((float)v00[j], (float)v01[j]), __fadd_rn((float)v10[j], (float)v11[j])), 0.25f));
  *reinterpret_cast<half8*>(y + (((int64_t)b * OH + oy) * OW + ox) * y_pitch + g * 8) = o;
}

// ------------------------------------------------------------------------------------------------------------------- convolution
struct ConvArgs {
  void* y;                  // + y_off: _Float16 or float
  _Float16* raw;            // + raw_off, or null
  const _Float16* x;        // + x_off
  const _Float16* res1;     // + res1_off, at the output pixel
  const _Float16* res2;
  const _Float16* up;       // + up_off, at (y >> 1, x >> 1) of an (H / 2, W / 2) map
  const uint4* wimg;
  const float* bias;        // or null
  const float* ia;          // input affine (Cin each), or null
  const float* ib;
  int y_pitch, raw_pitch, x_pitch, res1_pitch, res2_pitch, up_pitch;
  int H, W;
  int M;                    // B H W
  int nkc;                  // Cin / 32
  int nbt;                  // padded Cout / 16
  int cout;                 // channels stored
  int relu, y_f32;
};

// the operand of the input affine: f16(max(fmaf(a, x, b), 0)) in fp32; a tap outside the map is zero behind it
__device__ __forceinline__ half8 activate(const half8 v, const float4 a0, const float4 a1, const float4 b0, const float4 b1) {
  half8 o;
  o[0] = (_Float16)fmaxf(__fmaf_rn(a0.x, (float)v[0], b0.x), 0.f);
  o[1] = (_Float16)fmaxf(__fmaf_rn(a0.y, (float)v[1], b0.y), 0.f);
  o[2] = (_Float16)fmaxf(__fmaf_rn(a0.z, (float)v[2], b0.z), 0.f);
  o[3] = (_Float16)fmaxf(__fmaf_rn(a0.w, (float)v[3], b0.w), 0.f);
  o[4] = (_Float16)fmaxf(__fmaf_rn(a1.x, (float)v[4], b1.x), 0.f);
  o[5] = (_Float16)fmaxf(__fmaf_rn(a1.y, (float)v[5], b1.y), 0.f);
  o[6] = (_Float16)fmaxf(__fmaf_rn(a1.z, (float)v[6], b1.z), 0.f);
  o[7] = (_Float16)fmaxf(__fmaf_rn(a1.w, (float)v[7], b1.w), 0.f);
  return o;
}

// KS: filter extent, 1 or 3 (padding KS / 2); NB: blocks of 16 output channels per workgroup; AFF: with the input affine; D: how many
// K-steps' fragments are in flight.  D = 1 fetches one step ahead inside a tap and relies on the other waves of the SIMD to cover the
// latency; D = 3 is for launches too small to fill the chip (the 32 x 32 maps and below), where a wave is alone with its chain of
// taps x Cin / 32 dependent fetches: a ring of three stages runs across the tap boundaries.  The steps, their order and the MFMAs are
// the same, so the bits are.
template <int KS, int NB, bool AFF, int D>
__global__ __launch_bounds__(256) void fan_conv_kernel(const ConvArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lp = lane & 15, lg = lane >> 4;
  const int m0 = blockIdx.x * kTilePx + wv * 32, nb0 = blockIdx.y * NB;
  const int HW = a.H * a.W;

  // the lane's two pixels (clamped into the batch: the tail's loads are in bounds, its results are not stored)
  int pb[2], py[2], px[2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const int m = min(m0 + mb * 16 + lp, a.M - 1);
    pb[mb] = m / HW;
    const int r = m - pb[mb] * HW;
    py[mb] = r / a.W;
    px[mb] = r - py[mb] * a.W;
  }

  f32x4 acc[2][NB];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const unsigned char* xb = reinterpret_cast<const unsigned char*>(a.x) + lg * 16;
  const unsigned char* wb = reinterpret_cast<const unsigned char*>(a.wimg) + (int64_t)nb0 * 1024 + lane * 16;
  const int64_t wstep = (int64_t)a.nbt * 1024;                // bytes of one K-step of all output channels
  const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  // the affine's coefficients of the lane's 8 channels of a step: 32 kc + 8 lg ..; without the affine the pointers are never read
  const float* pa = AFF ? a.ia + lg * 8 : nullptr;
  const float* pbf = AFF ? a.ib + lg * 8 : nullptr;

  if constexpr (D > 1) {
    const int S = KS * KS * a.nkc;
    half8 sx[D][2], sw[D][NB];
    float4 sc[D][4];
    bool sin[D][2];
    uint32_t off[2];
    bool in[2];
    int ltap = 0, lkc = 0;                                    // the step the next fetch belongs to (wave-uniform)
    auto set_tap = [&](int tap) {
      const int ky = tap / KS, kx = tap - ky * KS;
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
        const int iy = py[mb] - KS / 2 + ky, ix = px[mb] - KS / 2 + kx;
        in[mb] = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const int cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);
        off[mb] = (uint32_t)((((int64_t)pb[mb] * a.H + cy) * a.W + cx) * a.x_pitch * 2);
      }
    };
    set_tap(0);
#pragma unroll
    for (int d = 0; d < D; ++d) {                             // fill the ring
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) sx[d][mb] = *reinterpret_cast<const half8*>(xb + off[mb] + lkc * 64), sin[d][mb] = in[mb];
      const unsigned char* pw = wb + ((int64_t)ltap * a.nkc + lkc) * wstep;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) sw[d][nb] = *reinterpret_cast<const half8*>(pw + nb * 1024);
      if (AFF) {
        sc[d][0] = *reinterpret_cast<const float4*>(pa + lkc * 32), sc[d][1] = *reinterpret_cast<const float4*>(pa + lkc * 32 + 4);
        sc[d][2] = *reinterpret_cast<const float4*>(pbf + lkc * 32), sc[d][3] = *reinterpret_cast<const float4*>(pbf + lkc * 32 + 4);
      }
      // past the last step the last step is fetched again (in bounds) and never used: no branch around a load
      if (!(ltap == KS * KS - 1 && lkc == a.nkc - 1) && ++lkc == a.nkc) lkc = 0, set_tap(++ltap);
    }
    for (int s0 = 0; s0 < S; s0 += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        half8 pxc[2], wtc[NB];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
          const half8 v = AFF ? activate(sx[d][mb], sc[d][0], sc[d][1], sc[d][2], sc[d][3]) : sx[d][mb];
          pxc[mb] = sin[d][mb] ? v : zero;                    // the select stands behind the transform
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) wtc[nb] = sw[d][nb];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) sx[d][mb] = *reinterpret_cast<const half8*>(xb + off[mb] + lkc * 64), sin[d][mb] = in[mb];
        const unsigned char* pw = wb + ((int64_t)ltap * a.nkc + lkc) * wstep;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) sw[d][nb] = *reinterpret_cast<const half8*>(pw + nb * 1024);
        if (AFF) {
          sc[d][0] = *reinterpret_cast<const float4*>(pa + lkc * 32), sc[d][1] = *reinterpret_cast<const float4*>(pa + lkc * 32 + 4);
          sc[d][2] = *reinterpret_cast<const float4*>(pbf + lkc * 32), sc[d][3] = *reinterpret_cast<const float4*>(pbf + lkc * 32 + 4);
        }
        if (!(ltap == KS * KS - 1 && lkc == a.nkc - 1) && ++lkc == a.nkc) lkc = 0, set_tap(++ltap);
        if (s0 + d < S) {                                     // wave-uniform: the ring's tail past the last step
#pragma unroll
          for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wtc[nb], pxc[mb], acc[mb][nb], 0, 0, 0);
        }
      }
    }
  } else
  for (int tap = 0; tap < KS * KS; ++tap) {
    const int ky = tap / KS, kx = tap - ky * KS;
    uint32_t off[2];
    bool in[2];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int iy = py[mb] - KS / 2 + ky, ix = px[mb] - KS / 2 + kx;
      in[mb] = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      const int cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);
      off[mb] = (uint32_t)((((int64_t)pb[mb] * a.H + cy) * a.W + cx) * a.x_pitch * 2);
    }
    const unsigned char* pw = wb + (int64_t)tap * a.nkc * wstep;
    half8 pxn[2], wtn[NB];
    float4 can[4];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) pxn[mb] = *reinterpret_cast<const half8*>(xb + off[mb]);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) wtn[nb] = *reinterpret_cast<const half8*>(pw + nb * 1024);
    if (AFF) {
      can[0] = *reinterpret_cast<const float4*>(pa), can[1] = *reinterpret_cast<const float4*>(pa + 4);
      can[2] = *reinterpret_cast<const float4*>(pbf), can[3] = *reinterpret_cast<const float4*>(pbf + 4);
    }
    for (int kc = 0; kc < a.nkc; ++kc) {
      half8 pxc[2], wtc[NB];
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) {
        const half8 v = AFF ? activate(pxn[mb], can[0], can[1], can[2], can[3]) : pxn[mb];
        pxc[mb] = in[mb] ? v : zero;                          // the select stands behind the transform
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) wtc[nb] = wtn[nb];
      const int kn = min(kc + 1, a.nkc - 1);                  // the last step fetches itself again: no branch around a load
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) pxn[mb] = *reinterpret_cast<const half8*>(xb + off[mb] + kn * 64);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) wtn[nb] = *reinterpret_cast<const half8*>(pw + kn * wstep + nb * 1024);
      if (AFF) {
        can[0] = *reinterpret_cast<const float4*>(pa + kn * 32), can[1] = *reinterpret_cast<const float4*>(pa + kn * 32 + 4);
        can[2] = *reinterpret_cast<const float4*>(pbf + kn * 32), can[3] = *reinterpret_cast<const float4*>(pbf + kn * 32 + 4);
      }
#pragma unroll
      for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wtc[nb], pxc[mb], acc[mb][nb], 0, 0, 0);
    }
  }

  // epilogue: the lane holds channels 16 (nb0 + nb) + 4 lg + r, r = 0 .. 3, of its pixel of block mb.  A group of four past `cout`
  // (the padding of 68 to 96) reads the last real group and is not stored.
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const bool inside = m0 + mb * 16 + lp < a.M;
    const int64_t p = ((int64_t)pb[mb] * a.H + py[mb]) * a.W + px[mb];
    const int64_t pu = ((int64_t)pb[mb] * (a.H >> 1) + (py[mb] >> 1)) * (a.W >> 1) + (px[mb] >> 1);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int ch0 = (nb0 + nb) * 16 + lg * 4;
      const bool real = ch0 < a.cout;
      const int ch = min(ch0, a.cout - 4);
      float v[4] = {acc[mb][nb][0], acc[mb][nb][1], acc[mb][nb][2], acc[mb][nb][3]};
      if (a.bias) {
        const float4 b4 = *reinterpret_cast<const float4*>(a.bias + ch);
        v[0] += b4.x, v[1] += b4.y, v[2] += b4.z, v[3] += b4.w;
      }
      if (a.relu) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      if (a.raw) {
        half4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (_Float16)v[r];
        if (inside && real) *reinterpret_cast<half4*>(a.raw + p * a.raw_pitch + ch) = o;
      }
      if (a.res1) {
        const half4 q = *reinterpret_cast<const half4*>(a.res1 + p * a.res1_pitch + ch);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)q[r];
      }
      if (a.res2) {
        const half4 q = *reinterpret_cast<const half4*>(a.res2 + p * a.res2_pitch + ch);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)q[r];
      }
      if (a.up) {
        const half4 q = *reinterpret_cast<const half4*>(a.up + pu * a.up_pitch + ch);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (float)q[r];
      }
      if (a.y_f32) {
        if (inside && real) *reinterpret_cast<float4*>(static_cast<float*>(a.y) + p * a.y_pitch + ch) = float4{v[0], v[1], v[2], v[3]};
      } else {
        half4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (_Float16)v[r];
        if (inside && real) *reinterpret_cast<half4*>(static_cast<_Float16*>(a.y) + p * a.y_pitch + ch) = o;
      }
    }
  }
}

template <int KS, bool AFF, int D>
void launch_conv_depth(const ConvArgs& a, hipStream_t s) {
  const unsigned tiles = (unsigned)((a.M + kTilePx - 1) / kTilePx);
  if (a.nbt % 4 == 0)
    fan_conv_kernel<KS, 4, AFF, D><<<dim3(tiles, (unsigned)(a.nbt / 4)), 256, 0, s>>>(a);
  else
    fan_conv_kernel<KS, 2, AFF, D><<<dim3(tiles, (unsigned)(a.nbt / 2)), 256, 0, s>>>(a);
}

// A launch of at most two workgroups per compute unit (the chip has 256) leaves a wave alone on its SIMD: the deep ring.  The choice
// changes no bit.
template <int KS, bool AFF>
void launch_conv(const ConvArgs& a, hipStream_t s) {
  const int64_t groups = (int64_t)((a.M + kTilePx - 1) / kTilePx) * (a.nbt % 4 == 0 ? a.nbt / 4 : a.nbt / 2);
  if (groups <= kDeepGroups)
    launch_conv_depth<KS, AFF, 3>(a, s);
  else
    launch_conv_depth<KS, AFF, 1>(a, s);
}

// -------------------------------------------------------------------------------------------------------------------------- decode
// hm: (B, n, n, pitch) fp32, the landmark's map at channel k.  One wave per (landmark, image).  face_alignment's get_preds_fromhm and
// its inverse transform: x0 + (px + 0.5 +- 0.25) s / n, the sign that of hm[py][px + 1] - hm[py][px - 1]; no offset on the border or
// for a zero (or unordered) difference.  fp32, every operation rounded on its own.
__global__ __launch_bounds__(64) void fan_decode_kernel(float* __restrict__ lm, float* __restrict__ peak, int32_t* __restrict__ flag,
                                                        const float* __restrict__ hm, int pitch, const float* __restrict__ box, int n, int K) {
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const float* m = hm + (int64_t)b * n * n * pitch + k;
  const float ninf = -__builtin_inff();
  float best = ninf;
  int at = 0x7fffffff, bad = 0;
  for (int i = lane; i < n * n; i += 64) {
    float v = m[(int64_t)i * pitch];
    if (!(fabsf(v) <= 3.402823466e38f)) bad = 1, v = ninf;   // NaN and both infinities: flagged, never the peak
    if (v > best || (v == best && i < at)) best = v, at = i;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float ov = __shfl_xor(best, d);
    const int oi = __shfl_xor(at, d), ob = __shfl_xor(bad, d);
    if (ov > best || (ov == best && oi < at)) best = ov, at = oi;
    bad |= ob;
  }
  if (lane != 0) return;
  const int py = at / n, px = at - py * n;
  float dx = 0.f, dy = 0.f;
  if (px > 0 && px < n - 1) {
    const float d = __fsub_rn(m[(int64_t)(at + 1) * pitch], m[(int64_t)(at - 1) * pitch]);
    dx = d > 0.f ? 0.25f : (d < 0.f ? -0.25f : 0.f);
  }
  if (py > 0 && py < n - 1) {
    const float d = __fsub_rn(m[(int64_t)(at + n) * pitch], m[(int64_t)(at - n) * pitch]);
    dy = d > 0.f ? 0.25f : (d < 0.f ? -0.25f : 0.f);
  }
  const float x0 = box[3 * b], y0 = box[3 * b + 1], sc = __fdiv_rn(box[3 * b + 2], (float)n);
  const int64_t o = (int64_t)b * K + k;
  lm[2 * o] = __fadd_rn(x0, __fmul_rn(__fadd_rn(__fadd_rn((float)px, 0.5f), dx), sc));
  lm[2 * o + 1] = __fadd_rn(y0, __fmul_rn(__fadd_rn(__fadd_rn((float)py, 0.5f), dy), sc));
  peak[o] = best;
  flag[o] = bad;
}

inline bool dims_ok(int B, int H, int W) { return B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= kMaxSide && W <= kMaxSide; }
inline int64_t act_bytes(int B, int H, int W, int pitch, int elem = 2) { return (int64_t)B * H * W * pitch * elem; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool overlap(const void* p, int64_t pn, const void* q, int64_t qn) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}
inline bool window_ok(int off, int pitch, int n, int unit) { return off >= 0 && off % unit == 0 && pitch % unit == 0 && pitch >= 1 && pitch <= 4096 && off + n <= pitch; }

}  // namespace

extern "C" {

int vsp_fan_stem_u8(void* y, const uint8_t* src, const float* box, const float* w, const float* b, int B, int H, int W, int side,
                    vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, H, W), "fan_stem: batch %d, photo %d x %d (sides 1..%d)", B, H, W, kMaxSide);
  VSP_REQUIRE(side >= 8 && side <= 1024 && side % 8 == 0, "fan_stem: side %d (a multiple of 8 in 8..1024)", side);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(y && src && box && w && b, "fan_stem: null pointer");
  VSP_REQUIRE(aligned8(y) && vsp::aligned16(w) && vsp::aligned16(b) && (reinterpret_cast<uintptr_t>(box) & 3u) == 0,
              "fan_stem: buffers must be aligned (y to 8 bytes, weights to 16, boxes to 4)");
  if ((int64_t)B * H * W * 3 >= kTwoGiB || act_bytes(B, side / 2, side / 2, 64) >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "fan_stem: a buffer of 2 GiB or more");
  const int P = (side / 2) * (side / 2);
  fan_stem_kernel<<<dim3((P + 255) / 256, B), 256, 0, vsp::as_stream(stream)>>>(static_cast<_Float16*>(y), src, box, w, b, H, W, side);
  return vsp::check_launch("fan_stem");
}

int vsp_fan_pool_f16(void* y, int y_pitch, int y_off, const void* x, int x_pitch, int x_off, int B, int H, int W, int C, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, H, W), "fan_pool: batch %d, map %d x %d", B, H, W);
  VSP_REQUIRE(H % 2 == 0 && W % 2 == 0, "fan_pool: an odd map, %d x %d", H, W);
  VSP_REQUIRE(C >= 8 && C <= 256 && C % 8 == 0, "fan_pool: %d channels (a multiple of 8 up to 256)", C);
  VSP_REQUIRE(window_ok(x_off, x_pitch, C, 8), "fan_pool: input channels %d..%d of a pitch of %d (offset and pitch multiples of 8)", x_off,
              x_off + C - 1, x_pitch);
  VSP_REQUIRE(window_ok(y_off, y_pitch, C, 8), "fan_pool: output channels %d..%d of a pitch of %d (offset and pitch multiples of 8)", y_off,
              y_off + C - 1, y_pitch);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(y && x, "fan_pool: null pointer");
  VSP_REQUIRE(vsp::aligned16(y) && vsp::aligned16(x), "fan_pool: buffers must be 16-byte aligned");
  const int64_t xb = act_bytes(B, H, W, x_pitch), yb = act_bytes(B, H / 2, W / 2, y_pitch);
  if (xb >= kTwoGiB || yb >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "fan_pool: a tensor of 2 GiB or more");
  VSP_REQUIRE(!overlap(y, yb, x, xb), "fan_pool: the output overlaps the input");
  const int64_t n = (int64_t)B * (H / 2) * (W / 2) * (C / 8);
  fan_pool_kernel<<<(unsigned)((n + 255) / 256), 256, 0, vsp::as_stream(stream)>>>(static_cast<_Float16*>(y) + y_off, y_pitch,
                                                                                    static_cast<const _Float16*>(x) + x_off, x_pitch, n, C / 8, H, W);
  return vsp::check_launch("fan_pool");
}

int vsp_fan_conv_f16(void* y, int y_pitch, int y_off, void* raw, int raw_pitch, int raw_off, const void* x, int x_pitch, int x_off, int B, int H,
                     int W, int Cin, int Cout, int ksize, int flags, const void* w_img, const float* b, const float* in_a, const float* in_b,
                     const void* res1, int res1_pitch, int res1_off, const void* res2, int res2_pitch, int res2_off, const void* up, int up_pitch,
                     int up_off, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, H, W), "fan_conv: batch %d, map %d x %d", B, H, W);
  VSP_REQUIRE(Cin >= 32 && Cin <= 256 && Cin % 32 == 0, "fan_conv: %d input channels; multiples of 32 up to 256 are served (68 padded to 96)", Cin);
  VSP_REQUIRE((Cout >= 32 && Cout <= 256 && Cout % 32 == 0) || Cout == 68, "fan_conv: %d output channels; multiples of 32 up to 256 and 68 are served",
              Cout);
  VSP_REQUIRE(ksize == 1 || ksize == 3, "fan_conv: filter %d x %d (1 x 1 or 3 x 3)", ksize, ksize);
  VSP_REQUIRE((flags & ~(VSP_FAN_RELU | VSP_FAN_OUT_F32)) == 0, "fan_conv: unknown flags %d", flags);
  const int f32 = (flags & VSP_FAN_OUT_F32) != 0;
  VSP_REQUIRE(window_ok(x_off, x_pitch, Cin, 8), "fan_conv: input channels %d..%d of a pitch of %d (offset and pitch multiples of 8)", x_off,
              x_off + Cin - 1, x_pitch);
  VSP_REQUIRE(window_ok(y_off, y_pitch, Cout, 4), "fan_conv: output channels %d..%d of a pitch of %d (offset and pitch multiples of 4)", y_off,
              y_off + Cout - 1, y_pitch);
  VSP_REQUIRE(!raw || window_ok(raw_off, raw_pitch, Cout, 4), "fan_conv: raw channels %d..%d of a pitch of %d (offset and pitch multiples of 4)", raw_off,
              raw_off + Cout - 1, raw_pitch);
  VSP_REQUIRE(!res1 || window_ok(res1_off, res1_pitch, Cout, 4), "fan_conv: residual channels %d..%d of a pitch of %d (offset and pitch multiples of 4)",
              res1_off, res1_off + Cout - 1, res1_pitch);
  VSP_REQUIRE(!res2 || window_ok(res2_off, res2_pitch, Cout, 4), "fan_conv: second residual channels %d..%d of a pitch of %d (offset and pitch multiples of 4)",
              res2_off, res2_off + Cout - 1, res2_pitch);
  VSP_REQUIRE(!up || window_ok(up_off, up_pitch, Cout, 4), "fan_conv: coarser-level channels %d..%d of a pitch of %d (offset and pitch multiples of 4)",
              up_off, up_off + Cout - 1, up_pitch);
  VSP_REQUIRE(!res2 || res1, "fan_conv: a second residual without a first");
  VSP_REQUIRE((in_a == nullptr) == (in_b == nullptr), "fan_conv: the input affine needs both a and b");
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(y && x && w_img, "fan_conv: null pointer");
  VSP_REQUIRE(vsp::aligned16(x) && vsp::aligned16(w_img) && vsp::aligned16(b) && vsp::aligned16(in_a) && vsp::aligned16(in_b) &&
                  (f32 ? vsp::aligned16(y) : aligned8(y)) && aligned8(raw) && aligned8(res1) && aligned8(res2) && aligned8(up),
              "fan_conv: buffers must be aligned (input, weights, bias, affine and an fp32 output to 16 bytes; f16 outputs and residuals to 8)");
  VSP_REQUIRE(!up || (H % 2 == 0 && W % 2 == 0), "fan_conv: the coarser level needs an even map, not %d x %d", H, W);
  const int64_t xb = act_bytes(B, H, W, x_pitch), yb = act_bytes(B, H, W, y_pitch, f32 ? 4 : 2), wb = raw ? act_bytes(B, H, W, raw_pitch) : 0;
  const int64_t r1 = res1 ? act_bytes(B, H, W, res1_pitch) : 0, r2 = res2 ? act_bytes(B, H, W, res2_pitch) : 0;
  const int64_t ub = up ? act_bytes(B, H / 2, W / 2, up_pitch) : 0;
  if (xb >= kTwoGiB || yb >= kTwoGiB || wb >= kTwoGiB || r1 >= kTwoGiB || r2 >= kTwoGiB || ub >= kTwoGiB)
    return vsp::fail(VSP_ENOTSUP, "fan_conv: a tensor of 2 GiB or more");
  VSP_REQUIRE(!overlap(y, yb, x, xb) && !(raw && overlap(raw, wb, x, xb)), "fan_conv: an output overlaps the input");
  VSP_REQUIRE(!raw || !overlap(raw, wb, y, yb), "fan_conv: the raw output overlaps the output");
  // a residual may be the very window the launch writes (each value is read by the lane that then writes it) and nothing else of it
  const void* rs[2] = {res1, res2};
  const int64_t rn[2] = {r1, r2};
  const int rp[2] = {res1_pitch, res2_pitch}, ro[2] = {res1_off, res2_off};
  for (int i = 0; i < 2; ++i) {
    if (!rs[i]) continue;
    if (overlap(y, yb, rs[i], rn[i]))
      VSP_REQUIRE(!f32 && rs[i] == y && rp[i] == y_pitch && ro[i] == y_off, "fan_conv: a residual overlaps the output without being its window");
    VSP_REQUIRE(!raw || !overlap(raw, wb, rs[i], rn[i]), "fan_conv: a residual overlaps the raw output");
  }
  VSP_REQUIRE(!up || (!overlap(y, yb, up, ub) && !(raw && overlap(raw, wb, up, ub))), "fan_conv: the coarser level overlaps an output");
  ConvArgs a = {};
  a.y = f32 ? static_cast<void*>(static_cast<float*>(y) + y_off) : static_cast<void*>(static_cast<_Float16*>(y) + y_off);
  a.raw = raw ? static_cast<_Float16*>(raw) + raw_off : nullptr;
  a.x = static_cast<const _Float16*>(x) + x_off;
  a.res1 = res1 ? static_cast<const _Float16*>(res1) + res1_off : nullptr, a.res2 = res2 ? static_cast<const _Float16*>(res2) + res2_off : nullptr;
  a.up = up ? static_cast<const _Float16*>(up) + up_off : nullptr;
  a.wimg = static_cast<const uint4*>(w_img), a.bias = b, a.ia = in_a, a.ib = in_b;
  a.y_pitch = y_pitch, a.raw_pitch = raw_pitch, a.x_pitch = x_pitch, a.res1_pitch = res1_pitch, a.res2_pitch = res2_pitch, a.up_pitch = up_pitch;
  a.H = H, a.W = W, a.M = B * H * W, a.nkc = Cin / 32, a.nbt = ((Cout + 31) / 32) * 2, a.cout = Cout;
  a.relu = (flags & VSP_FAN_RELU) != 0, a.y_f32 = f32;
  hipStream_t s = vsp::as_stream(stream);
  if (ksize == 1) {
    if (in_a) launch_conv<1, true>(a, s);
    else launch_conv<1, false>(a, s);
  } else {
    if (in_a) launch_conv<3, true>(a, s);
    else launch_conv<3, false>(a, s);
  }
  return vsp::check_launch("fan_conv");
}

int vsp_fan_decode_f32(float* lm, float* peak, int32_t* flag, const float* hm, int pitch, const float* box, int B, int n, int K, vsp_stream_t stream) {
  VSP_REQUIRE(B >= 0 && B <= 65535 && n >= 1 && n <= 1024, "fan_decode: batch %d, map %d x %d", B, n, n);
  VSP_REQUIRE(K >= 1 && K <= 4096 && pitch >= K && pitch <= 4096, "fan_decode: %d landmarks in a pitch of %d", K, pitch);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(lm && peak && flag && hm && box, "fan_decode: null pointer");
  VSP_REQUIRE(((reinterpret_cast<uintptr_t>(lm) | reinterpret_cast<uintptr_t>(peak) | reinterpret_cast<uintptr_t>(flag) | reinterpret_cast<uintptr_t>(hm) |
                reinterpret_cast<uintptr_t>(box)) & 3u) == 0, "fan_decode: buffers must be 4-byte aligned");
  if (act_bytes(B, n, n, pitch, 4) >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "fan_decode: a tensor of 2 GiB or more");
  fan_decode_kernel<<<dim3(K, B), 64, 0, vsp::as_stream(stream)>>>(lm, peak, flag, hm, pitch, box, n, K);
  return vsp::check_launch("fan_decode");
}

}  // extern "C"

// FID on the device: pytorch-fid's Inception-v3 in fp32.  Activations are (B, H, W, pitch) float, the images of a call back to
// back; a tensor is addressed by (pointer, channel pitch), so a branch of an Inception block writes its slice of the concatenated tensor.
//   fid_stem_kernel   u8 RGB images of any size -> bilinear resize (align_corners = false, no anti-aliasing) -> x / 127.5 - 1 ->
//                     Conv2d_1a 3 -> 32, 3x3 stride 2, + bias, ReLU.  K = 27 is fmaf work.  ONE kernel: the resized image would be a
//                     299 x 299 x 3 fp32 round trip per image, and recomputing a resized pixel for each of the (9 / 4 on average)
//                     outputs that read it costs four byte loads and six flops beside the 64 fmaf it feeds.
//   fid_conv_kernel   the other 93 layers: one implicit GEMM on v_mfma_f32_16x16x4_f32 for every filter (1x1, 3x3, 5x5, 1x7, 7x1, 1x3,
//                     3x1), any padding below the filter extent, stride 1 / 2, Cin and Cout multiples of 16, + bias, ReLU in fp32
//   fid_pool_kernel   max 3x3 / 2, average 3x3 / 1 / pad 1 over the in-bounds taps, max 3x3 / 1 / pad 1, and the global average
//
// fid_conv_kernel.  16x16x4 and not 32x32x2: both reach the same 64 FLOP / clk / SIMD, but the 16x16 form needs 4 accumulator
// registers per tile instead of 16, issues every 32 cycles with a dependent latency of 40, so the 4 independent accumulators a wave
// holds here already keep the pipe full, and a 16-channel granule is what Cout = 48, 80, 176 ... asks for.  256 threads; a workgroup
// owns 64 output pixels -- a FLAT index over batch, rows and columns, so odd maps (147, 73, 71, 35, 17) leave one ragged tile per call
// and not one per row -- and up to 64 output channels.  Wave v owns pixel blocks 2 (v & 1) + {0, 1} and channel blocks 2 (v >> 1) +
// {0, 1} of 16.  K = KH KW Cin is walked tap by tap in chunks of 16 input channels: 64 pixels x 16 channels of input (row stride 20
// floats) and 16 x 64 weights (row stride 80 floats) go to LDS, one float4 of each per thread, fetched into registers while the previous
// chunk is multiplied.  A tap outside the map is resolved by a clamped address and a select, never by a branch.  As in parse.hip the
// WEIGHTS are the MFMA's A operand and the pixels its B operand: a lane ends with four consecutive channels of one pixel and stores 16
// bytes.  K runs up to 11 200 (a 5x5 on 448 channels) and a single fmaf chain of that length carries about sqrt(K / 3) eps of rounding
// noise, so the sum is kept in two levels: segments of 8 chunks (128 products) are fmaf chains in the MFMA accumulator, and the
// segments are added in order in registers (about 8 eps within a segment plus sqrt(K / 384) eps across them).  The order of an output's
// sum depends on nothing but k (tap-major, then channel), so an image has the same bits at any batch size and position.
#include "vsp_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int64_t kTwoGiB = (int64_t)1 << 31;
constexpr int kXS = 20;                                       // floats per pixel of the LDS input chunk (16 + 4: conflict-free fragment reads)
constexpr int kWS = 80;                                       // floats per k row of the LDS weight chunk (64 + 16)
constexpr int kSeg = 8;                                       // chunks (128 products) per summation segment

// ---------------------------------------------------------------------------------------------------------------------------- stem
__global__ __launch_bounds__(256) void fid_stem_kernel(float* __restrict__ y, const uint8_t* __restrict__ src,
                                                       const vsp_det_src* __restrict__ items, const float* __restrict__ w,
                                                       const float* __restrict__ bias, int TH, int TW, int OH, int OW) {
  __shared__ __attribute__((aligned(16))) float sw[27 * 32];
  __shared__ __attribute__((aligned(16))) float sb[32];
  for (int i = threadIdx.x; i < 27 * 32; i += 256) sw[i] = w[i];
  if (threadIdx.x < 32) sb[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const vsp_det_src it = items[blockIdx.y];
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= OH * OW) return;
  const int oy = q / OW, ox = q - oy * OW;
  const uint8_t* img = src + it.off;
  float acc[32];
#pragma unroll
  for (int co = 0; co < 32; ++co) acc[co] = sb[co];
  // source position of target index t: ((2 t + 1) n_in - n_out) / (2 n_out), clamped at 0 -- the exact rational form of
  // (t + 0.5) n_in / n_out - 0.5; the weight is one division, and an equal size gives weight 0 exactly
  const int64_t dy2 = 2 * (int64_t)TH, dx2 = 2 * (int64_t)TW;
  for (int ky = 0; ky < 3; ++ky) {
    const int64_t ny = max((int64_t)(2 * (2 * oy + ky) + 1) * it.h - TH, (int64_t)0);
    const int y0 = (int)(ny / dy2), y1 = min(y0 + 1, it.h - 1);
    const float ly = (float)(ny - y0 * dy2) / (float)dy2;
    for (int kx = 0; kx < 3; ++kx) {
      const int64_t nx = max((int64_t)(2 * (2 * ox + kx) + 1) * it.w - TW, (int64_t)0);
      const int x0 = (int)(nx / dx2), x1 = min(x0 + 1, it.w - 1);
      const float lx = (float)(nx - x0 * dx2) / (float)dx2;
      const uint8_t* p00 = img + ((int64_t)y0 * it.w + x0) * 3;
      const uint8_t* p01 = img + ((int64_t)y0 * it.w + x1) * 3;
      const uint8_t* p10 = img + ((int64_t)y1 * it.w + x0) * 3;
      const uint8_t* p11 = img + ((int64_t)y1 * it.w + x1) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float top = (1.f - lx) * (float)p00[c] + lx * (float)p01[c];
        const float bot = (1.f - lx) * (float)p10[c] + lx * (float)p11[c];
        const float v = ((1.f - ly) * top + ly * bot) / 127.5f - 1.f;
        const float4* wr = reinterpret_cast<const float4*>(sw + ((ky * 3 + kx) * 3 + c) * 32);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
          const float4 w4 = wr[g];
          acc[4 * g] = fmaf(w4.x, v, acc[4 * g]);
          acc[4 * g + 1] = fmaf(w4.y, v, acc[4 * g + 1]);
          acc[4 * g + 2] = fmaf(w4.z, v, acc[4 * g + 2]);
          acc[4 * g + 3] = fmaf(w4.w, v, acc[4 * g + 3]);
        }
      }
    }
  }
  float4* yo = reinterpret_cast<float4*>(y + ((int64_t)it.slot * OH * OW + q) * 32);
#pragma unroll
  for (int g = 0; g < 8; ++g)
    yo[g] = make_float4(fmaxf(acc[4 * g], 0.f), fmaxf(acc[4 * g + 1], 0.f), fmaxf(acc[4 * g + 2], 0.f), fmaxf(acc[4 * g + 3], 0.f));
}

// --------------------------------------------------------------------------------------------------------------------- convolution
struct ConvArgs {
  float* y;
  const float* x;
  const float* w;
  const float* bias;
  int H, W, OH, OW, Cin, Cout, KH, KW, ph, pw, stride, x_pitch, c_off, c_pitch;
  int P;              // B OH OW
  int ncb;            // ceil(Cout / 64)
};

__global__ __launch_bounds__(256) void fid_conv_kernel(const ConvArgs a) {
  __shared__ __attribute__((aligned(16))) float s_x[64 * kXS];
  __shared__ __attribute__((aligned(16))) float s_w[16 * kWS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lp = lane & 15, lg = lane >> 4;
  const int tile = blockIdx.x / a.ncb, cb = blockIdx.x - tile * a.ncb;

  // staging: thread -> four channels of one pixel of the input chunk, and four output channels of one k row of the weight chunk
  const int spx = tid >> 2, sc4 = (tid & 3) * 4;
  const int pq = tile * 64 + spx;
  const bool pv = pq < a.P;
  const int p = min(pq, a.P - 1);
  const int b = p / (a.OH * a.OW), rem = p - b * (a.OH * a.OW), oy = rem / a.OW, ox = rem - oy * a.OW;
  const int iy0 = oy * a.stride - a.ph, ix0 = ox * a.stride - a.pw;
  const float* xb = a.x + (int64_t)b * a.H * a.W * a.x_pitch + sc4;
  const int wk = tid >> 4, wc4 = (tid & 15) * 4;
  const bool wok = cb * 64 + wc4 < a.Cout;
  const float* wb = a.w + (int64_t)wk * a.Cout + (wok ? cb * 64 + wc4 : 0);
  const int ncc = a.Cin >> 4, nchunks = a.KH * a.KW * ncc;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);

  auto fetch = [&](int ky, int kx, int cc, float4& vx, float4& vw) {
    const int iy = iy0 + ky, ix = ix0 + kx;
    const bool ok = pv && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    const int cy = min(max(iy, 0), a.H - 1), cx = min(max(ix, 0), a.W - 1);
    const float4 v = *reinterpret_cast<const float4*>(xb + ((int64_t)cy * a.W + cx) * a.x_pitch + cc * 16);
    vx = ok ? v : zero;
    const float4 u = *reinterpret_cast<const float4*>(wb + (int64_t)((ky * a.KW + kx) * a.Cin + cc * 16) * a.Cout);
    vw = wok ? u : zero;
  };

  const int pb0 = 2 * (wv & 1), nb0 = 2 * (wv >> 1);
  const bool use0 = (cb * 4 + nb0) * 16 < a.Cout, use1 = (cb * 4 + nb0 + 1) * 16 < a.Cout;     // wave-uniform
  f32x4 acc[2][2], tot[2][2];                                // acc: the running segment of kSeg chunks; tot: the segments added in order
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  float4 vx, vw;
  int ky = 0, kx = 0, cc = 0;
  fetch(0, 0, 0, vx, vw);
  for (int c = 0; c < nchunks; ++c) {
    if (c) __syncthreads();                                   // the previous chunk's fragment reads are done
    *reinterpret_cast<float4*>(s_x + spx * kXS + sc4) = vx;
    *reinterpret_cast<float4*>(s_w + wk * kWS + wc4) = vw;
    __syncthreads();
    if (++cc == ncc) {
      cc = 0;
      if (++kx == a.KW) kx = 0, ++ky;
    }
    if (c + 1 < nchunks) fetch(ky, kx, cc, vx, vw);           // in flight while this chunk is multiplied
    if (use0) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const float px0 = s_x[(pb0 * 16 + lp) * kXS + 4 * ks + lg], px1 = s_x[((pb0 + 1) * 16 + lp) * kXS + 4 * ks + lg];
        const float wt0 = s_w[(4 * ks + lg) * kWS + nb0 * 16 + lp];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt0, px0, acc[0][0], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt0, px1, acc[1][0], 0, 0, 0);
        if (use1) {
          const float wt1 = s_w[(4 * ks + lg) * kWS + (nb0 + 1) * 16 + lp];
          acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt1, px0, acc[0][1], 0, 0, 0);
          acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt1, px1, acc[1][1], 0, 0, 0);
        }
      }
    }
    if ((c & (kSeg - 1)) == kSeg - 1 || c + 1 == nchunks) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) tot[i][j] += acc[i][j], acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }

  // epilogue: the lane holds channels 4 lg + r, r = 0 .. 3, of channel block j for pixel lp of pixel block i
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int q = tile * 64 + (pb0 + i) * 16 + lp;
    if (q >= a.P) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ch = (cb * 4 + nb0 + j) * 16 + 4 * lg;
      if (ch >= a.Cout) continue;
      const float4 b4 = *reinterpret_cast<const float4*>(a.bias + ch);
      const float4 o = make_float4(fmaxf(tot[i][j][0] + b4.x, 0.f), fmaxf(tot[i][j][1] + b4.y, 0.f), fmaxf(tot[i][j][2] + b4.z, 0.f),
                                   fmaxf(tot[i][j][3] + b4.w, 0.f));
      *reinterpret_cast<float4*>(a.y + (int64_t)q * a.c_pitch + a.c_off + ch) = o;
    }
  }
}

// --------------------------------------------------------------------------------------------------------------------------- pools
// one thread per output pixel and four channels; MODE: VSP_FID_POOL_*
template <int MODE>
__global__ __launch_bounds__(256) void fid_pool_kernel(float* __restrict__ y, const float* __restrict__ x, int H, int W, int OH, int OW,
                                                       int C4, int x_pitch, int c_off, int c_pitch, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4) * 4;
  const int64_t q = i / C4;                                   // flat output pixel
  const int ox = (int)(q % OW), oy = (int)((q / OW) % OH);
  const int64_t b = q / ((int64_t)OW * OH);
  constexpr int ST = MODE == VSP_FID_POOL_MAX_S2 ? 2 : 1, PAD = MODE == VSP_FID_POOL_MAX_S2 ? 0 : 1;
  constexpr bool AVG = MODE == VSP_FID_POOL_AVG_S1;
  const float init = AVG ? 0.f : -INFINITY;
  float4 r = make_float4(init, init, init, init);
  int count = 0;
  const float* xb = x + b * H * W * x_pitch + c;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = oy * ST - PAD + ky, ix = ox * ST - PAD + kx;
      const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
      const float4 v = *reinterpret_cast<const float4*>(xb + ((int64_t)cy * W + cx) * x_pitch);
      count += ok ? 1 : 0;
      if (AVG) {
        r.x += ok ? v.x : 0.f, r.y += ok ? v.y : 0.f, r.z += ok ? v.z : 0.f, r.w += ok ? v.w : 0.f;
      } else {
        r.x = fmaxf(r.x, ok ? v.x : init), r.y = fmaxf(r.y, ok ? v.y : init), r.z = fmaxf(r.z, ok ? v.z : init),
        r.w = fmaxf(r.w, ok ? v.w : init);
      }
    }
  if (AVG) {
    const float n = (float)count;
    r = make_float4(r.x / n, r.y / n, r.z / n, r.w / n);
  }
  *reinterpret_cast<float4*>(y + q * c_pitch + c_off + c) = r;
}

// global average: one thread per image and four channels adds the H W pixels in row-major order
__global__ __launch_bounds__(256) void fid_gap_kernel(float* __restrict__ y, const float* __restrict__ x, int HW, int C4, int x_pitch,
                                                      int c_off, int c_pitch, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4) * 4;
  const int64_t b = i / C4;
  const float* xb = x + b * HW * x_pitch + c;
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = 0; p < HW; ++p) {
    const float4 v = *reinterpret_cast<const float4*>(xb + (int64_t)p * x_pitch);
    r.x += v.x, r.y += v.y, r.z += v.z, r.w += v.w;
  }
  const float n = (float)HW;
  *reinterpret_cast<float4*>(y + b * c_pitch + c_off + c) = make_float4(r.x / n, r.y / n, r.z / n, r.w / n);
}

// bytes from the first to one past the last element of a (pixels, pitch) tensor of which `ch` channels are touched
int64_t span_bytes(int64_t pixels, int pitch, int ch) { return ((pixels - 1) * pitch + ch) * 4; }

bool overlap(const void* p, int64_t pn, const void* q, int64_t qn) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}

bool filter_ok(int kh, int kw) {
  return (kh == 1 && kw == 1) || (kh == 3 && kw == 3) || (kh == 5 && kw == 5) || (kh == 1 && kw == 7) || (kh == 7 && kw == 1) ||
         (kh == 1 && kw == 3) || (kh == 3 && kw == 1);
}

}  // namespace

extern "C" {

int vsp_fid_stem_u8(float* y, const uint8_t* src, size_t src_bytes, const vsp_det_src* items, const vsp_det_src* items_dev, int n, int B,
                    int TH, int TW, const float* w, const float* b, vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && B >= 0 && n <= B, "fid_stem: %d items for a batch of %d", n, B);
  VSP_REQUIRE(TH >= 3 && TW >= 3 && TH <= 32768 && TW <= 32768, "fid_stem: target %d x %d (3..32768: the 3x3 stride-2 output must not be empty)",
              TH, TW);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(y && src && items && items_dev && w && b, "fid_stem: null pointer");
  VSP_REQUIRE(vsp::aligned16(y) && vsp::aligned16(w) && vsp::aligned16(b) && vsp::aligned16(items_dev), "fid_stem: buffers must be 16-byte aligned");
  const int OH = (TH - 3) / 2 + 1, OW = (TW - 3) / 2 + 1;
  if ((int64_t)src_bytes >= kTwoGiB || (int64_t)B * OH * OW * 128 >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "fid_stem: a tensor of 2 GiB or more");
  for (int i = 0; i < n; ++i) {
    const vsp_det_src& it = items[i];
    VSP_REQUIRE(it.h >= 1 && it.w >= 1 && it.h <= 32768 && it.w <= 32768, "fid_stem: item %d: image %d x %d (sides 1..32768)", i, it.h, it.w);
    VSP_REQUIRE(it.off >= 0 && it.off + (int64_t)3 * it.h * it.w <= (int64_t)src_bytes, "fid_stem: item %d: bytes outside src", i);
    VSP_REQUIRE(it.slot >= 0 && it.slot < B, "fid_stem: item %d: slot %d outside 0..%d", i, it.slot, B - 1);
  }
  VSP_REQUIRE(!overlap(y, (int64_t)B * OH * OW * 128, src, (int64_t)src_bytes), "fid_stem: the output overlaps the input");
  fid_stem_kernel<<<dim3((OH * OW + 255) / 256, n), 256, 0, vsp::as_stream(stream)>>>(y, src, items_dev, w, b, TH, TW, OH, OW);
  return vsp::check_launch("fid_stem");
}

int vsp_fid_conv_f32(float* out, const float* x, const float* w, const float* bias, int B, int H, int W, int Cin, int x_pitch, int Cout,
                     int KH, int KW, int ph, int pw, int stride, int c_off, int c_pitch, vsp_stream_t stream) {
  VSP_REQUIRE(B >= 0, "fid_conv: %d images", B);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(out && x && w && bias, "fid_conv: null pointer");
  VSP_REQUIRE(Cin >= 16 && Cin % 16 == 0 && Cout >= 16 && Cout % 16 == 0, "fid_conv: %d -> %d channels, multiples of 16 are served", Cin, Cout);
  VSP_REQUIRE(filter_ok(KH, KW), "fid_conv: filter %d x %d (1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1)", KH, KW);
  VSP_REQUIRE(stride == 1 || stride == 2, "fid_conv: stride %d (1 or 2)", stride);
  VSP_REQUIRE(ph >= 0 && ph < KH && pw >= 0 && pw < KW, "fid_conv: padding %d x %d of a %d x %d filter", ph, pw, KH, KW);
  VSP_REQUIRE(H >= 1 && W >= 1 && H < (1 << 20) && W < (1 << 20), "fid_conv: map %d x %d", H, W);
  VSP_REQUIRE(H + 2 * ph >= KH && W + 2 * pw >= KW, "fid_conv: a %d x %d map under a %d x %d filter with padding %d x %d: the output is empty", H, W,
              KH, KW, ph, pw);
  VSP_REQUIRE(x_pitch >= Cin && x_pitch % 4 == 0, "fid_conv: input pitch %d for %d channels (at least Cin, a multiple of 4)", x_pitch, Cin);
  VSP_REQUIRE(c_off >= 0 && c_off % 4 == 0 && c_pitch % 4 == 0 && (int64_t)c_pitch >= (int64_t)c_off + Cout,
              "fid_conv: output pitch %d < offset %d + %d channels (or off a multiple of 4)", c_pitch, c_off, Cout);
  VSP_REQUIRE(vsp::aligned16(out) && vsp::aligned16(x) && vsp::aligned16(w) && vsp::aligned16(bias), "fid_conv: buffers must be 16-byte aligned");
  const int OH = (H + 2 * ph - KH) / stride + 1, OW = (W + 2 * pw - KW) / stride + 1;
  const int64_t xpix = (int64_t)B * H * W, ypix = (int64_t)B * OH * OW;
  if (xpix * x_pitch * 4 >= kTwoGiB || ypix * c_pitch * 4 >= kTwoGiB || (int64_t)KH * KW * Cin * Cout * 4 >= kTwoGiB)
    return vsp::fail(VSP_ENOTSUP, "fid_conv: a tensor of 2 GiB or more");
  VSP_REQUIRE(!overlap(out + c_off, span_bytes(ypix, c_pitch, Cout), x, span_bytes(xpix, x_pitch, Cin)), "fid_conv: the output overlaps the input");
  ConvArgs a = {};
  a.y = out, a.x = x, a.w = w, a.bias = bias;
  a.H = H, a.W = W, a.OH = OH, a.OW = OW, a.Cin = Cin, a.Cout = Cout, a.KH = KH, a.KW = KW, a.ph = ph, a.pw = pw, a.stride = stride;
  a.x_pitch = x_pitch, a.c_off = c_off, a.c_pitch = c_pitch;
  a.P = (int)ypix, a.ncb = (Cout + 63) / 64;
  const int64_t grid = ((ypix + 63) / 64) * a.ncb;
  fid_conv_kernel<<<(unsigned)grid, 256, 0, vsp::as_stream(stream)>>>(a);
  return vsp::check_launch("fid_conv");
}

int vsp_fid_pool_f32(float* out, const float* x, int B, int H, int W, int C, int x_pitch, int mode, int c_off, int c_pitch,
                     vsp_stream_t stream) {
  VSP_REQUIRE(B >= 0, "fid_pool: %d images", B);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(out && x, "fid_pool: null pointer");
  VSP_REQUIRE(mode >= VSP_FID_POOL_MAX_S2 && mode <= VSP_FID_POOL_GLOBAL_AVG, "fid_pool: mode %d", mode);
  VSP_REQUIRE(C >= 16 && C % 16 == 0, "fid_pool: %d channels, multiples of 16 are served", C);
  VSP_REQUIRE(H >= 1 && W >= 1 && H < (1 << 20) && W < (1 << 20), "fid_pool: map %d x %d", H, W);
  VSP_REQUIRE(mode != VSP_FID_POOL_MAX_S2 || (H >= 3 && W >= 3), "fid_pool: a %d x %d map under 3x3 / 2 without padding: the output is empty", H, W);
  VSP_REQUIRE(x_pitch >= C && x_pitch % 4 == 0, "fid_pool: input pitch %d for %d channels (at least C, a multiple of 4)", x_pitch, C);
  VSP_REQUIRE(c_off >= 0 && c_off % 4 == 0 && c_pitch % 4 == 0 && (int64_t)c_pitch >= (int64_t)c_off + C,
              "fid_pool: output pitch %d < offset %d + %d channels (or off a multiple of 4)", c_pitch, c_off, C);
  VSP_REQUIRE(vsp::aligned16(out) && vsp::aligned16(x), "fid_pool: buffers must be 16-byte aligned");
  int OH = H, OW = W;
  if (mode == VSP_FID_POOL_MAX_S2) OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
  if (mode == VSP_FID_POOL_GLOBAL_AVG) OH = OW = 1;
  const int64_t xpix = (int64_t)B * H * W, ypix = (int64_t)B * OH * OW;
  if (xpix * x_pitch * 4 >= kTwoGiB || ypix * c_pitch * 4 >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "fid_pool: a tensor of 2 GiB or more");
  VSP_REQUIRE(!overlap(out + c_off, span_bytes(ypix, c_pitch, C), x, span_bytes(xpix, x_pitch, C)), "fid_pool: the output overlaps the input");
  const int64_t total = ypix * (C / 4);
  const unsigned grid = (unsigned)((total + 255) / 256);
  hipStream_t s = vsp::as_stream(stream);
  if (mode == VSP_FID_POOL_MAX_S2)
    fid_pool_kernel<VSP_FID_POOL_MAX_S2><<<grid, 256, 0, s>>>(out, x, H, W, OH, OW, C / 4, x_pitch, c_off, c_pitch, total);
  else if (mode == VSP_FID_POOL_AVG_S1)
    fid_pool_kernel<VSP_FID_POOL_AVG_S1><<<grid, 256, 0, s>>>(out, x, H, W, OH, OW, C / 4, x_pitch, c_off, c_pitch, total);
  else if (mode == VSP_FID_POOL_MAX_S1)
    fid_pool_kernel<VSP_FID_POOL_MAX_S1><<<grid, 256, 0, s>>>(out, x, H, W, OH, OW, C / 4, x_pitch, c_off, c_pitch, total);
  else
    fid_gap_kernel<<<grid, 256, 0, s>>>(out, x, H * W, C / 4, x_pitch, c_off, c_pitch, total);
  return vsp::check_launch("fid_pool");
}

}  // extern "C"

// Background upscaling for whole photos: Real-ESRGAN's RRDBNet (x4plus, x2plus: 64 features, growth 32) on f16 operands.
//   rrdb_head_kernel<S>      conv_first on the u8 photo where it lies: x / 255, for x2plus the pixel unshuffle and the reflection of an odd
//                            last row / column as index arithmetic, 3 | 12 -> 64 3x3 (zero padding), + bias; fp32 fmaf, f16 NHWC out
//   rrdb_conv_kernel<NB, 0>  every 3x3 between head and tail as an implicit GEMM on v_mfma_f32_16x16x32_f16: Cin = 64 .. 192 in steps of 32,
//                            Cout = 16 NB = 32 | 64, optional nearest x2 of the input, + fp32 bias, LeakyReLU(0.2), up to two scaled
//                            residuals, one rounding to f16, written into a channel slice of the output tensor
//   rrdb_conv_kernel<1, 1>   conv_last: 64 -> 3 (padded to 16), clamp, rintf(255 v) as u8 into the packed output, non-finite flag
// Activations are (H, W, pitch) _Float16; a tensor is a pointer and a channel pitch, an output also a channel offset, so a dense block is
// one 192-channel tensor whose convolutions write the slices behind the channels they read.
//
// rrdb_conv_kernel: 256 threads, one workgroup per tile of 8 rows x 32 columns of output pixels and all output channels.  K = 9 Cin is
// walked in chunks of 32 input channels (one chunk = 9 K-steps, one per tap).  The chunk's input tile with its halo (10 x 34 pixels x 64 B)
// lies in LDS at an 80-byte pixel stride (20 dwords: the 16 pixels of a ds_read_b128 quarter fall on 16 disjoint bank quads); the next
// chunk's 1 360 16-byte pieces are fetched into registers before the MFMA loop of the current one and stored to LDS behind it.  Padding
// and the nearest x2 are resolved in the address (clamped, so every load is in bounds and unconditional) and a select.  The weights of a
// layer do not fit LDS beside a tile for the wide layers (192 -> 64: 216 KB), so every layer reads its fragments straight from the packed
// image in L2, 1 KiB of consecutive bytes per wave and MFMA operand, as parse.hip does.  Wave v owns rows 2 v and 2 v + 1 of the tile.
// The WEIGHTS are the MFMA's A operand and the pixels its B operand: a lane holds four consecutive output channels of one pixel
// (column = lane & 15 = pixel, row = 4 (lane >> 4) + r = channel of the block) and stores 8 bytes per block.
#include "vsp_common.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTH = 8, kTW = 32, kIH = kTH + 2, kIW = kTW + 2;
constexpr int kPixStride = 80;                                // bytes per pixel of the LDS tile (64 + 16 of padding)
constexpr int kPieces = kIH * kIW * 4;                        // 16-byte pieces of one chunk's tile: 1 360
constexpr int kLoads = (kPieces + 255) / 256;                 // per thread: 6
constexpr int64_t kTwoGiB = (int64_t)1 << 31;

// ---------------------------------------------------------------------------------------------------------------------------- head
// S = 4: the photo itself, 3 channels.  S = 2: pixel_unshuffle(2) of the photo padded by reflection to even sides, channel 4 c + 2 dy + dx.
// w: (27 | 108, 64) fp32, row (3 ky + kx) Cin + channel.
template <int S>
__global__ __launch_bounds__(256) void rrdb_head_kernel(_Float16* __restrict__ y, int y_pitch, const uint8_t* __restrict__ src, int h, int w,
                                                        int nh, int nw, int row0, int rows, int tiles_x, const float* __restrict__ wt,
                                                        const float* __restrict__ bias) {
  constexpr int CIN = S == 4 ? 3 : 12;
  __shared__ __attribute__((aligned(16))) float sw[9 * CIN * 64];
  __shared__ __attribute__((aligned(16))) float sb[64];
  for (int i = threadIdx.x; i < 9 * CIN * 64; i += 256) sw[i] = wt[i];
  if (threadIdx.x < 64) sb[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const int ty = blockIdx.x / tiles_x;
  const int ry = ty * 8 + (threadIdx.x >> 5), ox = (blockIdx.x - ty * tiles_x) * 32 + (threadIdx.x & 31);
  if (ry >= rows || ox >= nw) return;
  const int oy = row0 + ry;
  float acc[64];
#pragma unroll
  for (int co = 0; co < 64; ++co) acc[co] = sb[co];
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy - 1 + ky;
    if (iy < 0 || iy >= nh) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox - 1 + kx;
      if (ix < 0 || ix >= nw) continue;
#pragma unroll
      for (int c = 0; c < CIN; ++c) {
        int py = iy, px = ix, pc = c;
        if (S == 2) {
          pc = c >> 2;
          py = 2 * iy + ((c >> 1) & 1);
          px = 2 * ix + (c & 1);
          py = py >= h ? h - 2 : py;                          // the one reflected row / column of an odd side
          px = px >= w ? w - 2 : px;
        }
        const float v = (float)src[((int64_t)py * w + px) * 3 + pc] / 255.f;
        const float4* wr = reinterpret_cast<const float4*>(sw + ((ky * 3 + kx) * CIN + c) * 64);
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
  half4* yo = reinterpret_cast<half4*>(y + ((int64_t)ry * nw + ox) * y_pitch);
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    half4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (_Float16)acc[4 * q + j];
    yo[q] = o;
  }
}

// ------------------------------------------------------------------------------------------------------------------- convolutions
struct ConvArgs {
  _Float16* y;
  const _Float16* x;
  const _Float16* r1;
  const _Float16* r2;
  const uint4* wimg;
  const float* bias;
  uint8_t* out;       // tail
  float* out_f32;
  int32_t* info;
  int64_t out_pitch;
  int keep0, keepn, out_w;
  int y_pitch, x_pitch, r1_pitch, r2_pitch;
  float s1, s2;
  int Ws;             // width of the stored input tensor
  int H, W;           // the domain the convolution sees = the output map (twice the stored size with `up`)
  int nkc;            // chunks of 32 input channels
  int up, act;
  int tiles_x;
};

// NB: blocks of 16 output channels.  TAIL: bytes of the packed output instead of an f16 tensor.
template <int NB, int TAIL>
__global__ __launch_bounds__(256) void rrdb_conv_kernel(const ConvArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char s_in[kIH * kIW * kPixStride];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lp = lane & 15, lg = lane >> 4;
  const int ty = blockIdx.x / a.tiles_x;
  const int oy0 = ty * kTH, ox0 = (blockIdx.x - ty * a.tiles_x) * kTW;

  // the thread's pieces of a chunk: byte offset of the (clamped) source pixel and whether the tap lies inside the map
  uint32_t off[kLoads];
  bool in[kLoads];
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    const int idx = min((int)threadIdx.x + 256 * i, kPieces - 1), pix = idx >> 2, ch = idx & 3, rr = pix / kIW, cc = pix - rr * kIW;
    const int dy = oy0 - 1 + rr, dx = ox0 - 1 + cc;
    in[i] = dy >= 0 && dy < a.H && dx >= 0 && dx < a.W;
    const int sy = min(max(dy, 0), a.H - 1) >> a.up, sx = min(max(dx, 0), a.W - 1) >> a.up;
    off[i] = (uint32_t)(((int64_t)sy * a.Ws + sx) * a.x_pitch * 2 + ch * 16);
  }
  const unsigned char* xb = reinterpret_cast<const unsigned char*>(a.x);
  uint4 pre[kLoads];
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    const uint4 v = *reinterpret_cast<const uint4*>(xb + off[i]);
    pre[i] = in[i] ? v : make_uint4(0u, 0u, 0u, 0u);
  }

  f32x4 acc[4][NB];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // lane's pixel of block mb before the tap offset: row 2 wv + (mb >> 1), column 16 (mb & 1) + lp of the tile
  const unsigned char* pin = s_in + ((2 * wv) * kIW + lp) * kPixStride + lg * 16;
  for (int kc = 0; kc < a.nkc; ++kc) {
    if (kc) __syncthreads();                                  // the previous chunk's fragment reads are done
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int idx = threadIdx.x + 256 * i;
      if (idx < kPieces) *reinterpret_cast<uint4*>(s_in + (idx >> 2) * kPixStride + (idx & 3) * 16) = pre[i];
    }
    __syncthreads();
    if (kc + 1 < a.nkc) {
#pragma unroll
      for (int i = 0; i < kLoads; ++i) {
        const uint4 v = *reinterpret_cast<const uint4*>(xb + off[i] + (kc + 1) * 64);
        pre[i] = in[i] ? v : make_uint4(0u, 0u, 0u, 0u);
      }
    }
    const unsigned char* pw = reinterpret_cast<const unsigned char*>(a.wimg) + (int64_t)kc * 9 * NB * 1024 + lane * 16;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      half8 px[4], wt[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) wt[nb] = *reinterpret_cast<const half8*>(pw + (tap * NB + nb) * 1024);
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
        px[mb] = *reinterpret_cast<const half8*>(pin + (((mb >> 1) + ky) * kIW + (mb & 1) * 16 + kx) * kPixStride);
#pragma unroll
      for (int mb = 0; mb < 4; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[nb], px[mb], acc[mb][nb], 0, 0, 0);
    }
  }

  // epilogue: the lane holds channels 16 nb + 4 lg + r, r = 0 .. 3, of its pixel of every block
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    const int gy = oy0 + 2 * wv + (mb >> 1), gx = ox0 + (mb & 1) * 16 + lp;
    const bool inside = gy < a.H && gx < a.W;
    if constexpr (!TAIL) {
      const int64_t p = (int64_t)min(gy, a.H - 1) * a.W + min(gx, a.W - 1);      // clamped: the residual loads are unconditional
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int ch = nb * 16 + lg * 4;
        const float4 b4 = *reinterpret_cast<const float4*>(a.bias + ch);
        float v[4] = {acc[mb][nb][0] + b4.x, acc[mb][nb][1] + b4.y, acc[mb][nb][2] + b4.z, acc[mb][nb][3] + b4.w};
        if (a.act) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = v[r] >= 0.f ? v[r] : 0.2f * v[r];
        }
        if (a.r1) {
          const half4 q = *reinterpret_cast<const half4*>(a.r1 + p * a.r1_pitch + ch);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaf(a.s1, v[r], (float)q[r]);
        }
        if (a.r2) {
          const half4 q = *reinterpret_cast<const half4*>(a.r2 + p * a.r2_pitch + ch);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaf(a.s2, v[r], (float)q[r]);
        }
        half4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (_Float16)v[r];
        if (inside) *reinterpret_cast<half4*>(a.y + p * a.y_pitch + ch) = o;
      }
    } else {
      if (!inside || lg != 0 || gy < a.keep0 || gy >= a.keep0 + a.keepn || gx >= a.out_w) continue;
      const int64_t o = (int64_t)(gy - a.keep0) * a.out_pitch + (int64_t)gx * 3;
      bool bad = false;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = acc[mb][0][c] + a.bias[c];
        const bool fin = isfinite(v);
        bad = bad || !fin;
        a.out[o + c] = fin ? (uint8_t)rintf(255.f * fminf(fmaxf(v, 0.f), 1.f)) : (uint8_t)0;
        if (a.out_f32) a.out_f32[o + c] = v;
      }
      if (bad) atomicOr(a.info, VSP_RRDB_NONFINITE);
    }
  }
}

template <int NB, int TAIL>
int launch_conv(const char* what, const ConvArgs& a, vsp_stream_t stream) {
  const int64_t grid = (int64_t)a.tiles_x * ((a.H + kTH - 1) / kTH);
  VSP_REQUIRE(grid < kTwoGiB, "%s: more than 2^31 tiles", what);
  rrdb_conv_kernel<NB, TAIL><<<(unsigned)grid, 256, 0, vsp::as_stream(stream)>>>(a);
  return vsp::check_launch(what);
}

bool overlap(const void* p, int64_t pn, const void* q, int64_t qn) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" {

int vsp_rrdb_head_u8(void* y, int y_pitch, const uint8_t* src, size_t src_bytes, int64_t src_off, int h, int w, int scale, int row0, int rows,
                     const float* wt, const float* b, vsp_stream_t stream) {
  VSP_REQUIRE(y && src && wt && b, "rrdb_head: null pointer");
  VSP_REQUIRE(scale == 2 || scale == 4, "rrdb_head: scale %d (2 or 4)", scale);
  VSP_REQUIRE(h >= 1 && w >= 1 && h < (1 << 20) && w < (1 << 20), "rrdb_head: photo %d x %d", h, w);
  VSP_REQUIRE(scale == 4 || ((h % 2 == 0 || h >= 2) && (w % 2 == 0 || w >= 2)),
              "rrdb_head: photo %d x %d, the reflection of an odd side needs at least 2", h, w);
  VSP_REQUIRE(y_pitch >= 64 && y_pitch % 4 == 0, "rrdb_head: pitch %d (at least 64, a multiple of 4)", y_pitch);
  VSP_REQUIRE(aligned8(y) && vsp::aligned16(wt) && vsp::aligned16(b), "rrdb_head: buffers must be aligned (y to 8 bytes, weights to 16)");
  if ((int64_t)src_bytes >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "rrdb_head: a tensor of 2 GiB or more");
  VSP_REQUIRE(src_off >= 0 && src_off + (int64_t)3 * h * w <= (int64_t)src_bytes, "rrdb_head: photo outside src");
  const int nh = scale == 4 ? h : (h + 1) / 2, nw = scale == 4 ? w : (w + 1) / 2;
  VSP_REQUIRE(row0 >= 0 && rows >= 1 && (int64_t)row0 + rows <= nh, "rrdb_head: rows %d..%lld of %d", row0, (long long)row0 + rows - 1, nh);
  if ((int64_t)rows * nw * y_pitch * 2 >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "rrdb_head: a tensor of 2 GiB or more");
  const int tiles_x = (nw + 31) / 32;
  const unsigned grid = (unsigned)(tiles_x * ((rows + 7) / 8));
  _Float16* yo = static_cast<_Float16*>(y);
  if (scale == 4)
    rrdb_head_kernel<4><<<grid, 256, 0, vsp::as_stream(stream)>>>(yo, y_pitch, src + src_off, h, w, nh, nw, row0, rows, tiles_x, wt, b);
  else
    rrdb_head_kernel<2><<<grid, 256, 0, vsp::as_stream(stream)>>>(yo, y_pitch, src + src_off, h, w, nh, nw, row0, rows, tiles_x, wt, b);
  return vsp::check_launch("rrdb_head");
}

int vsp_rrdb_conv_f16(void* y, int y_pitch, int y_off, const void* x, int x_pitch, int H, int W, int Cin, int Cout, int flags,
                      const void* w_img, const float* b, const void* r1, int r1_pitch, float s1, const void* r2, int r2_pitch, float s2,
                      vsp_stream_t stream) {
  VSP_REQUIRE(y && x && w_img && b, "rrdb_conv: null pointer");
  VSP_REQUIRE(Cin >= 64 && Cin <= 192 && Cin % 32 == 0 && (Cout == 32 || Cout == 64),
              "rrdb_conv: %d -> %d channels; 64, 96, 128, 160, 192 -> 32, 64 are served", Cin, Cout);
  VSP_REQUIRE(H >= 1 && W >= 1 && H < (1 << 20) && W < (1 << 20), "rrdb_conv: map %d x %d", H, W);
  VSP_REQUIRE((flags & ~(VSP_RRDB_ACT | VSP_RRDB_UP)) == 0, "rrdb_conv: unknown flags %d", flags);
  VSP_REQUIRE(!r2 || r1, "rrdb_conv: a second residual without a first");
  VSP_REQUIRE(x_pitch >= Cin && x_pitch % 8 == 0, "rrdb_conv: input pitch %d (at least Cin = %d, a multiple of 8)", x_pitch, Cin);
  VSP_REQUIRE(y_off >= 0 && y_off % 4 == 0 && y_pitch % 4 == 0 && y_pitch >= y_off + Cout,
              "rrdb_conv: output pitch %d, offset %d (multiples of 4, pitch at least offset + Cout = %d)", y_pitch, y_off, y_off + Cout);
  VSP_REQUIRE(!r1 || (r1_pitch >= Cout && r1_pitch % 4 == 0), "rrdb_conv: residual pitch %d (at least Cout = %d, a multiple of 4)", r1_pitch, Cout);
  VSP_REQUIRE(!r2 || (r2_pitch >= Cout && r2_pitch % 4 == 0), "rrdb_conv: residual pitch %d (at least Cout = %d, a multiple of 4)", r2_pitch, Cout);
  VSP_REQUIRE(vsp::aligned16(x) && vsp::aligned16(w_img) && vsp::aligned16(b) && aligned8(y) && aligned8(r1) && aligned8(r2),
              "rrdb_conv: buffers must be aligned (input, weights, bias to 16 bytes; output, residuals to 8)");
  const int up = (flags & VSP_RRDB_UP) != 0;
  const int OH = up ? 2 * H : H, OW = up ? 2 * W : W;
  const int64_t xb = (int64_t)H * W * x_pitch * 2, yb = (int64_t)OH * OW * y_pitch * 2;
  const int64_t r1b = r1 ? (int64_t)OH * OW * r1_pitch * 2 : 0, r2b = r2 ? (int64_t)OH * OW * r2_pitch * 2 : 0;
  if (xb >= kTwoGiB || yb >= kTwoGiB || r1b >= kTwoGiB || r2b >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "rrdb_conv: a tensor of 2 GiB or more");
  // the output may be a slice of the tensor it reads -- same base, same pitch, behind the channels read -- and nothing else of it
  if (y == x)
    VSP_REQUIRE(!up && y_pitch == x_pitch && y_off >= Cin, "rrdb_conv: the output slice %d..%d overlaps the channels 0..%d it reads", y_off,
                y_off + Cout - 1, Cin - 1);
  else
    VSP_REQUIRE(!overlap(y, yb, x, xb), "rrdb_conv: the output overlaps the input without being a slice of it");
  // a residual reads channels 0 .. Cout - 1 of its tensor: inside the output tensor only beside the slice written
  const void* rs[2] = {r1, r2};
  const int rp[2] = {r1_pitch, r2_pitch};
  const int64_t rb[2] = {r1b, r2b};
  for (int i = 0; i < 2; ++i) {
    if (!rs[i] || !overlap(y, yb, rs[i], rb[i])) continue;
    VSP_REQUIRE(rs[i] == y && rp[i] == y_pitch && y_off >= Cout, "rrdb_conv: residual %d aliases what the launch writes", i + 1);
  }
  ConvArgs a = {};
  a.y = static_cast<_Float16*>(y) + y_off, a.x = static_cast<const _Float16*>(x);
  a.r1 = static_cast<const _Float16*>(r1), a.r2 = static_cast<const _Float16*>(r2);
  a.wimg = static_cast<const uint4*>(w_img), a.bias = b;
  a.y_pitch = y_pitch, a.x_pitch = x_pitch, a.r1_pitch = r1_pitch, a.r2_pitch = r2_pitch, a.s1 = s1, a.s2 = s2;
  a.Ws = W, a.H = OH, a.W = OW, a.nkc = Cin / 32, a.up = up, a.act = (flags & VSP_RRDB_ACT) != 0;
  a.tiles_x = (OW + kTW - 1) / kTW;
  if (Cout == 32) return launch_conv<2, 0>("rrdb_conv", a, stream);
  return launch_conv<4, 0>("rrdb_conv", a, stream);
}

int vsp_rrdb_tail_u8(uint8_t* out, size_t out_bytes, int64_t out_off, int64_t out_pitch, int out_w, float* out_f32, int32_t* info,
                     const void* x, int x_pitch, int H, int W, int keep0, int keepn, const void* w_img, const float* b, vsp_stream_t stream) {
  VSP_REQUIRE(out && info && x && w_img && b, "rrdb_tail: null pointer");
  VSP_REQUIRE(H >= 1 && W >= 1 && H < (1 << 20) && W < (1 << 20), "rrdb_tail: map %d x %d", H, W);
  VSP_REQUIRE(x_pitch >= 64 && x_pitch % 8 == 0, "rrdb_tail: input pitch %d (at least 64, a multiple of 8)", x_pitch);
  VSP_REQUIRE(vsp::aligned16(x) && vsp::aligned16(w_img) && vsp::aligned16(b), "rrdb_tail: buffers must be 16-byte aligned");
  VSP_REQUIRE(keep0 >= 0 && keepn >= 1 && (int64_t)keep0 + keepn <= H, "rrdb_tail: rows %d..%lld of %d", keep0, (long long)keep0 + keepn - 1, H);
  VSP_REQUIRE(out_w >= 1 && out_w <= W, "rrdb_tail: %d columns of %d", out_w, W);
  if ((int64_t)H * W * x_pitch * 2 >= kTwoGiB || (int64_t)out_bytes >= kTwoGiB || (out_f32 && (int64_t)out_bytes * 4 >= kTwoGiB))
    return vsp::fail(VSP_ENOTSUP, "rrdb_tail: a tensor of 2 GiB or more");
  VSP_REQUIRE(out_off >= 0 && out_pitch >= (int64_t)3 * out_w && out_off + (int64_t)(keepn - 1) * out_pitch + (int64_t)3 * out_w <= (int64_t)out_bytes,
              "rrdb_tail: bytes outside out");
  ConvArgs a = {};
  a.x = static_cast<const _Float16*>(x), a.wimg = static_cast<const uint4*>(w_img), a.bias = b;
  a.out = out + out_off, a.out_f32 = out_f32 ? out_f32 + out_off : nullptr, a.info = info;
  a.out_pitch = out_pitch, a.keep0 = keep0, a.keepn = keepn, a.out_w = out_w;
  a.x_pitch = x_pitch, a.Ws = W, a.H = H, a.W = W, a.nkc = 2;
  a.tiles_x = (W + kTW - 1) / kTW;
  return launch_conv<1, 1>("rrdb_tail", a, stream);
}

}  // extern "C"

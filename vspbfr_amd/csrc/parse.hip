// Face-parsing paste masks for whole photos: facexlib's ParseNet on f16 operands, and the integer blur that turns its class
// map into paste weights.
//   parse_head_kernel          u8 RGB crops -> (u8 / 255 - 0.5) / 0.5, reflection, 3 -> 64 3x3, + bias; fp32 fmaf, f16 NHWC out
//   parse_conv_kernel<ST, 4, 0> every 3x3 between head and tail as an implicit GEMM on v_mfma_f32_16x16x32_f16: Cin, Cout multiples of 64,
//                              stride ST = 1 / 2, optional fused nearest x2 of the input, reflection by index, + fp32 bias, LeakyReLU(0.2),
//                              up to two f16 residuals, one rounding to f16
//   parse_conv_kernel<1, 2, 1> tail: 64 -> 19 (padded to 32), fp32 logits, argmax (ties to the lowest class), keep table, non-finite flag
//   parse_blur_kernel<V, LAST> one 1-D pass of the integer Gaussian (reflect-101), the last one with the weight and the border
// Activations are (F, H, W, C) _Float16, faces back to back; the tile list runs across the faces of a call.
//
// parse_conv_kernel: 256 threads; a workgroup owns one tile of 8 rows x TW columns of output pixels (TW = 32 at stride 1, 16 at stride 2)
// and one block of 64 output channels (128 at stride 2 where Cout allows it).  K = 9 Cin is walked in chunks of 64 input channels: the chunk's input tile with its halo goes to
// LDS at sr.hip's 144-byte pixel stride (10 x 34 pixels at stride 1; 17 x 33 at stride 2, its columns split by parity so that the 16
// pixels of a fragment read stay 144 bytes apart), upsampling and reflection resolved in the address of the global load, which is
// branch-free (clamped address).  The layer's weights do not fit LDS (256 -> 256: 1.18 MB), and a chunk's share of them is read once per
// wave: so the weight fragments come straight from the packed image in L2, 1 KiB of consecutive bytes per wave and MFMA operand.  Wave v
// owns rows 2 v and 2 v + 1 of the tile.  As in sr.hip the WEIGHTS are the MFMA's A operand and the pixels its B operand: a lane holds
// four consecutive output channels of one pixel, the f16 result leaves as 8-byte stores, and a residual is read at exactly the address
// the lane writes -- which is why a residual may be the output tensor itself.
#include "vsp_common.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTH = 8;                                        // rows of an output tile
constexpr int kPixStride = 144;                               // bytes per pixel of the LDS input tile (128 + 16 of padding)
constexpr int kIWp = 34;                                      // pixel positions per LDS row, both strides
constexpr int64_t kTwoGiB = (int64_t)1 << 31;

struct KeepTable { uint8_t v[VSP_PARSE_CLASSES + 1]; };
struct TapTable { int32_t g[VSP_PARSE_MAX_RADIUS + 1]; };

// reflection by index (-1 -> 1, n -> n - 2), then clamped: a tile may overhang the map, and what lies past the reflection ring only
// feeds outputs that are never stored
__device__ __forceinline__ int reflect_clamp(int d, int n) {
  d = d < 0 ? -d : d;
  d = d >= n ? 2 * n - 2 - d : d;
  return min(max(d, 0), n - 1);
}

// ---------------------------------------------------------------------------------------------------------------------------- head
__global__ __launch_bounds__(256) void parse_head_kernel(_Float16* __restrict__ y, const uint8_t* __restrict__ src, int H, int W,
                                                         int tiles_x, int tiles_face, const float* __restrict__ w,
                                                         const float* __restrict__ bias) {
  __shared__ __attribute__((aligned(16))) float sw[27 * 64];
  __shared__ __attribute__((aligned(16))) float sb[64];
  for (int i = threadIdx.x; i < 27 * 64; i += 256) sw[i] = w[i];
  if (threadIdx.x < 64) sb[threadIdx.x] = bias[threadIdx.x];
  __syncthreads();
  const int f = blockIdx.x / tiles_face, t = blockIdx.x - f * tiles_face, ty = t / tiles_x;
  const int oy = ty * 8 + (threadIdx.x >> 5), ox = (t - ty * tiles_x) * 32 + (threadIdx.x & 31);
  if (oy >= H || ox >= W) return;
  float acc[64];
#pragma unroll
  for (int co = 0; co < 64; ++co) acc[co] = sb[co];
  const uint8_t* ph = src + (int64_t)f * H * W * 3;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = reflect_clamp(oy - 1 + ky, H);
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = reflect_clamp(ox - 1 + kx, W);
      const uint8_t* px = ph + ((int64_t)iy * W + ix) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = ((float)px[c] / 255.f - 0.5f) / 0.5f;
        const float4* wr = reinterpret_cast<const float4*>(sw + ((ky * 3 + kx) * 3 + c) * 64);
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
  half8* yo = reinterpret_cast<half8*>(y + (((int64_t)f * H + oy) * W + ox) * 64);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (_Float16)acc[8 * q + j];
    yo[q] = o;
  }
}

// ------------------------------------------------------------------------------------------------------------------- convolutions
struct ConvArgs {
  _Float16* y;
  const _Float16* x;
  const _Float16* res1;
  const _Float16* res2;
  const uint4* wimg;
  const float* bias;
  uint8_t* cls;       // tail
  uint8_t* keep;
  float* logits;
  int32_t* info;
  int Hs, Ws;         // the stored input tensor
  int Hd, Wd;         // the domain the convolution sees (twice the stored size with `up`)
  int OH, OW;
  int Cin, Cout;
  int up, act;
  int tiles_x, tiles_face, ntiles;
};

template <int ST> struct Geo {
  static constexpr int TW = ST == 1 ? 32 : 16;                // output columns of a tile
  static constexpr int MBX = TW / 16;                         // blocks of 16 pixels per tile row
  static constexpr int IH = ST * (kTH - 1) + 3;               // input rows with halo: 10 / 17
  static constexpr int IW = ST * (TW - 1) + 3;                // input columns with halo: 34 / 33
  static constexpr int CHUNKS = IH * IW * 8;                  // 16-byte pieces of one chunk's tile
  static constexpr int LDS = IH * kIWp * kPixStride;          // 48 960 / 83 232
  // LDS position of input column c: at stride 2 the even columns first, then the odd ones
  __device__ static __forceinline__ int pos(int c) { return ST == 1 ? c : (c & 1) * 17 + (c >> 1); }
};

// ST: stride.  NB: blocks of 16 output channels per workgroup (2: the tail's padded 32; 4: one 64-channel unit of the weight image; 8: two
// units, which halves the input traffic per MFMA where a stride-2 tile has few pixels).  TAIL: logits, argmax and keep map instead of an
// f16 tensor.
template <int ST, int NB, int TAIL>
__global__ __launch_bounds__(256) void parse_conv_kernel(const ConvArgs a, const KeepTable kt) {
  using G = Geo<ST>;
  constexpr int MB = 2 * G::MBX;                              // pixel blocks per wave
  constexpr int WB = NB < 4 ? NB : 4;                         // channel blocks per unit of the weight image
  constexpr int NU = NB / WB;                                 // units per workgroup
  extern __shared__ __attribute__((aligned(16))) unsigned char s_in[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lp = lane & 15, lg = lane >> 4;
  const int ncb = TAIL ? 1 : a.Cout / (16 * NB);
  const int tile = blockIdx.x / ncb, cb = blockIdx.x - tile * ncb;
  const int f = tile / a.tiles_face, t = tile - f * a.tiles_face, ty = t / a.tiles_x;
  const int oy0 = ty * kTH, ox0 = (t - ty * a.tiles_x) * G::TW;
  const int nkc = a.Cin >> 6;
  const uint4* xin = reinterpret_cast<const uint4*>(a.x + (int64_t)f * a.Hs * a.Ws * a.Cin);
  const int cin8 = a.Cin >> 3;

  f32x4 acc[MB][NB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  // lane's pixel of block mb before the tap offset: row 2 wv + mb / MBX, column 16 (mb % MBX) + lp of the tile
  const unsigned char* pin = s_in + lg * 16;
  for (int kc = 0; kc < nkc; ++kc) {
    if (kc) __syncthreads();                                  // the previous chunk's fragment reads are done
    for (int idx = threadIdx.x; idx < G::CHUNKS; idx += 256) {
      const int pix = idx >> 3, ch = idx & 7, rr = pix / G::IW, cc = pix - rr * G::IW;
      int sy = reflect_clamp(ST * oy0 - 1 + rr, a.Hd), sx = reflect_clamp(ST * ox0 - 1 + cc, a.Wd);
      if (a.up) { sy >>= 1; sx >>= 1; }
      const uint4 v = xin[((int64_t)sy * a.Ws + sx) * cin8 + kc * 8 + ch];
      *reinterpret_cast<uint4*>(s_in + (rr * kIWp + G::pos(cc)) * kPixStride + ch * 16) = v;
    }
    __syncthreads();
    const unsigned char* pw = reinterpret_cast<const unsigned char*>(a.wimg) + ((int64_t)(cb * NU * nkc + kc) * 18 * WB) * 1024 + lane * 16;
    const int64_t unit = (int64_t)nkc * 18 * WB * 1024;       // bytes from one 64-channel unit of the image to the next
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        half8 px[MB], wt[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          wt[nb] = *reinterpret_cast<const half8*>(pw + (nb / WB) * unit + ((2 * tap + hf) * WB + nb % WB) * 1024);
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
          const int row = ST * (2 * wv + mb / G::MBX) + ky;
          const int p = ST == 1 ? 16 * (mb % G::MBX) + lp + kx : (kx & 1) * 17 + 16 * (mb % G::MBX) + lp + (kx >> 1);
          px[mb] = *reinterpret_cast<const half8*>(pin + (row * kIWp + p) * kPixStride + hf * 64);
        }
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[nb], px[mb], acc[mb][nb], 0, 0, 0);
      }
    }
  }

  // epilogue: the lane holds channels 16 nb + 4 lg + r, r = 0 .. 3, of its pixel of every block
  if constexpr (!TAIL) {
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int gy = oy0 + 2 * wv + mb / G::MBX, gx = ox0 + 16 * (mb % G::MBX) + lp;
      if (gy >= a.OH || gx >= a.OW) continue;
      const int64_t o = (((int64_t)f * a.OH + gy) * a.OW + gx) * a.Cout + cb * 16 * NB + lg * 4;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const float4 b4 = *reinterpret_cast<const float4*>(a.bias + cb * 16 * NB + nb * 16 + lg * 4);
        float v[4] = {acc[mb][nb][0] + b4.x, acc[mb][nb][1] + b4.y, acc[mb][nb][2] + b4.z, acc[mb][nb][3] + b4.w};
        if (a.act) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = v[r] >= 0.f ? v[r] : 0.2f * v[r];
        }
        if (a.res1) {
          const half4 q = *reinterpret_cast<const half4*>(a.res1 + o + nb * 16);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)q[r];
        }
        if (a.res2) {
          const half4 q = *reinterpret_cast<const half4*>(a.res2 + o + nb * 16);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += (float)q[r];
        }
        half4 h;
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = (_Float16)v[r];
        *reinterpret_cast<half4*>(a.y + o + nb * 16) = h;
      }
    }
  } else {
    // the tile's logits through LDS (33 floats per pixel), then one thread per pixel
    __syncthreads();
    float* s_log = reinterpret_cast<float*>(s_in);
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int pl = (2 * wv + mb / G::MBX) * G::TW + 16 * (mb % G::MBX) + lp;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ch = nb * 16 + lg * 4 + r;
          s_log[pl * 33 + ch] = acc[mb][nb][r] + a.bias[ch];
        }
    }
    __syncthreads();
    const int gy = oy0 + (int)threadIdx.x / G::TW, gx = ox0 + (int)threadIdx.x % G::TW;
    if (gy < a.OH && gx < a.OW) {
      const float* lg_ = s_log + threadIdx.x * 33;
      const int64_t p = ((int64_t)f * a.OH + gy) * a.OW + gx;
      int best = 0;
      float bv = lg_[0];
      bool fin = isfinite(bv);
      for (int c = 1; c < VSP_PARSE_CLASSES; ++c) {
        const float v = lg_[c];
        fin = fin && isfinite(v);
        if (v > bv) { bv = v; best = c; }                     // strictly greater: a tie stays with the lower class
      }
      if (!fin) best = 0;
      a.cls[p] = (uint8_t)best;
      a.keep[p] = kt.v[best];
      if (a.logits)
        for (int c = 0; c < VSP_PARSE_CLASSES; ++c) a.logits[p * VSP_PARSE_CLASSES + c] = lg_[c];
      if (!fin) atomicOr(a.info + f, VSP_PARSE_NONFINITE);
    }
  }
}

template <int ST, int NB, int TAIL>
int launch_conv(const char* what, const ConvArgs& a, const KeepTable& kt, vsp_stream_t stream) {
  static vsp::LdsAttrOnce once;
  const void* fn = reinterpret_cast<const void*>(&parse_conv_kernel<ST, NB, TAIL>);
  if (int rc = once.ensure(fn, Geo<ST>::LDS, what)) return rc;
  const int64_t grid = (int64_t)a.ntiles * (TAIL ? 1 : a.Cout / (16 * NB));
  VSP_REQUIRE(grid < kTwoGiB, "%s: more than 2^31 workgroups", what);
  parse_conv_kernel<ST, NB, TAIL><<<(unsigned)grid, 256, Geo<ST>::LDS, vsp::as_stream(stream)>>>(a, kt);
  return vsp::check_launch(what);
}

bool overlap(const void* p, int64_t pn, const void* q, int64_t qn) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
  return a < b + (uintptr_t)qn && b < a + (uintptr_t)pn;
}

// -------------------------------------------------------------------------------------------------------------------------- blur
__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * (n - 1) - i : i;
}

// V: along columns (0) or rows (1).  FIRST: the source is the u8 keep map (m0 = 16384 keep).  LAST: write the weight with its border.
template <int V, int FIRST, int LAST>
__global__ __launch_bounds__(256) void parse_blur_kernel(uint16_t* __restrict__ dst, const uint16_t* __restrict__ src,
                                                         const uint8_t* __restrict__ keep, int S, int64_t total, int R, int border,
                                                         const TapTable tt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % S), y = (int)((i / S) % S);
  const int64_t row0 = V ? i - (int64_t)y * S : i - x;         // element of the line's coordinate 0
  const int c = V ? y : x, step = V ? S : 1;
  int32_t sum = 0;
  for (int k = -R; k <= R; ++k) {
    const int64_t j = row0 + (int64_t)reflect101(c + k, S) * step;
    const int32_t m = FIRST ? (keep[j] ? 16384 : 0) : (int32_t)src[j];
    sum += tt.g[k < 0 ? -k : k] * m;
  }
  int32_t m = (sum + 32768) >> 16;
  if (LAST) {
    m = (m + 32) >> 6;
    if (x < border || y < border || x >= S - border || y >= S - border) m = 0;
  }
  dst[i] = (uint16_t)m;
}

}  // namespace

extern "C" {

int vsp_parse_head_u8(void* y, const uint8_t* crops, int F, int H, int W, const float* w, const float* b, vsp_stream_t stream) {
  VSP_REQUIRE(F >= 0, "parse_head: %d faces", F);
  if (F == 0) return VSP_OK;
  VSP_REQUIRE(y && crops && w && b, "parse_head: null pointer");
  VSP_REQUIRE(H >= 2 && W >= 2, "parse_head: map %d x %d, the reflection needs at least 2 x 2", H, W);
  VSP_REQUIRE(vsp::aligned16(y) && vsp::aligned16(w) && vsp::aligned16(b), "parse_head: buffers must be 16-byte aligned");
  if ((int64_t)F * H * W * 128 >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "parse_head: a tensor of 2 GiB or more");
  const int tiles_x = (W + 31) / 32, tiles_face = tiles_x * ((H + 7) / 8);
  parse_head_kernel<<<(unsigned)((int64_t)F * tiles_face), 256, 0, vsp::as_stream(stream)>>>(static_cast<_Float16*>(y), crops, H, W, tiles_x,
                                                                                          tiles_face, w, b);
  return vsp::check_launch("parse_head");
}

int vsp_parse_conv_f16(void* y, const void* x, int F, int H, int W, int Cin, int Cout, int stride, int flags, const void* w_img,
                       const float* b, const void* res1, const void* res2, vsp_stream_t stream) {
  VSP_REQUIRE(F >= 0, "parse_conv: %d faces", F);
  if (F == 0) return VSP_OK;
  VSP_REQUIRE(y && x && w_img && b, "parse_conv: null pointer");
  VSP_REQUIRE(Cin >= 64 && Cin % 64 == 0 && Cout >= 64 && Cout % 64 == 0, "parse_conv: %d -> %d channels, multiples of 64 are served", Cin, Cout);
  VSP_REQUIRE(H >= 2 && W >= 2, "parse_conv: map %d x %d, the reflection needs at least 2 x 2", H, W);
  VSP_REQUIRE(stride == 1 || stride == 2, "parse_conv: stride %d (1 or 2)", stride);
  VSP_REQUIRE((flags & ~(VSP_PARSE_ACT | VSP_PARSE_UP)) == 0, "parse_conv: unknown flags %d", flags);
  const int up = (flags & VSP_PARSE_UP) != 0;
  VSP_REQUIRE(!(up && stride == 2), "parse_conv: up together with stride 2");
  VSP_REQUIRE(!res2 || res1, "parse_conv: a second residual without a first");
  VSP_REQUIRE(vsp::aligned16(y) && vsp::aligned16(x) && vsp::aligned16(w_img) && vsp::aligned16(b) && vsp::aligned16(res1) && vsp::aligned16(res2),
              "parse_conv: buffers must be 16-byte aligned");
  VSP_REQUIRE(H < (1 << 20) && W < (1 << 20), "parse_conv: map %d x %d", H, W);
  const int Hd = up ? 2 * H : H, Wd = up ? 2 * W : W;
  const int OH = stride == 2 ? (Hd - 1) / 2 + 1 : Hd, OW = stride == 2 ? (Wd - 1) / 2 + 1 : Wd;
  const int64_t xb = (int64_t)F * H * W * Cin * 2, yb = (int64_t)F * OH * OW * Cout * 2;
  if (xb >= kTwoGiB || yb >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "parse_conv: a tensor of 2 GiB or more");
  VSP_REQUIRE(!overlap(y, yb, x, xb), "parse_conv: the output overlaps the input");
  VSP_REQUIRE(res1 == y || !res1 || !overlap(y, yb, res1, yb), "parse_conv: a residual overlaps the output without being it");
  VSP_REQUIRE(res2 == y || !res2 || !overlap(y, yb, res2, yb), "parse_conv: a residual overlaps the output without being it");
  ConvArgs a = {};
  a.y = static_cast<_Float16*>(y), a.x = static_cast<const _Float16*>(x);
  a.res1 = static_cast<const _Float16*>(res1), a.res2 = static_cast<const _Float16*>(res2);
  a.wimg = static_cast<const uint4*>(w_img), a.bias = b;
  a.Hs = H, a.Ws = W, a.Hd = Hd, a.Wd = Wd, a.OH = OH, a.OW = OW, a.Cin = Cin, a.Cout = Cout, a.up = up, a.act = (flags & VSP_PARSE_ACT) != 0;
  const int tw = stride == 1 ? 32 : 16;
  a.tiles_x = (OW + tw - 1) / tw;
  a.tiles_face = a.tiles_x * ((OH + kTH - 1) / kTH);
  const int64_t ntiles = (int64_t)F * a.tiles_face;
  VSP_REQUIRE(ntiles < kTwoGiB, "parse_conv: more than 2^31 tiles");
  a.ntiles = (int)ntiles;
  const KeepTable kt = {};
  if (stride == 1) return launch_conv<1, 4, 0>("parse_conv", a, kt, stream);
  if (Cout % 128 == 0) return launch_conv<2, 8, 0>("parse_conv", a, kt, stream);
  return launch_conv<2, 4, 0>("parse_conv", a, kt, stream);
}

int vsp_parse_mask_u8(uint8_t* cls, uint8_t* keep, float* logits, int32_t* info, const void* x, int F, int H, int W, const void* w_img,
                      const float* b, const uint8_t* keep_table, vsp_stream_t stream) {
  VSP_REQUIRE(F >= 0, "parse_mask: %d faces", F);
  if (F == 0) return VSP_OK;
  VSP_REQUIRE(cls && keep && info && x && w_img && b && keep_table, "parse_mask: null pointer");
  VSP_REQUIRE(H >= 2 && W >= 2, "parse_mask: map %d x %d, the reflection needs at least 2 x 2", H, W);
  VSP_REQUIRE(vsp::aligned16(x) && vsp::aligned16(w_img), "parse_mask: buffers must be 16-byte aligned");
  VSP_REQUIRE(H < (1 << 20) && W < (1 << 20), "parse_mask: map %d x %d", H, W);
  KeepTable kt = {};
  for (int c = 0; c < VSP_PARSE_CLASSES; ++c) {
    VSP_REQUIRE(keep_table[c] <= 1, "parse_mask: keep table entry %d is %d (0 or 1)", c, keep_table[c]);
    kt.v[c] = keep_table[c];
  }
  const int64_t px = (int64_t)F * H * W;
  if (px * 128 >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "parse_mask: a tensor of 2 GiB or more");
  ConvArgs a = {};
  a.x = static_cast<const _Float16*>(x), a.wimg = static_cast<const uint4*>(w_img), a.bias = b;
  a.cls = cls, a.keep = keep, a.logits = logits, a.info = info;
  a.Hs = a.Hd = a.OH = H, a.Ws = a.Wd = a.OW = W, a.Cin = 64, a.Cout = 32;
  a.tiles_x = (W + 31) / 32;
  a.tiles_face = a.tiles_x * ((H + kTH - 1) / kTH);
  a.ntiles = (int)(F * (int64_t)a.tiles_face);
  return launch_conv<1, 2, 1>("parse_mask", a, kt, stream);
}

int vsp_parse_blur_u16(uint16_t* out, const uint8_t* keep, uint16_t* work, size_t work_bytes, int F, int S, const int32_t* taps, int R,
                       int border, vsp_stream_t stream) {
  VSP_REQUIRE(F >= 0, "parse_blur: %d faces", F);
  if (F == 0) return VSP_OK;
  VSP_REQUIRE(out && keep && work && taps, "parse_blur: null pointer");
  VSP_REQUIRE(S >= 2 && S <= 32768, "parse_blur: size %d", S);
  VSP_REQUIRE(R >= 0 && R <= VSP_PARSE_MAX_RADIUS && R <= S - 1, "parse_blur: radius %d (0..%d and at most size - 1 = %d)", R,
              VSP_PARSE_MAX_RADIUS, S - 1);
  VSP_REQUIRE(border >= 0 && 2 * border <= S, "parse_blur: border %d of a size of %d", border, S);
  TapTable tt = {};
  int64_t sum = 0;
  for (int k = 0; k <= R; ++k) {
    VSP_REQUIRE(taps[k] >= 0 && taps[k] <= 65536, "parse_blur: tap %d is %d", k, taps[k]);
    tt.g[k] = taps[k];
    sum += k ? 2 * (int64_t)taps[k] : taps[k];
  }
  VSP_REQUIRE(sum == 65536, "parse_blur: the taps sum to %lld, not 65536", (long long)sum);
  const int64_t n = (int64_t)F * S * S;
  if (n * 2 >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "parse_blur: a tensor of 2 GiB or more");
  VSP_REQUIRE((int64_t)work_bytes >= 4 * n, "parse_blur: work of %zu bytes, %lld needed", work_bytes, (long long)(4 * n));
  VSP_REQUIRE(!overlap(out, 2 * n, work, 4 * n) && !overlap(out, 2 * n, keep, n) && !overlap(work, 4 * n, keep, n), "parse_blur: buffers overlap");
  uint16_t* wa = work;
  uint16_t* wb = work + n;
  const unsigned grid = (unsigned)((n + 255) / 256);
  hipStream_t s = vsp::as_stream(stream);
  parse_blur_kernel<0, 1, 0><<<grid, 256, 0, s>>>(wa, nullptr, keep, S, n, R, border, tt);
  parse_blur_kernel<1, 0, 0><<<grid, 256, 0, s>>>(wb, wa, nullptr, S, n, R, border, tt);
  parse_blur_kernel<0, 0, 0><<<grid, 256, 0, s>>>(wa, wb, nullptr, S, n, R, border, tt);
  parse_blur_kernel<1, 0, 1><<<grid, 256, 0, s>>>(out, wa, nullptr, S, n, R, border, tt);
  return vsp::check_launch("parse_blur");
}

}  // extern "C"

// Background upscaling for whole photos: Real-ESRGAN's compact network (SRVGGNetCompact, 64 features) on f16 operands.
//   sr_head_kernel          u8 RGB photos where they lie -> x / 255, 3 -> 64 3x3 (zero padding), + bias, PReLU; fp32 fmaf, f16 NHWC out
//   sr_conv_kernel<4, 0>    body: 64 -> 64 3x3 as an implicit GEMM on v_mfma_f32_16x16x32_f16, + fp32 bias, fp32 PReLU, f16 NHWC out
//   sr_conv_kernel<NB, S>   tail: 64 -> 3 S^2 (NB = 1 / 3 blocks of 16 output channels, zero-padded), + bias, pixel shuffle, + u8 / 255 of
//                           the source pixel, clamp, rintf(255 v) as u8 into the packed output (and the unclamped fp32 value for tests)
// Activations are (h, w, 64) _Float16 per item, items back to back at vsp_sr_item.act_off pixels.  One launch serves a whole ragged group:
// the tile list (8 rows x 32 columns of output pixels) runs across the items, a workgroup finds its item by bisection over tile0.
//
// sr_conv_kernel: 256 threads, one workgroup per CU, persistent (tile += gridDim.x).  LDS holds the layer's whole weight image
// (18 K-steps x NB blocks x 64 lanes x 16 B: 73 728 B for the body) for the lifetime of the workgroup, and one input tile with its halo,
// 10 x 34 pixels at a 144-byte pixel stride (48 960 B; 144 B = 36 dwords puts the 16 pixels of a ds_read_b128 quarter on 16 disjoint bank
// quads).  The next tile's 2 720 16-byte chunks are fetched into registers before the MFMA loop of the current one and stored to LDS behind it.
// Wave v owns rows 2 v and 2 v + 1 of the tile: four blocks of 16 consecutive pixels x NB channel blocks.  The WEIGHTS are the MFMA's A operand
// and the pixels its B operand, so an accumulator holds four consecutive output channels of one pixel per lane (column = lane & 15 = pixel,
// row = 4 (lane >> 4) + r = channel of the block) and the f16 result leaves as one 8-byte store per block.
// K = 576 is ordered tap-major: K-step s = 2 (3 ky + kx) + half covers input channels 32 half .. 32 half + 31 of tap (ky, kx); lane l supplies
// k = 8 (l >> 4) + j, j = 0 .. 7, of the step for both operands (upscale.pack_body_weight writes exactly that image).
#include "vsp_common.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTH = VSP_SR_TILE_H, kTW = VSP_SR_TILE_W, kIH = kTH + 2, kIW = kTW + 2;
constexpr int kPixStride = 144;                               // bytes per pixel of the LDS input tile (128 + 16 of padding)
constexpr int kInBytes = kIH * kIW * kPixStride;              // 48 960
constexpr int kChunks = kIH * kIW * 8;                        // 16-byte chunks of a tile with halo: 2 720
constexpr int kLoads = (kChunks + 255) / 256;                 // per thread: 11
constexpr int kSteps = 18;                                    // K-steps of 32: 9 taps x 2 channel halves

// the item of a tile: the last one whose tile0 is not above it (tile0 ascends, items[0].tile0 = 0)
__device__ __forceinline__ int sr_find(const vsp_sr_item* __restrict__ items, int n, int tile) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ void sr_tile_origin(const vsp_sr_item& it, int tile, int& ty0, int& tx0) {
  const int tiles_x = (it.w + kTW - 1) / kTW, t = tile - it.tile0, ty = t / tiles_x;
  ty0 = ty * kTH;
  tx0 = (t - ty * tiles_x) * kTW;
}

// ---------------------------------------------------------------------------------------------------------------------------- head
__global__ __launch_bounds__(256) void sr_head_kernel(_Float16* __restrict__ y, const uint8_t* __restrict__ src,
                                                      const vsp_sr_item* __restrict__ items, int n, const float* __restrict__ w,
                                                      const float* __restrict__ bias, const float* __restrict__ slope) {
  __shared__ __attribute__((aligned(16))) float sw[27 * 64];
  __shared__ __attribute__((aligned(16))) float sb[64], sa[64];
  for (int i = threadIdx.x; i < 27 * 64; i += 256) sw[i] = w[i];
  if (threadIdx.x < 64) { sb[threadIdx.x] = bias[threadIdx.x]; sa[threadIdx.x] = slope[threadIdx.x]; }
  __syncthreads();
  const vsp_sr_item it = items[sr_find(items, n, blockIdx.x)];
  int ty0, tx0;
  sr_tile_origin(it, blockIdx.x, ty0, tx0);
  const int oy = ty0 + (threadIdx.x >> 5), ox = tx0 + (threadIdx.x & 31);
  if (oy >= it.h || ox >= it.w) return;
  float acc[64];
#pragma unroll
  for (int co = 0; co < 64; ++co) acc[co] = sb[co];
  const uint8_t* ph = src + it.src_off;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy - 1 + ky;
    if (iy < 0 || iy >= it.h) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox - 1 + kx;
      if (ix < 0 || ix >= it.w) continue;
      const uint8_t* px = ph + ((int64_t)iy * it.w + ix) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = (float)px[c] / 255.f;
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
  half8* yo = reinterpret_cast<half8*>(y + (it.act_off + (int64_t)oy * it.w + ox) * 64);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = acc[8 * q + j];
      o[j] = (_Float16)(v >= 0.f ? v : sa[8 * q + j] * v);
    }
    yo[q] = o;
  }
}

// ------------------------------------------------------------------------------------------------------------------- body and tail
__device__ __forceinline__ void sr_fetch(uint4 (&r)[kLoads], const _Float16* __restrict__ x, const vsp_sr_item& it, int ty0, int tx0) {
  const uint4* base = reinterpret_cast<const uint4*>(x + it.act_off * 64);
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    const int idx = threadIdx.x + 256 * i, pix = idx >> 3, ch = idx & 7, rr = pix / kIW, cc = pix - rr * kIW;
    const int iy = ty0 - 1 + rr, ix = tx0 - 1 + cc;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (idx < kChunks && iy >= 0 && iy < it.h && ix >= 0 && ix < it.w) v = base[((int64_t)iy * it.w + ix) * 8 + ch];
    r[i] = v;
  }
}

__device__ __forceinline__ void sr_commit(unsigned char* s_in, const uint4 (&r)[kLoads]) {
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    const int idx = threadIdx.x + 256 * i, pix = idx >> 3, ch = idx & 7;
    if (idx < kChunks) *reinterpret_cast<uint4*>(s_in + pix * kPixStride + ch * 16) = r[i];
  }
}

// NB: blocks of 16 output channels.  S = 0: body (f16 NHWC out, PReLU); S = 2 / 4: tail (pixel shuffle by S, skip, u8 out).
template <int NB, int S>
__global__ __launch_bounds__(256) void sr_conv_kernel(_Float16* __restrict__ y, uint8_t* __restrict__ out, float* __restrict__ out_f32,
                                                      int32_t* __restrict__ info, const _Float16* __restrict__ x,
                                                      const uint8_t* __restrict__ src, const vsp_sr_item* __restrict__ items, int n,
                                                      int ntiles, const uint4* __restrict__ wimg, const float* __restrict__ bias,
                                                      const float* __restrict__ slope) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* s_in = smem;
  unsigned char* s_w = smem + kInBytes;
  float* s_b = reinterpret_cast<float*>(smem + kInBytes + kSteps * NB * 1024);
  float* s_a = s_b + NB * 16;
  for (int i = threadIdx.x; i < kSteps * NB * 64; i += 256) reinterpret_cast<uint4*>(s_w)[i] = wimg[i];
  if (threadIdx.x < NB * 16) {
    s_b[threadIdx.x] = bias[threadIdx.x];
    if constexpr (S == 0) s_a[threadIdx.x] = slope[threadIdx.x];
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lp = lane & 15, lg = lane >> 4;

  int tile = blockIdx.x;
  if (tile >= ntiles) return;
  vsp_sr_item it = items[sr_find(items, n, tile)];
  int ty0, tx0;
  sr_tile_origin(it, tile, ty0, tx0);
  uint4 pre[kLoads];
  sr_fetch(pre, x, it, ty0, tx0);
  while (true) {
    __syncthreads();                                          // the previous tile's fragment reads are done (first pass: none)
    sr_commit(s_in, pre);
    __syncthreads();                                          // tile and (first pass) weights are in LDS
    const vsp_sr_item cur = it;
    const int cy0 = ty0, cx0 = tx0;
    const int next = tile + gridDim.x;
    if (next < ntiles) {
      it = items[sr_find(items, n, next)];
      sr_tile_origin(it, next, ty0, tx0);
      sr_fetch(pre, x, it, ty0, tx0);
    }

    f32x4 acc[4][NB];
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    // lane's pixel of block mb, before the tap offset: row 2 wv + (mb >> 1), column 16 (mb & 1) + lp of the tile
    const unsigned char* pin = s_in + ((2 * wv) * kIW + lp) * kPixStride + lg * 16;
    const unsigned char* pw = s_w + lane * 16;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        half8 px[4], wt[NB];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
          px[mb] = *reinterpret_cast<const half8*>(pin + (((mb >> 1) + ky) * kIW + (mb & 1) * 16 + kx) * kPixStride + hf * 64);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) wt[nb] = *reinterpret_cast<const half8*>(pw + ((2 * tap + hf) * NB + nb) * 1024);
#pragma unroll
        for (int mb = 0; mb < 4; ++mb)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[nb], px[mb], acc[mb][nb], 0, 0, 0);
      }
    }

    // epilogue: lane holds channels 16 nb + 4 lg + r, r = 0 .. 3, of its pixel of every block
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      const int gy = cy0 + 2 * wv + (mb >> 1), gx = cx0 + (mb & 1) * 16 + lp;
      if (gy >= cur.h || gx >= cur.w) continue;
      if constexpr (S == 0) {
        _Float16* yo = y + (cur.act_off + (int64_t)gy * cur.w + gx) * 64 + lg * 4;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          half4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = acc[mb][nb][r] + s_b[nb * 16 + lg * 4 + r];
            o[r] = (_Float16)(v >= 0.f ? v : s_a[nb * 16 + lg * 4 + r] * v);
          }
          *reinterpret_cast<half4*>(yo + nb * 16) = o;
        }
      } else {
        if (gy < cur.keep0 || gy >= cur.keep0 + cur.keepn) continue;
        const uint8_t* sp = src + cur.src_off + ((int64_t)gy * cur.w + gx) * 3;
        const int64_t pitch = (int64_t)3 * S * cur.w;
        bool bad = false;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ch = nb * 16 + lg * 4 + r;              // = c S^2 + dy S + dx
            const int c = ch / (S * S), dy = (ch / S) % S, dx = ch % S;
            if (c < 3) {
              const float v = acc[mb][nb][r] + s_b[ch] + (float)sp[c] / 255.f;
              const bool fin = isfinite(v);
              bad = bad || !fin;
              const int64_t o = cur.out_off + (int64_t)(S * (gy - cur.keep0) + dy) * pitch + (int64_t)(S * gx + dx) * 3 + c;
              out[o] = fin ? (uint8_t)rintf(255.f * fminf(fmaxf(v, 0.f), 1.f)) : (uint8_t)0;
              if (out_f32) out_f32[o] = v;
            }
          }
        }
        if (bad) atomicOr(info + cur.slot, VSP_SR_NONFINITE);
      }
    }
    if (next >= ntiles) break;
    tile = next;
  }
}

constexpr int64_t kTwoGiB = (int64_t)1 << 31;
constexpr int conv_lds(int NB) { return kInBytes + kSteps * NB * 1024 + 2 * NB * 16 * 4; }

// The checks every entry makes on its item table before it launches -> VSP_OK and the group's tile count
int check_items(const char* what, const vsp_sr_item* items, int n, int64_t src_bytes, int64_t act_bytes, int64_t out_bytes, int scale,
                int n_info, int64_t* ntiles) {
  int64_t tiles = 0;
  for (int i = 0; i < n; ++i) {
    const vsp_sr_item& it = items[i];
    VSP_REQUIRE(it.h >= 1 && it.w >= 1, "%s: item %d: photo %d x %d", what, i, it.h, it.w);
    const int64_t px = (int64_t)it.h * it.w;
    VSP_REQUIRE(it.act_off >= 0 && (it.act_off + px) * 128 <= act_bytes, "%s: item %d: activation outside its buffer", what, i);
    VSP_REQUIRE(src_bytes < 0 || (it.src_off >= 0 && it.src_off + 3 * px <= src_bytes), "%s: item %d: bytes outside src", what, i);
    VSP_REQUIRE(it.tile0 == tiles, "%s: item %d: tile0 %d, expected %lld", what, i, it.tile0, (long long)tiles);
    if (scale) {
      VSP_REQUIRE(it.keep0 >= 0 && it.keepn >= 1 && (int64_t)it.keep0 + it.keepn <= it.h, "%s: item %d: rows %d..%d of %d", what, i, it.keep0,
                  it.keep0 + it.keepn - 1, it.h);
      VSP_REQUIRE(it.out_off >= 0 && it.out_off + (int64_t)3 * scale * scale * it.keepn * it.w <= out_bytes, "%s: item %d: bytes outside out",
                  what, i);
      VSP_REQUIRE(it.slot >= 0 && it.slot < n_info, "%s: item %d: slot %d outside 0..%d", what, i, it.slot, n_info - 1);
    }
    tiles += (int64_t)((it.h + kTH - 1) / kTH) * ((it.w + kTW - 1) / kTW);
    VSP_REQUIRE(tiles < kTwoGiB, "%s: more than 2^31 tiles", what);
  }
  *ntiles = tiles;
  return VSP_OK;
}

template <int NB, int S>
int launch_conv(const char* what, _Float16* y, uint8_t* out, float* out_f32, int32_t* info, const _Float16* x, const uint8_t* src,
                const vsp_sr_item* items_dev, int n, int64_t ntiles, const void* wimg, const float* b, const float* slope,
                vsp_stream_t stream) {
  static vsp::LdsAttrOnce once;
  const void* fn = reinterpret_cast<const void*>(&sr_conv_kernel<NB, S>);
  if (int rc = once.ensure(fn, conv_lds(NB), what)) return rc;
  const int grid = (int)(ntiles < vsp::kNumCU ? ntiles : vsp::kNumCU);
  sr_conv_kernel<NB, S><<<grid, 256, conv_lds(NB), vsp::as_stream(stream)>>>(y, out, out_f32, info, x, src, items_dev, n, (int)ntiles,
                                                                             reinterpret_cast<const uint4*>(wimg), b, slope);
  return vsp::check_launch(what);
}

}  // namespace

extern "C" {

int vsp_sr_head_u8(void* y, size_t act_bytes, const uint8_t* src, size_t src_bytes, const vsp_sr_item* items, const vsp_sr_item* items_dev,
                   int n, const float* w, const float* b, const float* slope, vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && n <= VSP_SR_MAX_ITEMS, "sr_head: %d items (0..%d)", n, VSP_SR_MAX_ITEMS);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(y && src && items && items_dev && w && b && slope, "sr_head: null pointer");
  VSP_REQUIRE(vsp::aligned16(y), "sr_head: the activation buffer must be 16-byte aligned");
  if ((int64_t)act_bytes >= kTwoGiB || (int64_t)src_bytes >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "sr_head: a tensor of 2 GiB or more");
  int64_t ntiles = 0;
  if (int rc = check_items("sr_head", items, n, (int64_t)src_bytes, (int64_t)act_bytes, 0, 0, 0, &ntiles)) return rc;
  sr_head_kernel<<<(int)ntiles, 256, 0, vsp::as_stream(stream)>>>(static_cast<_Float16*>(y), src, items_dev, n, w, b, slope);
  return vsp::check_launch("sr_head");
}

int vsp_sr_body_f16(void* y, const void* x, size_t act_bytes, const vsp_sr_item* items, const vsp_sr_item* items_dev, int n,
                    const void* w_img, const float* b, const float* slope, vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && n <= VSP_SR_MAX_ITEMS, "sr_body: %d items (0..%d)", n, VSP_SR_MAX_ITEMS);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(y && x && items && items_dev && w_img && b && slope, "sr_body: null pointer");
  VSP_REQUIRE(y != x, "sr_body: in place");
  VSP_REQUIRE(vsp::aligned16(y) && vsp::aligned16(x) && vsp::aligned16(w_img), "sr_body: buffers must be 16-byte aligned");
  if ((int64_t)act_bytes >= kTwoGiB) return vsp::fail(VSP_ENOTSUP, "sr_body: a tensor of 2 GiB or more");
  int64_t ntiles = 0;
  if (int rc = check_items("sr_body", items, n, -1, (int64_t)act_bytes, 0, 0, 0, &ntiles)) return rc;
  return launch_conv<4, 0>("sr_body", static_cast<_Float16*>(y), nullptr, nullptr, nullptr, static_cast<const _Float16*>(x), nullptr, items_dev,
                           n, ntiles, w_img, b, slope, stream);
}

int vsp_sr_tail_u8(uint8_t* out, size_t out_bytes, float* out_f32, int32_t* info, int n_info, const void* x, size_t act_bytes,
                   const uint8_t* src, size_t src_bytes, const vsp_sr_item* items, const vsp_sr_item* items_dev, int n, const void* w_img,
                   const float* b, int scale, vsp_stream_t stream) {
  VSP_REQUIRE(scale == 2 || scale == 4, "sr_tail: scale %d (2 or 4)", scale);
  VSP_REQUIRE(n >= 0 && n <= VSP_SR_MAX_ITEMS, "sr_tail: %d items (0..%d)", n, VSP_SR_MAX_ITEMS);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(out && info && x && src && items && items_dev && w_img && b, "sr_tail: null pointer");
  VSP_REQUIRE(n_info >= 1, "sr_tail: %d info words", n_info);
  VSP_REQUIRE(vsp::aligned16(x) && vsp::aligned16(w_img), "sr_tail: buffers must be 16-byte aligned");
  if ((int64_t)act_bytes >= kTwoGiB || (int64_t)src_bytes >= kTwoGiB || (int64_t)out_bytes >= kTwoGiB ||
      (out_f32 && (int64_t)out_bytes * 4 >= kTwoGiB))
    return vsp::fail(VSP_ENOTSUP, "sr_tail: a tensor of 2 GiB or more");
  int64_t ntiles = 0;
  if (int rc = check_items("sr_tail", items, n, (int64_t)src_bytes, (int64_t)act_bytes, (int64_t)out_bytes, scale, n_info, &ntiles)) return rc;
  const _Float16* xs = static_cast<const _Float16*>(x);
  if (scale == 2)
    return launch_conv<1, 2>("sr_tail", nullptr, out, out_f32, info, xs, src, items_dev, n, ntiles, w_img, b, nullptr, stream);
  return launch_conv<3, 4>("sr_tail", nullptr, out, out_f32, info, xs, src, items_dev, n, ntiles, w_img, b, nullptr, stream);
}

}  // extern "C"

// Pillow-exact 8-bit LANCZOS resize + crop of a ragged batch of RGB images for gfx950 (definitions: include/vspbfr_hip.h).
//
// Pillow's own structure, two launches over the whole batch:
//   horizontal  one workgroup per (item, source row the crop's vertical pass reads): the row segment the crop's columns read is staged
//               into LDS with aligned dword loads over the byte stream (a packed RGB row is 3 * sw bytes and is not dword aligned in
//               general: the LDS copy keeps the misalignment of the global segment, so a global dword is an LDS dword; only dwords that
//               straddle the ends of the source buffer are assembled from bytes); one thread per output column, three channels, writes
//               the uint8 intermediate row (row stride rounded up to dwords) into `work`.
//   vertical    one workgroup per (item, output row): a thread owns 4 consecutive bytes of the row, reads one aligned dword per tap from
//               the intermediate rows and writes the uint8 NHWC bytes and / or the normalised fp32 NCHW values.
// An item flagged VSP_RESAMPLE_COPY skips the horizontal pass; the vertical kernel copies its source bytes.
//
// vsp_lanczos_resize_ragged_u8 runs the same two bodies with a window (W_i, H_i) and a byte offset per item (vsp_resample_dst): the grids
// span the largest row count of the batch and a workgroup whose item has no such row returns.  The uniform kernels keep their signatures
// and are front ends of the bodies too.
//
// Numerics: 32-bit integer accumulation from 2^21, arithmetic shift by 22, clamp to 0..255 -- ImagingResampleHorizontal_8bpc /
// ImagingResampleVertical_8bpc.  No floating point before the final normalisation, which is three separately rounded fp32
// operations (torch's ToTensor + Normalize(0.5, 0.5) on the host): __fdiv_rn / __fsub_rn cannot be contracted or approximated.
//
// Bounds: the entry checks every item on the host (sizes, crop, taps, every offset against the buffer sizes it is given) before it
// launches; the kernels clamp what they read from the coefficient tables (xmin / count) to the staged segment / rows, so a wrong
// table gives wrong pixels, not a wild read.
#include "vsp_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kSegDwords = VSP_RESAMPLE_MAX_SIDE * 3 / 4 + 2;   // a whole source row + 3 bytes of misalignment, in dwords

__host__ __device__ inline int work_stride(int W) { return (3 * W + 3) / 4 * 4; }

__device__ __forceinline__ int clip8(int acc) {
  const int v = acc >> VSP_RESAMPLE_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// source row row0 + blockIdx.x of item `it` -> row blockIdx.x of its intermediate image, for a window W columns wide
__device__ __forceinline__ void horizontal_row(uint32_t* seg, uint8_t* work, const uint8_t* src, int64_t src_bytes, const int32_t* coef,
                                               const vsp_resample_item& it, int W) {
  const int nrows = it.row1 - it.row0 + 1;
  if ((it.flags & VSP_RESAMPLE_COPY) || (int)blockIdx.x >= nrows) return;
  const int tid = threadIdx.x;
  const int32_t* xmin = coef + it.hco;
  const int32_t* count = xmin + it.nw;
  const int32_t* taps = count + it.nw;   // taps[k * nw + x]
  // columns of the (possibly mirrored) source that the crop window reads: [c0, c1)
  int c0 = xmin[it.x0], c1 = xmin[it.x0 + W - 1] + count[it.x0 + W - 1];
  c0 = max(0, min(c0, it.sw));
  c1 = max(c0, min(c1, it.sw));
  const int npix = c1 - c0;
  const bool flip = it.flags & VSP_RESAMPLE_FLIP;
  const int s0 = flip ? it.sw - c1 : c0;   // first stored column of the segment
  const int row = it.row0 + (int)blockIdx.x;
  const uintptr_t lo = (uintptr_t)src, hi = lo + (uintptr_t)src_bytes;
  const uintptr_t A = lo + (uintptr_t)(it.src_off + ((int64_t)row * it.sw + s0) * 3);
  const int L = npix * 3;
  const int mis = (int)(A & 3);
  for (int d = tid; d * 4 < mis + L; d += kThreads) {
    const uintptr_t p = (A & ~(uintptr_t)3) + 4u * (uintptr_t)d;
    uint32_t v = 0;
    if (p >= lo && p + 4 <= hi) {
      v = *reinterpret_cast<const uint32_t*>(p);
    } else {   // the first / last dword of the buffer: only the bytes that belong to it
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k >= lo && p + k < hi) v |= (uint32_t)(*reinterpret_cast<const uint8_t*>(p + k)) << (8 * k);
    }
    seg[d] = v;
  }
  __syncthreads();
  const uint8_t* ls = reinterpret_cast<const uint8_t*>(seg) + mis;
  uint8_t* out = work + it.work_off + (int64_t)blockIdx.x * work_stride(W);
  for (int x = tid; x < W; x += kThreads) {
    const int ox = it.x0 + x;
    int lo_x = xmin[ox], n = count[ox];
    lo_x = max(lo_x, c0);
    n = max(0, min(min(n, it.hk), c1 - lo_x));
    int a0 = 1 << (VSP_RESAMPLE_PRECISION_BITS - 1), a1 = a0, a2 = a0;
    // pixel j of the mirrored row sits at stored column sw - 1 - j, i.e. at segment pixel (c1 - 1 - j) when flipped, (j - c0) when not
    const uint8_t* p = ls + 3 * (flip ? c1 - 1 - lo_x : lo_x - c0);
    const int step = flip ? -3 : 3;
    for (int k = 0; k < n; ++k) {
      const int w = taps[(int64_t)k * it.nw + ox];
      a0 += (int)p[0] * w;
      a1 += (int)p[1] * w;
      a2 += (int)p[2] * w;
      p += step;
    }
    out[3 * x + 0] = (uint8_t)clip8(a0);
    out[3 * x + 1] = (uint8_t)clip8(a1);
    out[3 * x + 2] = (uint8_t)clip8(a2);
  }
}

__global__ __launch_bounds__(kThreads) void lanczos_horizontal_kernel(uint8_t* work, const uint8_t* src, int64_t src_bytes,
                                                                       const int32_t* coef, const vsp_resample_item* items, int W) {
  __shared__ uint32_t seg[kSegDwords];
  const vsp_resample_item it = items[blockIdx.y];
  horizontal_row(seg, work, src, src_bytes, coef, it, W);
}

__global__ __launch_bounds__(kThreads) void lanczos_horizontal_ragged_kernel(uint8_t* work, const uint8_t* src, int64_t src_bytes,
                                                                              const int32_t* coef, const vsp_resample_item* items,
                                                                              const vsp_resample_dst* dst) {
  __shared__ uint32_t seg[kSegDwords];
  const vsp_resample_item it = items[blockIdx.y];
  horizontal_row(seg, work, src, src_bytes, coef, it, dst[blockIdx.y].W);
}

// output row y of item `it`, W columns wide: o8 / of point at the row's first uint8 / fp32 value (or are null), `plane` is the distance
// of the fp32 channel planes
__device__ __forceinline__ void vertical_row(uint8_t* o8, float* of, int64_t plane, const uint8_t* work, const uint8_t* src,
                                             const int32_t* coef, const vsp_resample_item& it, int y, int W) {
  const int rowbytes = 3 * W;
  const bool copy = it.flags & VSP_RESAMPLE_COPY;
  const bool flip = it.flags & VSP_RESAMPLE_FLIP;
  int lo_y = 0, n = 0;
  const int32_t* taps = nullptr;
  const uint8_t* rows = nullptr;
  const int stride = work_stride(W);
  if (!copy) {
    const int32_t* ymin = coef + it.vco;
    const int32_t* count = ymin + it.nh;
    const int oy = it.y0 + y;
    taps = count + it.nh + oy;   // taps[k * nh]
    lo_y = max(ymin[oy], it.row0);
    n = max(0, min(min(count[oy], it.vk), it.row1 + 1 - lo_y));
    rows = work + it.work_off + (int64_t)(lo_y - it.row0) * stride;
  }
  for (int j0 = threadIdx.x * 4; j0 < rowbytes; j0 += kThreads * 4) {
    int v[4];
    if (copy) {
      const uint8_t* s = src + it.src_off + (int64_t)y * it.sw * 3;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = j0 + e;
        if (j < rowbytes) {
          const int x = j / 3, c = j - 3 * x;
          v[e] = s[3 * (flip ? it.sw - 1 - x : x) + c];
        } else {
          v[e] = 0;
        }
      }
    } else {
      int a[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = 1 << (VSP_RESAMPLE_PRECISION_BITS - 1);
      const uint8_t* p = rows + j0;   // work_off, stride and j0 are multiples of 4: aligned dwords
      for (int k = 0; k < n; ++k) {
        const uint32_t d = *reinterpret_cast<const uint32_t*>(p);
        const int w = taps[(int64_t)k * it.nh];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] += (int)((d >> (8 * e)) & 255u) * w;
        p += stride;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = clip8(a[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + e;
      if (j >= rowbytes) break;
      if (o8) o8[j] = (uint8_t)v[e];
      if (of) {
        const int x = j / 3, c = j - 3 * x;
        of[c * plane + x] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)v[e], 255.0f), 0.5f), 0.5f);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void lanczos_vertical_kernel(uint8_t* out_u8, float* out_f32, const uint8_t* work,
                                                                     const uint8_t* src, const int32_t* coef,
                                                                     const vsp_resample_item* items, int H, int W) {
  const vsp_resample_item it = items[blockIdx.y];
  const int y = blockIdx.x;
  const int rowbytes = 3 * W;
  const int64_t img = blockIdx.y;
  uint8_t* o8 = out_u8 ? out_u8 + (img * H + y) * rowbytes : nullptr;
  float* of = out_f32 ? out_f32 + img * 3 * H * W + (int64_t)y * W : nullptr;
  vertical_row(o8, of, (int64_t)H * W, work, src, coef, it, y, W);
}

__global__ __launch_bounds__(kThreads) void lanczos_vertical_ragged_kernel(uint8_t* out, const uint8_t* work, const uint8_t* src,
                                                                            const int32_t* coef, const vsp_resample_item* items,
                                                                            const vsp_resample_dst* dst) {
  const vsp_resample_dst d = dst[blockIdx.y];
  const int y = blockIdx.x;
  if (y >= d.H) return;
  const vsp_resample_item it = items[blockIdx.y];
  vertical_row(out + d.out_off + (int64_t)y * 3 * d.W, nullptr, 0, work, src, coef, it, y, d.W);
}

inline int ksize_of(int in_size, int out_size) {   // Resample.c precompute_coeffs: (int)ceil(support) * 2 + 1
  double fs = (double)in_size / (double)out_size;
  if (fs < 1.0) fs = 1.0;
  const double support = 3.0 * fs;
  int c = (int)support;
  if ((double)c < support) ++c;
  return c * 2 + 1;
}

// Every check of one item against its window (H, W) and the buffer sizes; *rows = the intermediate rows it needs (0 for a copy item).
int check_item(int i, const vsp_resample_item& it, int H, int W, size_t src_bytes, const int32_t* coef, size_t coef_ints, const uint8_t* work,
               size_t work_bytes, int* rows_out) {
  const int64_t stride = work_stride(W);
  *rows_out = 0;
  VSP_REQUIRE(it.sw > 0 && it.sh > 0 && it.nw > 0 && it.nh > 0, "lanczos_resize: item %d has a zero size", i);
  if (it.sw > VSP_RESAMPLE_MAX_SIDE || it.sh > VSP_RESAMPLE_MAX_SIDE || it.nw > VSP_RESAMPLE_MAX_SIDE || it.nh > VSP_RESAMPLE_MAX_SIDE)
    return vsp::fail(VSP_ENOTSUP, "lanczos_resize: item %d has a side above %d", i, VSP_RESAMPLE_MAX_SIDE);
  const bool copy = it.flags & VSP_RESAMPLE_COPY;
  const int hk = copy ? 0 : ksize_of(it.sw, it.nw), vk = copy ? 0 : ksize_of(it.sh, it.nh);
  if (hk > VSP_RESAMPLE_MAX_TAPS || vk > VSP_RESAMPLE_MAX_TAPS)
    return vsp::fail(VSP_ENOTSUP, "lanczos_resize: item %d needs %d x %d taps (reduction above 16x; at most %d)", i, hk, vk,
                     VSP_RESAMPLE_MAX_TAPS);
  VSP_REQUIRE(it.x0 >= 0 && it.y0 >= 0 && (int64_t)it.x0 + W <= it.nw && (int64_t)it.y0 + H <= it.nh,
              "lanczos_resize: item %d: crop %d x %d at (%d, %d) outside the resized %d x %d image", i, W, H, it.x0, it.y0, it.nw, it.nh);
  VSP_REQUIRE(it.src_off >= 0 && (uint64_t)it.src_off + 3ull * it.sw * it.sh <= (uint64_t)src_bytes,
              "lanczos_resize: item %d: source outside the %zu source bytes", i, src_bytes);
  if (copy) {
    VSP_REQUIRE(it.sw == W && it.sh == H && it.nw == W && it.nh == H, "lanczos_resize: item %d: a copy item must have the output size", i);
    return VSP_OK;
  }
  VSP_REQUIRE(it.hk == hk && it.vk == vk, "lanczos_resize: item %d: tap counts %d, %d do not match its sizes (%d, %d)", i, it.hk, it.vk, hk, vk);
  VSP_REQUIRE(coef && work, "lanczos_resize: null pointer");
  VSP_REQUIRE(it.hco >= 0 && (uint64_t)it.hco + (uint64_t)it.nw * (2 + hk) <= (uint64_t)coef_ints && it.vco >= 0 &&
                  (uint64_t)it.vco + (uint64_t)it.nh * (2 + vk) <= (uint64_t)coef_ints,
              "lanczos_resize: item %d: coefficient table outside the %zu coefficients", i, coef_ints);
  VSP_REQUIRE(it.row0 >= 0 && it.row0 <= it.row1 && it.row1 < it.sh, "lanczos_resize: item %d: source rows %d..%d", i, it.row0, it.row1);
  const int rows = it.row1 - it.row0 + 1;
  VSP_REQUIRE(it.work_off >= 0 && (it.work_off & 3) == 0 && (uint64_t)it.work_off + (uint64_t)rows * stride <= (uint64_t)work_bytes,
              "lanczos_resize: item %d: rows outside the %zu work bytes", i, work_bytes);
  *rows_out = rows;
  return VSP_OK;
}

}  // namespace

extern "C" {

size_t vsp_lanczos_work_bytes(int rows, int W) {
  if (rows <= 0 || W <= 0 || W > VSP_RESAMPLE_MAX_SIDE || rows > VSP_RESAMPLE_MAX_SIDE) return 0;
  return (size_t)rows * (size_t)work_stride(W);
}

int vsp_lanczos_resize_u8(uint8_t* out_u8, float* out_f32, const uint8_t* src, size_t src_bytes, const int32_t* coef, size_t coef_ints,
                          uint8_t* work, size_t work_bytes, const vsp_resample_item* items, const vsp_resample_item* items_dev, int n,
                          int H, int W, vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && n <= VSP_RESAMPLE_MAX_ITEMS, "lanczos_resize: 0..%d items (got %d)", VSP_RESAMPLE_MAX_ITEMS, n);
  VSP_REQUIRE(H > 0 && W > 0, "lanczos_resize: output size %d x %d", H, W);
  if (H > VSP_RESAMPLE_MAX_SIDE || W > VSP_RESAMPLE_MAX_SIDE)
    return vsp::fail(VSP_ENOTSUP, "lanczos_resize: output side above %d", VSP_RESAMPLE_MAX_SIDE);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(out_u8 || out_f32, "lanczos_resize: null pointer (no output)");
  VSP_REQUIRE(src && items && items_dev, "lanczos_resize: null pointer");
  VSP_REQUIRE((reinterpret_cast<uintptr_t>(work) & 3u) == 0 && (reinterpret_cast<uintptr_t>(coef) & 3u) == 0,
              "lanczos_resize: work and coef must be 4-byte aligned");
  int max_rows = 0;
  for (int i = 0; i < n; ++i) {
    int rows = 0;
    const int rc = check_item(i, items[i], H, W, src_bytes, coef, coef_ints, work, work_bytes, &rows);
    if (rc != VSP_OK) return rc;
    max_rows = rows > max_rows ? rows : max_rows;
  }
  hipStream_t s = vsp::as_stream(stream);
  if (max_rows > 0) {
    lanczos_horizontal_kernel<<<dim3((unsigned)max_rows, (unsigned)n), kThreads, 0, s>>>(work, src, (int64_t)src_bytes, coef, items_dev, W);
    int rc = vsp::check_launch("lanczos_horizontal");
    if (rc != VSP_OK) return rc;
  }
  lanczos_vertical_kernel<<<dim3((unsigned)H, (unsigned)n), kThreads, 0, s>>>(out_u8, out_f32, work, src, coef, items_dev, H, W);
  return vsp::check_launch("lanczos_vertical");
}

int vsp_lanczos_resize_ragged_u8(uint8_t* out, size_t out_bytes, const uint8_t* src, size_t src_bytes, const int32_t* coef, size_t coef_ints,
                                 uint8_t* work, size_t work_bytes, const vsp_resample_item* items, const vsp_resample_item* items_dev,
                                 const vsp_resample_dst* dst, const vsp_resample_dst* dst_dev, int n, vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && n <= VSP_RESAMPLE_MAX_ITEMS, "lanczos_resize: 0..%d items (got %d)", VSP_RESAMPLE_MAX_ITEMS, n);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(out, "lanczos_resize: null pointer (no output)");
  VSP_REQUIRE(src && items && items_dev && dst && dst_dev, "lanczos_resize: null pointer");
  VSP_REQUIRE((reinterpret_cast<uintptr_t>(work) & 3u) == 0 && (reinterpret_cast<uintptr_t>(coef) & 3u) == 0,
              "lanczos_resize: work and coef must be 4-byte aligned");
  int max_rows = 0, max_h = 0;
  uint64_t end = 0;   // first byte behind the destinations so far: they ascend, so one running end finds every overlap
  for (int i = 0; i < n; ++i) {
    const vsp_resample_dst& d = dst[i];
    VSP_REQUIRE(d.H > 0 && d.W > 0, "lanczos_resize: item %d: output size %d x %d", i, d.H, d.W);
    if (d.H > VSP_RESAMPLE_MAX_SIDE || d.W > VSP_RESAMPLE_MAX_SIDE)
      return vsp::fail(VSP_ENOTSUP, "lanczos_resize: item %d: output side above %d", i, VSP_RESAMPLE_MAX_SIDE);
    const uint64_t bytes = 3ull * (uint64_t)d.W * (uint64_t)d.H;
    VSP_REQUIRE(d.out_off >= 0 && (uint64_t)d.out_off <= (uint64_t)out_bytes && bytes <= (uint64_t)out_bytes - (uint64_t)d.out_off,
                "lanczos_resize: item %d: destination outside the %zu output bytes", i, out_bytes);
    VSP_REQUIRE((uint64_t)d.out_off >= end, "lanczos_resize: item %d: destination descends or overlaps the one before", i);
    end = (uint64_t)d.out_off + bytes;
    int rows = 0;
    const int rc = check_item(i, items[i], d.H, d.W, src_bytes, coef, coef_ints, work, work_bytes, &rows);
    if (rc != VSP_OK) return rc;
    max_rows = rows > max_rows ? rows : max_rows;
    max_h = d.H > max_h ? d.H : max_h;
  }
  hipStream_t s = vsp::as_stream(stream);
  if (max_rows > 0) {
    lanczos_horizontal_ragged_kernel<<<dim3((unsigned)max_rows, (unsigned)n), kThreads, 0, s>>>(work, src, (int64_t)src_bytes, coef,
                                                                                                 items_dev, dst_dev);
    int rc = vsp::check_launch("lanczos_horizontal_ragged");
    if (rc != VSP_OK) return rc;
  }
  lanczos_vertical_ragged_kernel<<<dim3((unsigned)max_h, (unsigned)n), kThreads, 0, s>>>(out, work, src, coef, items_dev, dst_dev);
  return vsp::check_launch("lanczos_vertical_ragged");
}

}  // extern "C"

// NIQE features of uint8 RGB images for gfx950 (Mittal et al. 2013, as everybody runs it; definition: include/vspbfr_hip.h).
//
// One 256-thread workgroup owns one 96 x 96 block of one image and computes BOTH scales of it from one staged luma region in a
// single launch: the block plus a halo of 9 (scale 2's pixel i reads input rows 2i-3 .. 2i+4, and its 7 x 7 Gaussian reads image-2
// pixels -3 .. +50 of the block: input rows -9 .. +104, 114 rows).  Three boundary rules meet here and each is applied where its
// operator reads, never baked into another one's data:
//   * the staged luma is gathered with SYMMETRIC REFLECTION about the cropped image (the bicubic downscale's rule);
//   * scale 1's Gaussian CLAMPS its cropped-image coordinate and then indexes the stage (always a true pixel);
//   * scale 2's Gaussian CLAMPS its image-2 coordinate and then indexes the 54 x 54 image-2 patch.
//
// Numerics.  Both images are integers: Y, and I2 = sum taps * taps * Y (|I2| < 2^25, int32) = 65536 x the half-size image.  Everything
// local is shift invariant, so the block subtracts its own rounded mean luma c first, exactly and in integers (Y - c, I2 - 65536 c),
// and only then goes to fp32: the accumulated squares have the size of the block's contrast, not of its brightness, and a flat
// block gives exact zeros.  mu' = G * x', var = G * x'^2 - mu'^2 (one fma), sigma = sqrt|var|, MSCN = (x' - mu') / (sigma + 1), with
// IEEE division and square root.  The products and the six raw moments per map are formed and reduced in float64 in a fixed order.
//
// Exact zeros: a sample equal to zero lies on neither side (n-, n+) and counts in the totals.  A side without samples gives
// 0 / 0 = NaN for its deviation, the block's row of features holds NaN, and the score drops the row.
//
// Determinism: per thread in a fixed stride, a fixed butterfly per wave, the four waves in order.  A block never looks at another
// block or at the batch: image i gets the same bits in any batch, at any position, on any launch.
//
// LDS: 13224 (stage, bytes) + 36864 (MSCN; before that the downscale's row pass and the image-2 patch) + 23040 (row sums of one
// 24-row strip) + 1 KiB of reduction slots = 74 KiB: two workgroups per CU.
#include "vsp_common.h"
#include <cmath>

namespace {

constexpr int kBlk = 96;                 // block side at scale 1
constexpr int kStage = 114;              // staged luma rows / columns: block + 9 on every side
constexpr int kStageStride = 116;
constexpr int kBlk2 = 48;                // block side at scale 2
constexpr int kPatch2 = 54;              // image-2 patch: block + 3 on every side
constexpr int kPatch2Stride = 55;
constexpr int kStrip = 24;               // scale-1 rows per strip of the separable Gaussian
constexpr int kThreads = 256;
constexpr int kGam = 9801;               // gamma = 0.2, 0.201, ... 10
constexpr int kMaps = 5, kMom = 6;

struct NiqeTaps { float g[7]; };

__device__ __forceinline__ int reflect_sym(int v, int n) { return v < 0 ? -1 - v : (v >= n ? 2 * n - 1 - v : v); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// BT.601 luma of 8-bit RGB, exactly: round-half-even(16 + (65.481 R + 128.553 G + 24.966 B) / 255)
__device__ __forceinline__ int luma601(int r, int g, int b) {
  const int n = 65481 * r + 128553 * g + 24966 * b;   // <= 55 845 000
  int q = n / 255000;
  const int rem2 = 2 * (n - q * 255000);
  q += (rem2 > 255000 || (rem2 == 255000 && (q & 1))) ? 1 : 0;
  return 16 + q;
}

// scale 1: x' = Y - c at block-relative (rr, cc), the cropped-image coordinate clamped (edge replicate)
struct Src1 {
  const uint8_t* y; int oy, ox, Hc, Wc, c;   // oy, ox: cropped-image coordinates of the block's first pixel
  __device__ __forceinline__ int row(int rr) const { return clampi(oy + rr, 0, Hc - 1) - oy + 9; }
  __device__ __forceinline__ int col(int cc) const { return clampi(ox + cc, 0, Wc - 1) - ox + 9; }
  __device__ __forceinline__ float at(int lr, int lc) const { return (float)((int)y[lr * kStageStride + lc] - c); }
};
// scale 2: the image-2 patch, its own coordinate clamped
struct Src2 {
  const float* p; int oy, ox, Hc, Wc;
  __device__ __forceinline__ int row(int rr) const { return clampi(oy + rr, 0, Hc - 1) - oy + 3; }
  __device__ __forceinline__ int col(int cc) const { return clampi(ox + cc, 0, Wc - 1) - ox + 3; }
  __device__ __forceinline__ float at(int lr, int lc) const { return p[lr * kPatch2Stride + lc]; }
};

// MSCN of output rows row0 .. row0 + ROWS - 1 of an N x N block into mscn; returns this thread's sum of sigma (double)
template <int N, int ROWS, typename Src>
__device__ __forceinline__ double mscn_strip(float* mscn, float* hbuf, const Src& src, int row0, const NiqeTaps& t, int tid) {
  constexpr int HR = ROWS + 6;
  float* h1 = hbuf;
  float* h2 = hbuf + HR * N;
  // horizontal sums of x' and x'^2: 4 adjacent positions per item share their 10 inputs
  for (int it = tid; it < HR * (N / 4); it += kThreads) {
    const int hr = it / (N / 4), x0 = (it - hr * (N / 4)) * 4;
    const int lr = src.row(row0 + hr - 3);
    float v[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) v[k] = src.at(lr, src.col(x0 + k - 3));
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const float x = v[o + k];
        s1 = fmaf(t.g[k], x, s1);
        s2 = fmaf(t.g[k], x * x, s2);
      }
      h1[hr * N + x0 + o] = s1;
      h2[hr * N + x0 + o] = s2;
    }
  }
  __syncthreads();
  // vertical sums and the normalisation: 4 positions below each other per item share their 10 rows
  double sharp = 0.0;
  for (int it = tid; it < (ROWS / 4) * N; it += kThreads) {
    const int g = it / N, j = it - g * N;
    float a1[10], a2[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) {
      a1[k] = h1[(4 * g + k) * N + j];
      a2[k] = h2[(4 * g + k) * N + j];
    }
    const int lc = src.col(j);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float mu = 0.f, m2 = 0.f;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        mu = fmaf(t.g[k], a1[o + k], mu);
        m2 = fmaf(t.g[k], a2[o + k], m2);
      }
      const float sd = sqrtf(fabsf(fmaf(-mu, mu, m2)));
      const int r = row0 + 4 * g + o;
      const float x = src.at(src.row(r), lc);
      mscn[r * N + j] = (x - mu) / (sd + 1.f);
      sharp += (double)sd;
    }
  }
  __syncthreads();
  return sharp;
}

// The six raw moments of the five maps of an N x N MSCN block (the block and its products with four circular shifts), reduced
// over the workgroup in a fixed order, then the float64 finish: 18 features.
template <int N>
__device__ __forceinline__ void moments_features(double* feat18, double* mom30, const float* mscn, double (*red)[kMaps * kMom],
                                                 const double* table, int tid) {
  double acc[kMaps][kMom];
#pragma unroll
  for (int m = 0; m < kMaps; ++m)
#pragma unroll
    for (int k = 0; k < kMom; ++k) acc[m][k] = 0.0;
  for (int p = tid; p < N * N; p += kThreads) {
    const int i = p / N, j = p - i * N;
    const int im = i == 0 ? N - 1 : i - 1, jm = j == 0 ? N - 1 : j - 1, jp = j == N - 1 ? 0 : j + 1;
    const double a = (double)mscn[p];
    double v[kMaps];
    v[0] = a;
    v[1] = a * (double)mscn[i * N + jm];     // roll (0, 1)
    v[2] = a * (double)mscn[im * N + j];     // roll (1, 0)
    v[3] = a * (double)mscn[im * N + jm];    // roll (1, 1)
    v[4] = a * (double)mscn[im * N + jp];    // roll (1, -1)
#pragma unroll
    for (int m = 0; m < kMaps; ++m) {
      const double x = v[m], xx = x * x;
      const bool neg = x < 0.0, pos = x > 0.0;
      acc[m][0] += neg ? 1.0 : 0.0;
      acc[m][1] += neg ? xx : 0.0;
      acc[m][2] += pos ? 1.0 : 0.0;
      acc[m][3] += pos ? xx : 0.0;
      acc[m][4] += fabs(x);
      acc[m][5] += xx;
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int m = 0; m < kMaps; ++m)
#pragma unroll
    for (int k = 0; k < kMom; ++k) {
      const double s = wave_sum_d(acc[m][k]);
      if (lane == 0) red[wave][m * kMom + k] = s;
    }
  __syncthreads();
  if (tid < kMaps) {
    const int m = tid;
    double q[kMom];
#pragma unroll
    for (int k = 0; k < kMom; ++k) {
      q[k] = ((red[0][m * kMom + k] + red[1][m * kMom + k]) + red[2][m * kMom + k]) + red[3][m * kMom + k];
      if (mom30) mom30[m * kMom + k] = q[k];
    }
    const double n = (double)(N * N);
    const double ls = sqrt(q[1] / q[0]), rs = sqrt(q[3] / q[2]);
    const double gh = ls / rs;
    const double ma = q[4] / n;
    const double rhat = ma * ma / (q[5] / n);
    const double g2 = gh * gh + 1.0;
    const double rnorm = rhat * (gh * gh * gh + 1.0) * (gh + 1.0) / (g2 * g2);
    // first minimum of (r(gamma) - rnorm)^2 over the increasing table: the neighbours of the crossing; NaN -> index 0
    const double* rt = table + kGam;
    int idx = 0;
    if (rnorm == rnorm) {
      int lo = 0, hi = kGam;   // first index with rt[idx] >= rnorm
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rt[mid] < rnorm) lo = mid + 1; else hi = mid;
      }
      idx = lo >= kGam ? kGam - 1 : lo;
      if (idx > 0) {
        const double d0 = rt[idx - 1] - rnorm, d1 = rt[idx] - rnorm;
        if (d0 * d0 <= d1 * d1) idx -= 1;
      }
    }
    const double alpha = table[idx], bs = table[2 * kGam + idx], mr = table[3 * kGam + idx];
    const double bl = ls * bs, br = rs * bs;
    if (m == 0) {
      feat18[0] = alpha;
      feat18[1] = (bl + br) / 2.0;
    } else {
      double* f = feat18 + 2 + 4 * (m - 1);
      f[0] = alpha;
      f[1] = (br - bl) * mr;
      f[2] = bl;
      f[3] = br;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void niqe_block_kernel(double* features, double* moments, float* sharpness, const uint8_t* img,
                                                                   int H, int W, int cb, int nbx, int nby, const double* table, NiqeTaps t) {
  __shared__ uint8_t ybuf[kStage * kStageStride];
  __shared__ float mbuf[kBlk * kBlk];
  __shared__ float hbuf[2 * (kStrip + 6) * kBlk];
  __shared__ double red[4][kMaps * kMom];
  __shared__ unsigned int redu[4];
  static_assert(kPatch2 * kStage + kPatch2 * kPatch2Stride <= kBlk * kBlk, "row pass + image-2 patch must fit the MSCN buffer");
  static_assert(2 * (kBlk2 + 6) * kBlk2 <= 2 * (kStrip + 6) * kBlk, "scale-2 row sums must fit the strip buffer");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
  const int Hc = nby * kBlk, Wc = nbx * kBlk;
  const int oy = by * kBlk, ox = bx * kBlk;
  const int64_t blk = (int64_t)b * (nbx * nby) + blockIdx.x;

  // ---- stage the luma of the block + 9, reflected about the cropped image; the block's own sum on the way
  unsigned int ysum = 0;
  for (int p = tid; p < kStage * kStage; p += kThreads) {
    const int r = p / kStage, q = p - r * kStage;
    const int yy = reflect_sym(oy - 9 + r, Hc), xx = reflect_sym(ox - 9 + q, Wc);
    const uint8_t* px = img + (((int64_t)b * H + (cb + yy)) * W + (cb + xx)) * 3;
    const int y = luma601(px[0], px[1], px[2]);
    ybuf[r * kStageStride + q] = (uint8_t)y;
    if (r >= 9 && r < 9 + kBlk && q >= 9 && q < 9 + kBlk) ysum += (unsigned int)y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ysum += __shfl_xor(ysum, o, 64);
  if (lane == 0) redu[wave] = ysum;
  __syncthreads();
  const int c = (int)((redu[0] + redu[1] + redu[2] + redu[3] + (kBlk * kBlk) / 2) / (kBlk * kBlk));

  // ---- scale 2: bicubic antialiased half-size image, 8 taps / 256 at stride 2, rows then columns, in integers
  {
    int* T = reinterpret_cast<int*>(mbuf);                  // [54][114]
    float* patch = mbuf + kPatch2 * kStage;                  // [54][55]
    for (int p = tid; p < kPatch2 * kStage; p += kThreads) {
      const int i = p / kStage, q = p - i * kStage;
      const uint8_t* col = ybuf + (2 * i) * kStageStride + q;
      const int s = -3 * ((int)col[0] + (int)col[7 * kStageStride]) - 9 * ((int)col[kStageStride] + (int)col[6 * kStageStride]) +
                    29 * ((int)col[2 * kStageStride] + (int)col[5 * kStageStride]) + 111 * ((int)col[3 * kStageStride] + (int)col[4 * kStageStride]);
      T[p] = s;
    }
    __syncthreads();
    for (int p = tid; p < kPatch2 * kPatch2; p += kThreads) {
      const int i = p / kPatch2, j = p - i * kPatch2;
      const int* row = T + i * kStage + 2 * j;
      const int s = -3 * (row[0] + row[7]) - 9 * (row[1] + row[6]) + 29 * (row[2] + row[5]) + 111 * (row[3] + row[4]);
      patch[i * kPatch2Stride + j] = (float)(s - c * 65536) * (1.f / 65536.f);
    }
    __syncthreads();
    const Src2 s2{patch, by * kBlk2, bx * kBlk2, Hc / 2, Wc / 2};
    mscn_strip<kBlk2, kBlk2>(mbuf, hbuf, s2, 0, t, tid);     // MSCN over the dead row pass, the patch stays intact
    moments_features<kBlk2>(features + blk * 36 + 18, moments ? moments + (blk * 2 + 1) * (kMaps * kMom) : nullptr, mbuf, red, table, tid);
  }

  // ---- scale 1, in strips of 24 rows
  {
    const Src1 s1{ybuf, oy, ox, Hc, Wc, c};
    double sharp = 0.0;
#pragma unroll 1
    for (int st = 0; st < kBlk / kStrip; ++st) sharp += mscn_strip<kBlk, kStrip>(mbuf, hbuf, s1, st * kStrip, t, tid);
    sharp = wave_sum_d(sharp);
    if (lane == 0) red[wave][0] = sharp;
    __syncthreads();
    if (tid == 0) sharpness[blk] = (float)((((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]) / (double)(kBlk * kBlk));
    __syncthreads();
    moments_features<kBlk>(features + blk * 36, moments ? moments + (blk * 2) * (kMaps * kMom) : nullptr, mbuf, red, table, tid);
  }
}

inline bool niqe_dims_ok(int B, int H, int W, int cb) {
  if (B < 0 || B > 65535 || cb < 0 || H < 1 || W < 1 || H > 32768 || W > 32768 || cb > 16384) return false;
  const int nby = (H - 2 * cb) / kBlk, nbx = (W - 2 * cb) / kBlk;
  return H - 2 * cb >= kBlk && W - 2 * cb >= kBlk && (int64_t)nby * nbx >= 2;
}

}  // namespace

extern "C" {

size_t vsp_niqe_work_bytes(int B, int H, int W, int crop_border) {
  (void)B; (void)H; (void)W; (void)crop_border;
  return 0;   // every reduction ends inside the block's own workgroup
}

int vsp_niqe_features_u8(double* features, double* moments, float* sharpness, const uint8_t* img, int B, int H, int W, int crop_border,
                         const double* rgam_table, void* work, vsp_stream_t stream) {
  (void)work;
  VSP_REQUIRE(crop_border >= 0, "niqe: crop_border must not be negative (got %d)", crop_border);
  VSP_REQUIRE(B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768, "niqe: bad dims (B <= 65535, H, W <= 32768)");
  VSP_REQUIRE(niqe_dims_ok(B, H, W, crop_border), "niqe: a %d x %d image with crop_border %d has fewer than two 96 x 96 blocks", H, W,
              crop_border);
  VSP_REQUIRE(features && sharpness && img && rgam_table, "niqe: null pointer");
  if (B == 0) return VSP_OK;
  const int nby = (H - 2 * crop_border) / kBlk, nbx = (W - 2 * crop_border) / kBlk;
  NiqeTaps t{};
  {
    double g[7], sum = 0.0;
    const double sigma = 7.0 / 6.0;
    for (int k = 0; k < 7; ++k) sum += g[k] = exp(-(double)((k - 3) * (k - 3)) / (2.0 * sigma * sigma));
    for (int k = 0; k < 7; ++k) t.g[k] = (float)(g[k] / sum);
  }
  const dim3 grid((unsigned)(nbx * nby), (unsigned)B);
  niqe_block_kernel<<<grid, kThreads, 0, vsp::as_stream(stream)>>>(features, moments, sharpness, img, H, W, crop_border, nbx, nby, rgam_table, t);
  return vsp::check_launch("niqe_block");
}

}  // extern "C"

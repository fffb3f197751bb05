// Pair statistics of two uint8 images for gfx950: the exact sum of squared differences (-> PSNR) and the mean structural
// similarity over the valid window positions, in one pass over both images (definitions: include/vspbfr_hip.h).
//
// One 256-thread workgroup owns a 32 x 32 tile of window positions of one image pair, all channels.  The tile plus its
// (w - 1) halo of both images is staged into LDS as bytes with aligned dword loads over the byte stream (an NHWC uint8 row is
// W * C bytes and is not dword aligned in general: each LDS row keeps the misalignment of its global row, so a global dword
// is an LDS dword; only dwords that straddle the ends of the tensor are assembled from bytes).  The five moments
// (x, y, xx, yy, xy) go through a separable window sum: a horizontal pass into LDS (4 adjacent positions per thread share
// their w + 3 bytes), a vertical pass in registers (4 positions below each other share their w + 3 rows).
//
// Numerics.  Box window: every sum up to the final ratio is an exact 32-bit integer (49 * Sxx - Sx^2 <= 49^2 * 255^2 < 2^31),
// so the cancellation of E[x^2] - E[x]^2 costs nothing; one fp32 ratio per position.  Gaussian window: the taps are not
// integers; the moments are accumulated in fp32 around the tile's own rounded mean per image and channel (variance and
// covariance are shift invariant, the shift is added back to the means), which keeps the accumulated squares at the size of
// the tile's contrast instead of its brightness and makes the result insensitive to the taps' own rounding.
//
// Determinism.  Positions are summed in double in a fixed order: per thread, then a fixed butterfly per wave, then the four
// waves in order -> one partial per tile in `work`; the finish kernel (one workgroup per image) adds the tiles in a fixed
// strided order.  Nothing depends on the batch size or on scheduling: image i gets the same bits in any batch.
#include "vsp_common.h"
#include <cmath>
#include <type_traits>

namespace {

constexpr int kTile = 32;             // window positions per tile side
constexpr int kRowDwords = 33;        // LDS row: 3 bytes of misalignment + (32 + 10) * 3 bytes, rounded up to dwords
constexpr int kThreads = 256;

struct GaussTaps { float t[11]; };

template <typename T> __device__ __forceinline__ T wave_sum_t(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// WIN = 7: box window, int moments, sample covariance.  WIN = 11: Gaussian window, centred fp32 moments, population covariance.
template <int WIN, int C>
__global__ __launch_bounds__(kThreads) void pair_stats_tile_kernel(double* part_ssim, unsigned long long* part_sse, const uint8_t* a,
                                                                    const uint8_t* b, int H, int W, int ntx, int nty, GaussTaps g) {
  constexpr bool GAUSS = WIN == 11;
  using T = typename std::conditional<GAUSS, float, int>::type;
  constexpr int IN = kTile + WIN - 1;   // staged rows / columns per tile
  constexpr int NV = WIN + 3;           // inputs of 4 adjacent window positions
  __shared__ uint32_t tile[2][IN][kRowDwords];
  __shared__ T hbuf[5][IN][kTile];
  __shared__ uint32_t red[4][8];
  __shared__ double redd[4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.y, tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
  const int ox0 = tx * kTile, oy0 = ty * kTile;
  const int OWv = W - WIN + 1, OHv = H - WIN + 1;
  const int nvx = min(kTile, OWv - ox0), nvy = min(kTile, OHv - oy0);   // window positions of this tile
  const int ncols = nvx + WIN - 1, nrows = nvy + WIN - 1;                // staged pixels of this tile
  const int64_t rowbytes = (int64_t)W * C;
  const int64_t tile_off = (((int64_t)img * H + oy0) * W + ox0) * C;
  const int64_t total = (int64_t)gridDim.y * H * rowbytes;
  const int L = ncols * C;

  // ---- stage both images: aligned dwords of the byte stream, zero outside the tile
  for (int i = tid; i < 2 * IN * kRowDwords; i += kThreads) {
    const int which = i / (IN * kRowDwords), rem = i - which * (IN * kRowDwords);
    const int r = rem / kRowDwords, d = rem - r * kRowDwords;
    const uint8_t* base = which ? b : a;
    uint32_t v = 0;
    if (r < nrows) {
      const uintptr_t lo = (uintptr_t)base, hi = lo + (uintptr_t)total;
      const uintptr_t A = lo + (uintptr_t)(tile_off + (int64_t)r * rowbytes);
      const uintptr_t p = (A & ~(uintptr_t)3) + 4u * (uintptr_t)d;
      if (p < A + (uintptr_t)L) {
        if (p >= lo && p + 4 <= hi) {
          v = *reinterpret_cast<const uint32_t*>(p);
        } else {   // the first / last dword of the tensor: only the bytes that belong to it
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (p + k >= lo && p + k < hi) v |= (uint32_t)(*reinterpret_cast<const uint8_t*>(p + k)) << (8 * k);
        }
      }
    }
    tile[which][r][d] = v;
  }
  __syncthreads();
  const uint8_t* la = reinterpret_cast<const uint8_t*>(&tile[0][0][0]);
  const uint8_t* lb = reinterpret_cast<const uint8_t*>(&tile[1][0][0]);
  const int misa = (int)(((uintptr_t)a + (uintptr_t)tile_off) & 3), misb = (int)(((uintptr_t)b + (uintptr_t)tile_off) & 3);
  const int rb3 = (int)(rowbytes & 3);
  auto row_a = [&](int r) { return la + r * (kRowDwords * 4) + ((misa + r * rb3) & 3); };
  auto row_b = [&](int r) { return lb + r * (kRowDwords * 4) + ((misb + r * rb3) & 3); };

  // ---- squared differences of the pixels this tile owns (each pixel of the image exactly once: the last tile of a row /
  // column owns the border too), and the tile's channel sums for the centring
  uint32_t acc[7] = {0, 0, 0, 0, 0, 0, 0};   // sse, sum a[c], sum b[c]
  {
    const int own_w = tx == ntx - 1 ? ncols : kTile, own_h = ty == nty - 1 ? nrows : kTile;
    for (int p = tid; p < nrows * ncols; p += kThreads) {
      const int r = p / ncols, x = p - r * ncols;
      const uint8_t* pa = row_a(r) + x * C;
      const uint8_t* pb = row_b(r) + x * C;
      const bool own = x < own_w && r < own_h;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int va = pa[c], vb = pb[c], df = va - vb;
        if (own) acc[0] += (uint32_t)(df * df);
        if (GAUSS) { acc[1 + c] += (uint32_t)va; acc[4 + c] += (uint32_t)vb; }
      }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      if (!GAUSS && k > 0) break;
      const uint32_t s = wave_sum_t<uint32_t>(acc[k]);
      if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
  }
  const uint32_t sse_tile = red[0][0] + red[1][0] + red[2][0] + red[3][0];

  double ssum = 0.0;
  const int vx_ = tid & 31, vr0 = (tid >> 5) * 4;   // vertical pass: column and first of the 4 rows of this thread
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    int ca = 0, cb = 0;
    if (GAUSS) {
      const uint32_t n = (uint32_t)(nrows * ncols);
      ca = (int)((red[0][1 + c] + red[1][1 + c] + red[2][1 + c] + red[3][1 + c] + n / 2) / n);
      cb = (int)((red[0][4 + c] + red[1][4 + c] + red[2][4 + c] + red[3][4 + c] + n / 2) / n);
    }
    // ---- horizontal window sums of the five moments: 4 adjacent positions per item
    for (int i = tid; i < IN * (kTile / 4); i += kThreads) {
      const int r = i >> 3, x0 = (i & 7) * 4;
      const uint8_t* pa = row_a(r) + x0 * C + c;
      const uint8_t* pb = row_b(r) + x0 * C + c;
      T va[NV], vb[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        va[j] = (T)((int)pa[j * C] - ca);
        vb[j] = (T)((int)pb[j * C] - cb);
      }
      T s[5][4];
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        T s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
          const T x = va[o + k], y = vb[o + k];
          if constexpr (GAUSS) {
            const float w = g.t[k];
            s0 = fmaf(w, x, s0); s1 = fmaf(w, y, s1); s2 = fmaf(w, x * x, s2); s3 = fmaf(w, y * y, s3); s4 = fmaf(w, x * y, s4);
          } else {
            s0 += x; s1 += y; s2 += x * x; s3 += y * y; s4 += x * y;
          }
        }
        s[0][o] = s0; s[1][o] = s1; s[2][o] = s2; s[3][o] = s3; s[4][o] = s4;
      }
#pragma unroll
      for (int m = 0; m < 5; ++m)
#pragma unroll
        for (int o = 0; o < 4; ++o) hbuf[m][r][x0 + o] = s[m][o];
    }
    __syncthreads();
    // ---- vertical window sums and the ratio: 4 positions below each other per thread
    T v[5][4];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
      for (int o = 0; o < 4; ++o) v[m][o] = 0;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      T h[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) h[m] = hbuf[m][vr0 + k][vx_];
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        if (k - o < 0 || k - o >= WIN) continue;
#pragma unroll
        for (int m = 0; m < 5; ++m) {
          if constexpr (GAUSS) v[m][o] = fmaf(g.t[k - o], h[m], v[m][o]);
          else v[m][o] += h[m];
        }
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      float q;
      if constexpr (GAUSS) {
        const float C1 = 6.5025f, C2 = 58.5225f;
        const float mx = v[0][o], my = v[1][o];
        const float ux = (float)ca + mx, uy = (float)cb + my;
        const float vx = fmaf(-mx, mx, v[2][o]), vy = fmaf(-my, my, v[3][o]), vxy = fmaf(-mx, my, v[4][o]);
        q = ((2.f * ux * uy + C1) * (2.f * vxy + C2)) / ((fmaf(ux, ux, uy * uy) + C1) * (vx + vy + C2));
      } else {
        // N = 49:  (2 ux uy + C1) / (ux^2 + uy^2 + C1) = (2 Sx Sy + N^2 C1) / (Sx^2 + Sy^2 + N^2 C1), and with the sample
        // covariance vxy = (N Sxy - Sx Sy) / (N (N - 1)):  (2 vxy + C2) / (vx + vy + C2) has the common factor N (N - 1)
        const float K1 = 2401.f * 6.5025f, K2 = 2352.f * 58.5225f;
        const int sx = v[0][o], sy = v[1][o];
        const float a1 = (float)(2 * sx * sy), b1 = (float)(sx * sx + sy * sy);
        const float a2 = (float)(2 * (49 * v[4][o] - sx * sy));
        const float b2 = (float)((49 * v[2][o] - sx * sx) + (49 * v[3][o] - sy * sy));
        q = ((a1 + K1) * (a2 + K2)) / ((b1 + K1) * (b2 + K2));
      }
      if (vx_ < nvx && vr0 + o < nvy) ssum += (double)q;
    }
    __syncthreads();   // hbuf is rewritten by the next channel
  }

  ssum = wave_sum_t<double>(ssum);
  if (lane == 0) redd[wave] = ssum;
  __syncthreads();
  if (tid == 0) {
    const int64_t slot = (int64_t)img * ((int64_t)ntx * nty) + blockIdx.x;
    part_ssim[slot] = ((redd[0] + redd[1]) + redd[2]) + redd[3];
    part_sse[slot] = sse_tile;
  }
}

__global__ __launch_bounds__(kThreads) void pair_stats_finish_kernel(unsigned long long* sse, double* ssim, const double* part_ssim,
                                                                      const unsigned long long* part_sse, int ntiles, double count) {
  __shared__ double rs[4];
  __shared__ unsigned long long re[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* ps = part_ssim + (int64_t)blockIdx.x * ntiles;
  const unsigned long long* pe = part_sse + (int64_t)blockIdx.x * ntiles;
  double s = 0.0;
  unsigned long long e = 0;
  for (int i = tid; i < ntiles; i += kThreads) {
    s += ps[i];
    e += pe[i];
  }
  s = wave_sum_t<double>(s);
  e = wave_sum_t<unsigned long long>(e);
  if (lane == 0) { rs[wave] = s; re[wave] = e; }
  __syncthreads();
  if (tid == 0) {
    ssim[blockIdx.x] = (((rs[0] + rs[1]) + rs[2]) + rs[3]) / count;
    sse[blockIdx.x] = re[0] + re[1] + re[2] + re[3];
  }
}

inline bool pair_stats_dims_ok(int B, int H, int W, int C, int window) {
  return B >= 0 && B <= 65535 && (window == VSP_WIN_UNIFORM7 || window == VSP_WIN_GAUSS11) && (C == 1 || C == 3) && H >= window &&
         W >= window && H <= 32768 && W <= 32768;
}

inline int64_t pair_stats_tiles(int H, int W, int window) {
  return (int64_t)((W - window + 1 + kTile - 1) / kTile) * ((H - window + 1 + kTile - 1) / kTile);
}

}  // namespace

extern "C" {

size_t vsp_pair_stats_work_bytes(int B, int H, int W, int C, int window) {
  if (!pair_stats_dims_ok(B, H, W, C, window)) return 0;
  return (size_t)B * (size_t)pair_stats_tiles(H, W, window) * (sizeof(double) + sizeof(unsigned long long));
}

int vsp_pair_stats_u8(unsigned long long* sse, double* ssim, const uint8_t* a, const uint8_t* b, int B, int H, int W, int C,
                      int window, void* work, vsp_stream_t stream) {
  VSP_REQUIRE(window == VSP_WIN_UNIFORM7 || window == VSP_WIN_GAUSS11, "pair_stats: window must be VSP_WIN_UNIFORM7 or VSP_WIN_GAUSS11");
  VSP_REQUIRE(C == 1 || C == 3, "pair_stats: C must be 1 or 3 (got %d)", C);
  VSP_REQUIRE(H >= window && W >= window, "pair_stats: image %d x %d is smaller than the %d x %d window", H, W, window, window);
  VSP_REQUIRE(pair_stats_dims_ok(B, H, W, C, window), "pair_stats: bad dims (B <= 65535, H, W <= 32768)");
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(sse && ssim && a && b && work, "pair_stats: null pointer");
  VSP_REQUIRE((reinterpret_cast<uintptr_t>(work) & 7u) == 0, "pair_stats: work must be 8-byte aligned");
  const int ntx = (W - window + 1 + kTile - 1) / kTile, nty = (H - window + 1 + kTile - 1) / kTile;
  const int64_t ntiles = (int64_t)ntx * nty;
  double* part_ssim = static_cast<double*>(work);
  unsigned long long* part_sse = reinterpret_cast<unsigned long long*>(part_ssim + (int64_t)B * ntiles);
  GaussTaps g{};
  {
    double t[11], sum = 0.0;
    for (int k = 0; k < 11; ++k) sum += t[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k < 11; ++k) g.t[k] = (float)(t[k] / sum);
  }
  const dim3 grid((unsigned)ntiles, (unsigned)B);
  hipStream_t s = vsp::as_stream(stream);
  if (window == VSP_WIN_UNIFORM7) {
    if (C == 3) pair_stats_tile_kernel<7, 3><<<grid, kThreads, 0, s>>>(part_ssim, part_sse, a, b, H, W, ntx, nty, g);
    else pair_stats_tile_kernel<7, 1><<<grid, kThreads, 0, s>>>(part_ssim, part_sse, a, b, H, W, ntx, nty, g);
  } else {
    if (C == 3) pair_stats_tile_kernel<11, 3><<<grid, kThreads, 0, s>>>(part_ssim, part_sse, a, b, H, W, ntx, nty, g);
    else pair_stats_tile_kernel<11, 1><<<grid, kThreads, 0, s>>>(part_ssim, part_sse, a, b, H, W, ntx, nty, g);
  }
  int rc = vsp::check_launch("pair_stats_tile");
  if (rc != VSP_OK) return rc;
  const double count = (double)C * (double)(W - window + 1) * (double)(H - window + 1);
  pair_stats_finish_kernel<<<(unsigned)B, kThreads, 0, s>>>(sse, ssim, part_ssim, part_sse, (int)ntiles, count);
  return vsp::check_launch("pair_stats_finish");
}

}  // extern "C"

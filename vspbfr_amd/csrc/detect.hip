// Face detection for whole photos: the fp32 layers of RetinaFace / MobileNet-0.25 and its post-processing.
//   det_entry_kernel    u8 RGB photos -> mean subtraction, channel swap, 3 -> 8 stride-2 3x3 (the canvas is never stored)
//   det_sep_kernel      depthwise 3x3 (stride 1 / 2) -> pointwise 1x1; the depthwise tile lives in LDS
//   det_conv3_kernel    dense 3x3, stride 1, 16 output channels per workgroup, into a channel window of the output (the SSH concatenation)
//   det_lateral_kernel  1x1 to 64 channels + nearest upsample-add of the coarser level
//   det_heads_kernel    the three 1x1 heads of one level, written in the (B, priors, .) layout
//   det_nms_kernel      one workgroup per image: decode, candidate selection, sort, suppression mask, greedy sweep
// Activations are NCHW fp32.  Every pointwise weight is laid out [ci][co] (3x3: [ci][tap][co]) so that the row a thread needs is
// wave-uniform and contiguous.  The arithmetic is plain fmaf chains over ci; tests/detect_ref.py restates every layer in float64.
#include "vsp_common.h"

namespace {

__device__ __forceinline__ float act_f(float v, int act, float slope) { return (act && v < 0.f) ? v * slope : v; }

// ------------------------------------------------------------------------------------------------------------------------- entry
__global__ __launch_bounds__(256) void det_entry_kernel(float* __restrict__ y, const uint8_t* __restrict__ src,
                                                        const vsp_det_src* __restrict__ items, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int OH, int OW, int act, float slope) {
  __shared__ float sw[27 * 8 + 8];
  for (int i = threadIdx.x; i < 27 * 8 + 8; i += 256) sw[i] = i < 216 ? w[i] : bias[i - 216];
  __syncthreads();
  const vsp_det_src it = items[blockIdx.y];
  const int P = OH * OW, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int oy = p / OW, ox = p - oy * OW;
  float acc[8];
#pragma unroll
  for (int co = 0; co < 8; ++co) acc[co] = sw[216 + co];
  const uint8_t* ph = src + it.off;
  const float mean[3] = {104.f, 117.f, 123.f};
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if (iy < 0 || iy >= it.h) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if (ix < 0 || ix >= it.w) continue;
      const uint8_t* px = ph + ((int64_t)iy * it.w + ix) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = (float)px[2 - c] - mean[c];          // network channel c is B, G, R
        const float* wr = sw + (c * 9 + ky * 3 + kx) * 8;
#pragma unroll
        for (int co = 0; co < 8; ++co) acc[co] = fmaf(wr[co], v, acc[co]);
      }
    }
  }
  float* yo = y + (int64_t)it.slot * 8 * P + p;
#pragma unroll
  for (int co = 0; co < 8; ++co) yo[(int64_t)co * P] = act_f(acc[co], act, slope);
}

// ------------------------------------------------------------------------------------------------------- depthwise-separable block
// A workgroup takes TPX = 64 S consecutive output pixels of one image: all 256 threads fill t[Cin][TPX] with the activated depthwise
// result, then wave v takes the (64-pixel subtile, 16-channel group) pairs v, v + 4, ... and walks Cin once per pair.
__global__ __launch_bounds__(256) void det_sep_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ wd,
                                                      const float* __restrict__ bd, const float* __restrict__ wp,
                                                      const float* __restrict__ bp, int Cin, int Cout, int H, int W, int OH, int OW,
                                                      int stride, float slope, int S) {
  extern __shared__ float t[];
  const int TPX = 64 * S, P = OH * OW, b = blockIdx.y, tile0 = blockIdx.x * TPX;
  const float* xb = x + (int64_t)b * Cin * H * W;
  for (int idx = threadIdx.x; idx < Cin * TPX; idx += 256) {
    const int ci = idx / TPX, gp = tile0 + (idx - ci * TPX);
    float v = 0.f;
    if (gp < P) {
      const int oy = gp / OW, ox = gp - oy * OW;
      const float* xc = xb + (int64_t)ci * H * W;
      const float* k = wd + ci * 9;
      float s = bd[ci];
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride - 1 + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = ox * stride - 1 + kx;
          if (ix < 0 || ix >= W) continue;
          s = fmaf(k[ky * 3 + kx], xc[iy * W + ix], s);
        }
      }
      v = s < 0.f ? s * slope : s;
    }
    t[idx] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = Cout >> 4, nitems = S * G;
  for (int item = wv; item < nitems; item += 4) {
    const int sub = item / G, co0 = (item - sub * G) * 16, p = sub * 64 + lane;
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = bp[co0 + j];
    const float* tp = t + p;
    const float* wq = wp + co0;
    for (int ci = 0; ci < Cin; ++ci) {
      const float v = tp[ci * TPX];
      const float* wr = wq + ci * Cout;
#pragma unroll
      for (int j = 0; j < 16; ++j) acc[j] = fmaf(wr[j], v, acc[j]);
    }
    const int gp = tile0 + p;
    if (gp < P) {
      float* yo = y + ((int64_t)b * Cout + co0) * P + gp;
#pragma unroll
      for (int j = 0; j < 16; ++j) yo[(int64_t)j * P] = acc[j] < 0.f ? acc[j] * slope : acc[j];
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------------- dense 3x3
// 8 rows x 32 columns of output and 16 output channels per workgroup, one pixel per thread; 8 input channels with their halo per LDS
// stage.  The channel groups of a tile are workgroups of their own (blockIdx.z = image * groups + group): a thread's serial chain is
// Cin * 9 * 16 multiply-adds whatever Cout is, and the small maps of the coarse levels still give the chip a few hundred workgroups.
constexpr int kConv3Co = 16;
__global__ __launch_bounds__(256) void det_conv3_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int Cin, int Cout, int H, int W, int y_ch,
                                                        int y_coff, int act, float slope) {
  __shared__ float tile[8][10][34];
  const int groups = Cout / kConv3Co;
  const int tx0 = blockIdx.x * 32, ty0 = blockIdx.y * 8, b = blockIdx.z / groups, co0 = (blockIdx.z - b * groups) * kConv3Co;
  const int c = threadIdx.x & 31, r = threadIdx.x >> 5;
  float acc[kConv3Co];
#pragma unroll
  for (int co = 0; co < kConv3Co; ++co) acc[co] = bias[co0 + co];
  const float* xb = x + (int64_t)b * Cin * H * W;
  for (int ci0 = 0; ci0 < Cin; ci0 += 8) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < 8 * 340; idx += 256) {
      const int ch = idx / 340, rem = idx - ch * 340, rr = rem / 34, cc = rem - rr * 34;
      const int iy = ty0 - 1 + rr, ix = tx0 - 1 + cc;
      float v = 0.f;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = xb[((int64_t)(ci0 + ch) * H + iy) * W + ix];
      tile[ch][rr][cc] = v;
    }
    __syncthreads();
    for (int ch = 0; ch < 8; ++ch) {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float v = tile[ch][r + ky][c + kx];
          const float* wr = w + ((int64_t)(ci0 + ch) * 9 + ky * 3 + kx) * Cout + co0;
#pragma unroll
          for (int co = 0; co < kConv3Co; ++co) acc[co] = fmaf(wr[co], v, acc[co]);
        }
      }
    }
  }
  const int oy = ty0 + r, ox = tx0 + c;
  if (oy < H && ox < W) {
    float* yo = y + (((int64_t)b * y_ch + y_coff + co0) * H + oy) * W + ox;
#pragma unroll
    for (int co = 0; co < kConv3Co; ++co) yo[(int64_t)co * H * W] = act_f(acc[co], act, slope);
  }
}

// ------------------------------------------------------------------------------------------------------------- lateral 1x1 + upsample-add
__global__ __launch_bounds__(256) void det_lateral_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, const float* __restrict__ up, int Cin, int H,
                                                          int W, int h2, int w2, int act, float slope) {
  const int P = H * W, p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= P) return;
  float acc[64];
#pragma unroll
  for (int co = 0; co < 64; ++co) acc[co] = bias[co];
  const float* xp = x + (int64_t)b * Cin * P + p;
  for (int ci = 0; ci < Cin; ++ci) {
    const float v = xp[(int64_t)ci * P];
    const float* wr = w + ci * 64;
#pragma unroll
    for (int co = 0; co < 64; ++co) acc[co] = fmaf(wr[co], v, acc[co]);
  }
  const int oy = p / W, ox = p - oy * W;
  const float* us = up ? up + (int64_t)b * 64 * h2 * w2 + ((oy * h2) / H) * w2 + (ox * w2) / W : nullptr;
  float* yo = y + (int64_t)b * 64 * P + p;
#pragma unroll
  for (int co = 0; co < 64; ++co) {
    float v = act_f(acc[co], act, slope);
    if (us) v += us[(int64_t)co * h2 * w2];
    yo[(int64_t)co * P] = v;
  }
}

// --------------------------------------------------------------------------------------------------------------------------- heads
__global__ __launch_bounds__(256) void det_heads_kernel(float* __restrict__ conf, float* __restrict__ loc, float* __restrict__ lm,
                                                        const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, int HW, int P, int p0) {
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= HW) return;
  float acc[32];
#pragma unroll
  for (int co = 0; co < 32; ++co) acc[co] = bias[co];
  const float* xp = x + (int64_t)b * 64 * HW + p;
  for (int ci = 0; ci < 64; ++ci) {
    const float v = xp[(int64_t)ci * HW];
    const float* wr = w + ci * 32;
#pragma unroll
    for (int co = 0; co < 32; ++co) acc[co] = fmaf(wr[co], v, acc[co]);
  }
  const int64_t q = (int64_t)b * P + p0 + 2 * p;             // the cell's first prior: anchors are adjacent
  float* c = conf + q * 2;
  float* l = loc + q * 4;
  float* m = lm + q * 10;
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = acc[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) l[i] = acc[4 + i];
#pragma unroll
  for (int i = 0; i < 20; ++i) m[i] = acc[12 + i];
}

// ------------------------------------------------------------------------------------------------------------------- decode + NMS
constexpr int kNmsThreads = 1024, kNmsWaves = kNmsThreads / 64;
constexpr int kMaskStride = VSP_DET_MAX_CANDIDATES / 32;      // words per row of the suppression mask: one per lane of the sweeping wave

__device__ __forceinline__ void det_prior(int idx, int Hc, int Wc, float& cx, float& cy, float& m) {
  const int W0 = (Wc + 7) >> 3, H0 = (Hc + 7) >> 3, W1 = (Wc + 15) >> 4, H1 = (Hc + 15) >> 4, W2 = (Wc + 31) >> 5;
  const int n0 = 2 * H0 * W0, n1 = 2 * H1 * W1;
  int k, r, Wk;
  if (idx < n0) { k = 0; r = idx; Wk = W0; }
  else if (idx < n0 + n1) { k = 1; r = idx - n0; Wk = W1; }
  else { k = 2; r = idx - n0 - n1; Wk = W2; }
  const int cell = r >> 1, i = cell / Wk, j = cell - i * Wk;
  const float step = (float)(8 << k);
  m = (float)(16 << (2 * k + (r & 1)));
  cx = ((float)j + 0.5f) * step;
  cy = ((float)i + 0.5f) * step;
}

__device__ __forceinline__ void det_box(const float* l, float cx, float cy, float m, float* box) {
  const float v = 0.1f * m;
  const float bx = cx + l[0] * v, by = cy + l[1] * v;
  const float bw = m * expf(0.2f * l[2]), bh = m * expf(0.2f * l[3]);
  box[0] = bx - 0.5f * bw;
  box[1] = by - 0.5f * bh;
  box[2] = bx + 0.5f * bw;
  box[3] = by + 0.5f * bh;
}

__device__ __forceinline__ int nms_block_sum(int v, int* sh) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
  __syncthreads();
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  int tot = 0;
#pragma unroll
  for (int k = 0; k < kNmsWaves; ++k) tot += sh[k];
  return tot;
}

__device__ __forceinline__ int nms_block_excl_scan(int v, int* sh, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(incl, d);
    if (lane >= d) incl += o;
  }
  __syncthreads();
  if (lane == 63) sh[wv] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kNmsWaves; ++k) {
    const int s = sh[k];
    if (k < wv) base += s;
    tot += s;
  }
  *total = tot;
  return base + incl - v;
}

__global__ __launch_bounds__(kNmsThreads) void det_nms_kernel(vsp_det_face* __restrict__ faces, int32_t* __restrict__ info,
                                                              uint8_t* __restrict__ work, int64_t work_per_image, int64_t key_bytes,
                                                              const float* __restrict__ conf, const float* __restrict__ loc,
                                                              const float* __restrict__ lm, int P, int Hc, int Wc, float thr, float nms,
                                                              int K, int max_faces) {
  __shared__ unsigned long long skey[VSP_DET_MAX_CANDIDATES];
  __shared__ float sbox[VSP_DET_MAX_CANDIDATES][4];
  __shared__ int sh[kNmsWaves];
  __shared__ uint32_t skeepw[64];
  __shared__ int spre[64];
  const int tid = threadIdx.x, b = blockIdx.x;
  uint32_t* keys = reinterpret_cast<uint32_t*>(work + (int64_t)b * work_per_image);
  uint32_t* mask = reinterpret_cast<uint32_t*>(work + (int64_t)b * work_per_image + key_bytes);
  const float* cb = conf + (int64_t)b * P * 2;
  const float* lb = loc + (int64_t)b * P * 4;
  const float* mb = lm + (int64_t)b * P * 10;

  // 1. keys: the score's bits for a candidate, 0 for everything else
  int mine = 0, bad = 0;
  for (int i = tid; i < P; i += kNmsThreads) {
    const float score = 1.f / (1.f + expf(cb[2 * i] - cb[2 * i + 1]));
    uint32_t key = 0;
    if (score > thr) {
      float cx, cy, m, box[4];
      det_prior(i, Hc, Wc, cx, cy, m);
      det_box(lb + 4 * i, cx, cy, m, box);
      bool fin = isfinite(box[0]) && isfinite(box[1]) && isfinite(box[2]) && isfinite(box[3]);
      const float v = 0.1f * m;
#pragma unroll
      for (int q = 0; q < 10; ++q) fin = fin && isfinite(((q & 1) ? cy : cx) + mb[10 * i + q] * v);
      if (fin) { key = __float_as_uint(score); ++mine; }
      else ++bad;
    }
    keys[i] = key;
  }
  const int ncand = nms_block_sum(mine, sh);
  const int nbad = nms_block_sum(bad, sh);
  __syncthreads();

  // 2. the K-th largest key, bit by bit, when there are more than K candidates; ties at it go to the lower prior index (step 3)
  uint32_t T = 0;
  int n_gt = ncand, eq_take = 0;
  if (ncand > K) {
    for (int bit = 31; bit >= 0; --bit) {
      const uint32_t cand = T | (1u << bit);
      int c = 0;
      for (int i = tid; i < P; i += kNmsThreads) c += keys[i] >= cand;
      if (nms_block_sum(c, sh) >= K) T = cand;
    }
    int c = 0;
    for (int i = tid; i < P; i += kNmsThreads) c += keys[i] > T;
    n_gt = nms_block_sum(c, sh);
    eq_take = K - n_gt;
  }
  const int M = ncand < K ? ncand : K;

  // 3. ordered compaction (prefix sums over the prior index) into skey = (score bits, ~prior)
  int base_gt = 0, base_eq = 0;
  for (int c0 = 0; c0 < P; c0 += kNmsThreads) {
    const int i = c0 + tid;
    const uint32_t key = i < P ? keys[i] : 0u;
    const int gt = key > T, eq = T != 0u && key == T;
    int total;
    const int excl = nms_block_excl_scan(gt | (eq << 16), sh, &total);
    const unsigned long long rec = ((unsigned long long)key << 32) | (0xFFFFFFFFu - (uint32_t)i);
    if (gt) {
      const int pos = base_gt + (excl & 0xffff);
      if (pos < VSP_DET_MAX_CANDIDATES) skey[pos] = rec;
    } else if (eq) {
      const int rk = base_eq + (excl >> 16);
      if (rk < eq_take && n_gt + rk < VSP_DET_MAX_CANDIDATES) skey[n_gt + rk] = rec;
    }
    base_gt += total & 0xffff;
    base_eq += total >> 16;
  }
  int N = 64;
  while (N < M) N <<= 1;                                      // M <= K <= 2048
  __syncthreads();
  for (int i = M + tid; i < N; i += kNmsThreads) skey[i] = 0ull;

  // 4. bitonic sort, descending: score first, lower prior index first among equal scores
  for (int k = 2; k <= N; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < N; i += kNmsThreads) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = skey[i], c = skey[l];
          if (((i & k) == 0) ? a < c : a > c) { skey[i] = c; skey[l] = a; }
        }
      }
    }
  }
  __syncthreads();

  // 5. boxes of the sorted candidates, then the suppression mask: bit j of row i = (j > i and IoU(i, j) > nms)
  for (int i = tid; i < M; i += kNmsThreads) {
    const int idx = (int)(0xFFFFFFFFu - (uint32_t)skey[i]);
    float cx, cy, m;
    det_prior(idx, Hc, Wc, cx, cy, m);
    det_box(lb + 4 * idx, cx, cy, m, sbox[i]);
  }
  __syncthreads();
  const int MW = (M + 31) >> 5;
  for (int item = tid; item < M * MW; item += kNmsThreads) {
    const int i = item / MW, wd = item - i * MW;
    uint32_t bits = 0;
    if (wd * 32 + 31 > i) {
      const float ax1 = sbox[i][0], ay1 = sbox[i][1], ax2 = sbox[i][2], ay2 = sbox[i][3];
      const float aa = (ax2 - ax1) * (ay2 - ay1);
      for (int q = 0; q < 32; ++q) {
        const int j = wd * 32 + q;
        if (j > i && j < M) {
          const float iw = fminf(ax2, sbox[j][2]) - fmaxf(ax1, sbox[j][0]);
          const float ih = fminf(ay2, sbox[j][3]) - fmaxf(ay1, sbox[j][1]);
          const float inter = fmaxf(iw, 0.f) * fmaxf(ih, 0.f);
          const float ab = (sbox[j][2] - sbox[j][0]) * (sbox[j][3] - sbox[j][1]);
          if (inter / (aa + ab - inter) > nms) bits |= 1u << q;
        }
      }
    }
    mask[(int64_t)i * kMaskStride + wd] = bits;
  }
  __syncthreads();

  // 6. one wave sweeps the candidates in order; lane l owns the `removed` and `kept` bits of candidates 32 l .. 32 l + 31
  if (tid < 64) {
    uint32_t removed = 0, keptw = 0;
    int kept = 0, capped = 0;
    for (int i = 0; i < M; ++i) {
      const uint32_t wrd = __shfl(removed, i >> 5);
      if (!((wrd >> (i & 31)) & 1u)) {
        if (kept == max_faces) { capped = 1; break; }
        ++kept;
        if (tid == (i >> 5)) keptw |= 1u << (i & 31);
        if (tid < MW) removed |= mask[(int64_t)i * kMaskStride + tid];
      }
    }
    const int pc = __popc(keptw);
    int incl = pc;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (tid >= d) incl += o;
    }
    skeepw[tid] = keptw;
    spre[tid] = incl - pc;
    if (tid == 0) {
      info[4 * b] = kept;
      info[4 * b + 1] = (ncand > K ? VSP_DET_CAND_CAPPED : 0) | (capped ? VSP_DET_FACES_CAPPED : 0) | (nbad ? VSP_DET_NONFINITE : 0);
      info[4 * b + 2] = ncand;
      info[4 * b + 3] = nbad;
    }
  }
  __syncthreads();

  // 7. the records of the kept candidates, in order
  for (int i = tid; i < M; i += kNmsThreads) {
    const uint32_t wrd = skeepw[i >> 5];
    if (!((wrd >> (i & 31)) & 1u)) continue;
    const int k = spre[i >> 5] + __popc(wrd & ((1u << (i & 31)) - 1u));
    const int idx = (int)(0xFFFFFFFFu - (uint32_t)skey[i]);
    float cx, cy, m;
    det_prior(idx, Hc, Wc, cx, cy, m);
    vsp_det_face f;
#pragma unroll
    for (int q = 0; q < 4; ++q) f.box[q] = sbox[i][q];
    f.score = __uint_as_float((uint32_t)(skey[i] >> 32));
    const float v = 0.1f * m;
#pragma unroll
    for (int q = 0; q < 10; ++q) f.lm[q] = ((q & 1) ? cy : cx) + mb[10 * idx + q] * v;
    f.prior = idx;
    faces[(int64_t)b * max_faces + k] = f;
  }
}

constexpr int64_t kTwoGiB = (int64_t)1 << 31;

inline bool dims_ok(int B, int H, int W) { return B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= VSP_DET_MAX_SIDE && W <= VSP_DET_MAX_SIDE; }
inline int64_t tensor_bytes(int B, int C, int H, int W) { return (int64_t)B * C * H * W * 4; }

}  // namespace

extern "C" {

int vsp_det_entry_u8(float* y, const uint8_t* src, size_t src_bytes, const vsp_det_src* items, const vsp_det_src* items_dev, int n,
                     const float* w, const float* b, int B, int Hc, int Wc, int act, float slope, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, Hc, Wc), "det_entry: batch %d, canvas %d x %d (sides 1..%d)", B, Hc, Wc, VSP_DET_MAX_SIDE);
  VSP_REQUIRE(n >= 0 && n <= B, "det_entry: %d items for a batch of %d", n, B);
  VSP_REQUIRE(act == 0 || act == 1, "det_entry: act %d", act);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(y && src && items && items_dev && w && b, "det_entry: null pointer");
  const int OH = (Hc + 1) / 2, OW = (Wc + 1) / 2;
  if ((int64_t)src_bytes >= kTwoGiB || tensor_bytes(B, 8, OH, OW) >= kTwoGiB)
    return vsp::fail(VSP_ENOTSUP, "det_entry: a buffer of 2 GiB or more");
  for (int i = 0; i < n; ++i) {
    const vsp_det_src& it = items[i];
    VSP_REQUIRE(it.h >= 1 && it.w >= 1 && it.h <= Hc && it.w <= Wc, "det_entry: item %d: photo %d x %d does not fit the %d x %d canvas", i,
                it.h, it.w, Hc, Wc);
    VSP_REQUIRE(it.off >= 0 && it.off + (int64_t)3 * it.h * it.w <= (int64_t)src_bytes, "det_entry: item %d: bytes outside src", i);
    VSP_REQUIRE(it.slot >= 0 && it.slot < B, "det_entry: item %d: slot %d outside 0..%d", i, it.slot, B - 1);
  }
  det_entry_kernel<<<dim3((OH * OW + 255) / 256, n), 256, 0, vsp::as_stream(stream)>>>(y, src, items_dev, w, b, OH, OW, act, slope);
  return vsp::check_launch("det_entry");
}

int vsp_det_sep_f32(float* y, const float* x, const float* wd, const float* bd, const float* wp, const float* bp, int B, int Cin, int Cout,
                    int H, int W, int stride, float slope, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, H, W), "det_sep: batch %d, map %d x %d", B, H, W);
  VSP_REQUIRE(Cin >= 1 && Cin <= 256, "det_sep: Cin %d (1..256)", Cin);
  VSP_REQUIRE(Cout >= 16 && Cout <= 256 && Cout % 16 == 0, "det_sep: Cout %d (a multiple of 16 up to 256)", Cout);
  VSP_REQUIRE(stride == 1 || stride == 2, "det_sep: stride %d (1 or 2)", stride);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(y && x && wd && bd && wp && bp, "det_sep: null pointer");
  const int OH = (H - 1) / stride + 1, OW = (W - 1) / stride + 1;
  if (tensor_bytes(B, Cin, H, W) >= kTwoGiB || tensor_bytes(B, Cout, OH, OW) >= kTwoGiB)
    return vsp::fail(VSP_ENOTSUP, "det_sep: a tensor of 2 GiB or more");
  int S = Cout == 16 ? 4 : Cout == 32 ? 2 : 1;                // keep the four waves busy in the pointwise phase
  while (S > 1 && Cin * 64 * S * 4 > 65536) S >>= 1;
  const int TPX = 64 * S;
  det_sep_kernel<<<dim3((OH * OW + TPX - 1) / TPX, B), 256, (size_t)Cin * TPX * 4, vsp::as_stream(stream)>>>(
      y, x, wd, bd, wp, bp, Cin, Cout, H, W, OH, OW, stride, slope, S);
  return vsp::check_launch("det_sep");
}

int vsp_det_conv3x3_f32(float* y, const float* x, const float* w, const float* b, int B, int Cin, int Cout, int H, int W, int y_ch,
                        int y_coff, int act, float slope, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, H, W), "det_conv3x3: batch %d, map %d x %d", B, H, W);
  VSP_REQUIRE(Cin >= 8 && Cin <= 1024 && Cin % 8 == 0, "det_conv3x3: Cin %d (a multiple of 8)", Cin);
  VSP_REQUIRE(Cout == 16 || Cout == 32 || Cout == 64, "det_conv3x3: Cout %d (16, 32 or 64)", Cout);
  VSP_REQUIRE(y_coff >= 0 && y_ch >= 1 && y_ch <= 4096 && y_coff + Cout <= y_ch, "det_conv3x3: channels %d..%d of %d", y_coff,
              y_coff + Cout - 1, y_ch);
  VSP_REQUIRE(act == 0 || act == 1, "det_conv3x3: act %d", act);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(y && x && w && b, "det_conv3x3: null pointer");
  if (tensor_bytes(B, Cin, H, W) >= kTwoGiB || tensor_bytes(B, y_ch, H, W) >= kTwoGiB)
    return vsp::fail(VSP_ENOTSUP, "det_conv3x3: a tensor of 2 GiB or more");
  VSP_REQUIRE((int64_t)B * (Cout / kConv3Co) <= 65535, "det_conv3x3: batch %d times %d channel groups exceeds the grid", B, Cout / kConv3Co);
  const dim3 grid((W + 31) / 32, (H + 7) / 8, B * (Cout / kConv3Co));
  det_conv3_kernel<<<grid, 256, 0, vsp::as_stream(stream)>>>(y, x, w, b, Cin, Cout, H, W, y_ch, y_coff, act, slope);
  return vsp::check_launch("det_conv3x3");
}

int vsp_det_lateral_f32(float* y, const float* x, const float* w, const float* b, const float* up, int B, int Cin, int H, int W, int h2,
                        int w2, int act, float slope, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, H, W), "det_lateral: batch %d, map %d x %d", B, H, W);
  VSP_REQUIRE(Cin >= 1 && Cin <= 4096, "det_lateral: Cin %d", Cin);
  VSP_REQUIRE(act == 0 || act == 1, "det_lateral: act %d", act);
  VSP_REQUIRE(!up || (h2 >= 1 && w2 >= 1 && h2 <= H && w2 <= W), "det_lateral: coarser map %d x %d for %d x %d", h2, w2, H, W);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(y && x && w && b, "det_lateral: null pointer");
  if (tensor_bytes(B, Cin, H, W) >= kTwoGiB || tensor_bytes(B, 64, H, W) >= kTwoGiB)
    return vsp::fail(VSP_ENOTSUP, "det_lateral: a tensor of 2 GiB or more");
  det_lateral_kernel<<<dim3((H * W + 255) / 256, B), 256, 0, vsp::as_stream(stream)>>>(y, x, w, b, up, Cin, H, W, h2, w2, act, slope);
  return vsp::check_launch("det_lateral");
}

int vsp_det_heads_f32(float* conf, float* loc, float* lm, const float* x, const float* w, const float* b, int B, int H, int W, int P,
                      int p0, vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, H, W), "det_heads: batch %d, map %d x %d", B, H, W);
  VSP_REQUIRE(p0 >= 0 && P >= 1 && (int64_t)p0 + (int64_t)2 * H * W <= P, "det_heads: priors %d..%lld of %d", p0,
              (long long)p0 + (long long)2 * H * W - 1, P);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(conf && loc && lm && x && w && b, "det_heads: null pointer");
  if (tensor_bytes(B, 64, H, W) >= kTwoGiB || (int64_t)B * P * 40 >= kTwoGiB)
    return vsp::fail(VSP_ENOTSUP, "det_heads: a tensor of 2 GiB or more");
  det_heads_kernel<<<dim3((H * W + 255) / 256, B), 256, 0, vsp::as_stream(stream)>>>(conf, loc, lm, x, w, b, H * W, P, p0);
  return vsp::check_launch("det_heads");
}

int vsp_det_priors(int Hc, int Wc) {
  if (Hc < 1 || Wc < 1 || Hc > VSP_DET_MAX_SIDE || Wc > VSP_DET_MAX_SIDE) return 0;
  int P = 0;
  for (int s = 8; s <= 32; s *= 2) P += 2 * ((Hc + s - 1) / s) * ((Wc + s - 1) / s);
  return P;
}

size_t vsp_det_work_bytes(int B, int Hc, int Wc, int max_candidates) {
  const int P = vsp_det_priors(Hc, Wc);
  if (B < 1 || B > 65535 || P == 0 || max_candidates < 1 || max_candidates > VSP_DET_MAX_CANDIDATES) return 0;
  const size_t keys = ((size_t)P * 4 + 15) / 16 * 16;
  return (size_t)B * (keys + (size_t)max_candidates * kMaskStride * 4);
}

int vsp_det_decode_nms_f32(vsp_det_face* faces, int32_t* info, uint8_t* work, size_t work_bytes, const float* conf, const float* loc,
                           const float* lm, int B, int Hc, int Wc, float threshold, float nms, int max_candidates, int max_faces,
                           vsp_stream_t stream) {
  VSP_REQUIRE(dims_ok(B, Hc, Wc), "det_decode_nms: batch %d, canvas %d x %d (sides 1..%d)", B, Hc, Wc, VSP_DET_MAX_SIDE);
  VSP_REQUIRE(threshold >= 0.f && threshold < 1.f, "det_decode_nms: threshold %g outside [0, 1)", (double)threshold);
  VSP_REQUIRE(nms >= 0.f && nms <= 1.f, "det_decode_nms: nms %g outside [0, 1]", (double)nms);
  VSP_REQUIRE(max_candidates >= 1 && max_candidates <= VSP_DET_MAX_CANDIDATES, "det_decode_nms: max_candidates %d (1..%d)", max_candidates,
              VSP_DET_MAX_CANDIDATES);
  VSP_REQUIRE(max_faces >= 1, "det_decode_nms: max_faces %d", max_faces);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(faces && info && work && conf && loc && lm, "det_decode_nms: null pointer");
  const int P = vsp_det_priors(Hc, Wc);
  if ((int64_t)B * P * 40 >= kTwoGiB || (int64_t)B * max_faces * (int64_t)sizeof(vsp_det_face) >= kTwoGiB || (int64_t)work_bytes >= kTwoGiB)
    return vsp::fail(VSP_ENOTSUP, "det_decode_nms: a buffer of 2 GiB or more");
  const size_t need = vsp_det_work_bytes(B, Hc, Wc, max_candidates);
  VSP_REQUIRE(work_bytes >= need, "det_decode_nms: work of %zu bytes, %zu needed", work_bytes, need);
  VSP_REQUIRE(vsp::aligned16(work), "det_decode_nms: work must be 16-byte aligned");
  const int64_t key_bytes = ((int64_t)P * 4 + 15) / 16 * 16;
  det_nms_kernel<<<B, kNmsThreads, 0, vsp::as_stream(stream)>>>(faces, info, work, (int64_t)(need / B), key_bytes, conf, loc, lm, P, Hc, Wc,
                                                                 threshold, nms, max_candidates, max_faces);
  return vsp::check_launch("det_decode_nms");
}

}  // extern "C"

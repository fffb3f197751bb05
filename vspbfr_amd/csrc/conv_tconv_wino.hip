// Stride-2 transposed 3x3 convolution (the up-convs) as a FUSED Winograd F(2x2,2x2) phase kernel on the fp32 MFMA.
//
// On the (H+1) x (W+1) position grid of conv_pipe.hip MODE 1, position (m, c) produces the 2 x 2 outputs y[2m+py, 2c+px]:
//   phase (0,0) = W[0,0] x[m,c] + W[0,2] x[m,c-1] + W[2,0] x[m-1,c] + W[2,2] x[m-1,c-1]      (2 x 2 taps)
//   phase (0,1) = W[0,1] x[m,c] + W[2,1] x[m-1,c]                                            (2 x 1)
//   phase (1,0) = W[1,0] x[m,c] + W[1,2] x[m,c-1]                                            (1 x 2)
//   phase (1,1) = W[1,1] x[m,c]                                                              (1 x 1)
// A 2-tap correlation y_i = g0 d_i + g1 d_(i+1) over two neighbouring positions is Winograd F(2,2) with points 0, 1, inf:
//   m0 = (d0 - d1) g0, m1 = d1 (g0 + g1), m2 = (d2 - d1) g1, y0 = m0 + m1, y1 = m1 + m2 -- three products instead of four, every
// constant 0 or +-1.  One tile = 2 x 2 positions = 4 x 4 outputs over the 3 x 3 input window d[r][s] = x[m0-1+r, c0-1+s]; per (ci, co)
// it takes 9 + 6 + 6 + 4 = 25 products where the direct form takes 36.  The 25 products read 16 distinct transformed weights
// (the 1-tap axis of phases (0,1) / (1,0) / (1,1) has no transform, so both positions along it share the weight):
//   U[3 i + j]  = gy_i gx_j W      phase (0,0), g_0 = tap 2, g_1 = tap 2 + tap 0, g_2 = tap 0
//   U[9 + i]    = gy_i W[., 1]     phase (0,1)
//   U[12 + j]   = gx_j W[1, .]     phase (1,0)
//   U[15]       = W[1, 1]          phase (1,1)
// Mapping: v_mfma_f32_16x16x4_f32 with A = U (M = 16 output channels), B = transformed input (N = 16 tiles, K = 4 input channels); lane
// (tile n = lane & 15, channel kq = lane >> 4) loads the 3 x 3 window of ITS tile and ITS channel straight from global memory (nine
// 4-byte buffer loads, two k-steps ahead; words outside the image come back as zeros from the buffer range check: the implicit padding
// of the position grid), transforms it in registers (16 subtractions) and holds the 25 B operands of the k-step.  The tiles of an
// image are numbered row-major and a wave takes 16 consecutive ones, so the ragged last tile row / column (H + 1 and W + 1 are odd on
// every map of the path) costs no idle N-blocks; the epilogue masks what lies outside (2H+1) x (2W+1).
// A workgroup = 4 waves = 64 tiles x ONE block of 16 output channels: 25 accumulator quads per lane (100 registers, two waves per SIMD).
// U goes global -> registers -> LDS (two chunks of two k-steps, one barrier per chunk), multiplied by the style scale of its input
// channel on the way (the copy passes through registers anyway), so the window path carries no multiply.
//   U image: [co / 16][ci / 4][quad 4][lane 64][4]   lane = 16 (ci % 4) + (co % 16), element e of quad q: U[4 q + e]
#include "conv_kernel.h"

namespace vspconv {

namespace {

typedef float tw_f4 __attribute__((ext_vector_type(4)));
typedef float tw_f4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int TW_THR = 256;               // 4 waves: 64 tiles x 16 output channels
constexpr int TW_KC = 2;                  // k-steps (of 4 input channels) per LDS chunk
constexpr int TW_SLAB = 4 * 64 * 4;       // floats of one (channel block, k-step) slab of U
constexpr int TW_OOB = 0x7ffffff0;

struct TwPlan {
  int ntx, ntiles, nwn, ncb, nks;         // tiles per row / per image, workgroups per image along the tiles, 16-channel blocks, k-steps
};

// ------------------------------------------------------------------------------------------------------------ weights
// g_0 = tap 2, g_1 = tap 2 + tap 0, g_2 = tap 0 (the 2-tap axis of an even output phase); sums in fp64, rounded once
__global__ __launch_bounds__(256) void tconvw_weight_kernel(float* __restrict__ U, const float* __restrict__ wp, int cin, int cout, int nks,
                                                            int64_t units, float scale) {
  const int64_t unit = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= units) return;
  const int lane = threadIdx.x & 63, kq = lane >> 4, lr = lane & 15;
  const int ks = (int)(unit % nks), cb = (int)(unit / nks);
  const int ci = 4 * ks + kq, co = 16 * cb + lr;
  const bool ok = ci < cin && co < cout;
  double w[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) w[t] = ok ? (double)wp[((int64_t)t * cin + ci) * cout + co] * (double)scale : 0.0;
  const double c[3][3] = {{0., 0., 1.}, {1., 0., 1.}, {1., 0., 0.}};   // c[i][tap]: the taps g_i sums
  float u[16];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double s = 0.;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) s += c[i][ky] * c[j][kx] * w[ky * 3 + kx];
      u[3 * i + j] = (float)s;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double s = 0., t = 0.;
#pragma unroll
    for (int k = 0; k < 3; ++k) { s += c[i][k] * w[k * 3 + 1]; t += c[i][k] * w[3 + k]; }
    u[9 + i] = (float)s;
    u[12 + i] = (float)t;
  }
  u[15] = (float)w[4];
  tw_f4* dst = reinterpret_cast<tw_f4*>(U + unit * (int64_t)TW_SLAB) + lane;
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[q * 64] = tw_f4{u[4 * q], u[4 * q + 1], u[4 * q + 2], u[4 * q + 3]};
}

// ------------------------------------------------------------------------------------------------------------ the convolution
__global__ __launch_bounds__(TW_THR, 2) void conv_tconv_wino_kernel(const ConvK p, const TwPlan pl) {
  __shared__ __attribute__((aligned(16))) float Ul[2 * TW_KC * TW_SLAB];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, kq = lane >> 4;

  // work order: every XCD (workgroup id % 8) walks a contiguous range of (image, tile group, channel block) with the channel blocks of
  // one tile group adjacent -- they read the same windows back to back out of one L2 (conv_kernel.h)
  const int GT = gridDim.x, wgid = blockIdx.x;
  const int xcd = wgid & 7, xq = GT >> 3, xr = GT & 7;
  int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (wgid >> 3);
  const int cb = lid % pl.ncb;
  lid /= pl.ncb;
  const int wn = lid % pl.nwn, b = lid / pl.nwn;
  const int nks = pl.nks;
  const int chw = p.H * p.W;

  // the lane's tile and the byte offsets of its 3 x 3 window inside channel kq of a k-step (TW_OOB: outside -> reads 0)
  const int tile = wn * 64 + wave * 16 + lr;
  const bool tok = tile < pl.ntiles;
  const int ty = tile / pl.ntx, tx = tile - ty * pl.ntx;
  const int m0 = 2 * ty, c0 = 2 * tx;
  int voff[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int iy = m0 - 1 + r, ix = c0 - 1 + s;
      const bool in = tok && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
      voff[3 * r + s] = in ? (kq * chw + iy * p.W + ix) * 4 : TW_OOB;
    }
  const float* xb = p.x + (int64_t)b * p.x_ch * chw;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, p.Cin * chw * 4, 0x00020000);
  const __amdgpu_buffer_rsrc_t urs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w) + (int64_t)cb * nks * TW_SLAB, 0, nks * TW_SLAB * 4, 0x00020000);
  const float* scp = p.wtp + (int64_t)b * p.wt_bs + (int64_t)((tid >> 4) & 3) * p.wt_cs;   // style scale of the channel this thread stages

  // Raw windows in FOUR register sets: k-step ks reads set ks % 4 and the loads of k-step ks + 2 go into set (ks + 2) % 4, whose last
  // reader was k-step ks - 2 -- a load never targets a register that is still read, so nothing is copied (and waited for) behind it.
  // (Two sets and a conditional k-step: hipcc loaded into fresh registers and moved them over at the end of the k-step, behind
  //  s_waitcnt vmcnt(8 .. 0) -- the whole load latency exposed in every k-step.)
  float win[2 * TW_KC][9];
  tw_f4 ust[TW_KC];        // U of the next chunk
  float usc[TW_KC];
  // (the loop body is four k-steps; a k-step past Cin / 4 takes zeros on BOTH operands: its U comes from an out-of-range offset, its window
  //  through a descriptor of zero bytes -- a scalar select, no vector instruction --, so an Inf of a real input never meets a zero weight)
  const __amdgpu_buffer_rsrc_t zrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, 0, 0x00020000);
  auto load_win = [&](int ks, float (&w)[9]) {
    const bool past = ks >= nks;
    const int so = __builtin_amdgcn_readfirstlane((past ? nks - 1 : ks) * 4 * chw * 4);
    const __amdgpu_buffer_rsrc_t rs = past ? zrs : xrs;
#pragma unroll
    for (int e = 0; e < 9; ++e) w[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff[e], so, 0));
  };
  auto load_u = [&](int ch) {                    // (k-steps past the end: an out-of-range offset reads zeros)
#pragma unroll
    for (int kk = 0; kk < TW_KC; ++kk) {
      const int ks = ch * TW_KC + kk;
      const int ksc = ks < nks ? ks : nks - 1;
      ust[kk] = __builtin_bit_cast(tw_f4, __builtin_amdgcn_raw_buffer_load_b128(urs, ks < nks ? tid * 16 : TW_OOB,
                                                                                  __builtin_amdgcn_readfirstlane(ksc * TW_SLAB * 4), 0));
      usc[kk] = scp[(int64_t)4 * ksc * p.wt_cs];
    }
  };
  auto commit_u = [&](float* buf) {
#pragma unroll
    for (int kk = 0; kk < TW_KC; ++kk) *reinterpret_cast<tw_f4*>(buf + kk * TW_SLAB + tid * 4) = ust[kk] * usc[kk];
  };

  tw_f4 acc[25];
#pragma unroll
  for (int i = 0; i < 25; ++i) acc[i] = tw_f4{0.f, 0.f, 0.f, 0.f};

  // one k-step: transform the window (16 subtractions), then 25 MFMAs
  auto kstep = [&](const float (&d)[9], const float* us) {
    float a[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const tw_f4 v = *reinterpret_cast<const tw_f4*>(us + q * 256 + lane * 4);
      a[4 * q] = v[0]; a[4 * q + 1] = v[1]; a[4 * q + 2] = v[2]; a[4 * q + 3] = v[3];
    }
    float A[3][3], V[3][3], R[2][3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {           // the y transform of the window's columns
      A[0][s] = d[s] - d[3 + s];
      A[1][s] = d[3 + s];
      A[2][s] = d[6 + s] - d[3 + s];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {           // phase (0,0): the x transform of its rows
      V[i][0] = A[i][0] - A[i][1];
      V[i][1] = A[i][1];
      V[i][2] = A[i][2] - A[i][1];
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {           // phase (1,0): the x transform of the two raw rows
      R[r][0] = d[3 * (1 + r)] - d[3 * (1 + r) + 1];
      R[r][1] = d[3 * (1 + r) + 1];
      R[r][2] = d[3 * (1 + r) + 2] - d[3 * (1 + r) + 1];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * i + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3 * i + j], V[i][j], acc[3 * i + j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int c = 0; c < 2; ++c) acc[9 + 2 * i + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[9 + i], A[i][1 + c], acc[9 + 2 * i + c], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[15 + 3 * r + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[12 + j], R[r][j], acc[15 + 3 * r + j], 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 2; ++c)
        acc[21 + 2 * r + c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[15], d[3 * (1 + r) + 1 + c], acc[21 + 2 * r + c], 0, 0, 0);
  };

  // ---- pipeline: LDS[ch & 1] = U of chunk ch | registers = U of chunk ch + 1, windows of the next two k-steps.  The loop body is two
  //      chunks (four k-steps: every register set and LDS buffer is a compile-time constant); Cin is padded to 16 with zero U.
  static_assert(TW_KC == 2, "the loop body below is written for two k-steps per chunk");
  float* const buf0 = Ul;
  float* const buf1 = Ul + TW_KC * TW_SLAB;
  load_u(0);
  load_win(0, win[0]);
  load_win(1, win[1]);
  commit_u(buf0);
  load_u(1);
  __syncthreads();
  for (int ks0 = 0; ks0 < nks; ks0 += 4) {
    const int ch = ks0 >> 1;
    load_win(ks0 + 2, win[2]);
    kstep(win[0], buf0);
    __builtin_amdgcn_sched_barrier(0);
    load_win(ks0 + 3, win[3]);
    kstep(win[1], buf0 + TW_SLAB);
    commit_u(buf1);
    load_u(ch + 2);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    load_win(ks0 + 4, win[0]);
    kstep(win[2], buf1);
    __builtin_amdgcn_sched_barrier(0);
    load_win(ks0 + 5, win[1]);
    kstep(win[3], buf1 + TW_SLAB);
    commit_u(buf0);
    load_u(ch + 3);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
  }

  // ---- epilogue: the output transform in-lane (A^T = [[1,1,0],[0,1,1]] on the 2-tap axes), the operand chain of conv_pipe's transposed
  //      branch, one 16-byte store per output row of the tile (16 neighbouring lanes join to 256-byte runs)
  const int Cout = p.cout_g;
  const float* osp = p.osp + (int64_t)b * Cout * p.oss;
  const float s1 = p.s1, g1 = p.g1, g2 = p.g2;
  const int oss = p.oss, css = p.css, cbs = p.cbs, b1s = p.b1s, b2s = p.b2s, s2s = p.s2s;
  const int y_plane = p.y_h * p.y_w;
  float* yb = p.y + ((int64_t)b * p.y_ch + p.y_coff) * y_plane;
  const int nrow = tok ? min(4, 2 * p.H + 1 - 2 * m0) : 0;     // valid output rows / columns of the tile: 4, or 1 on the ragged edge
  const int ncol = tok ? min(4, 2 * p.W + 1 - 2 * c0) : 0;     // (3 when H / W is odd)
  const int ybase = 2 * m0 * p.y_w + 2 * c0;
  const bool only_os = css == 0 && cbs == 0 && b1s == 0 && b2s == 0 && s2s == 0 && s1 == 1.f && g1 == 1.f && g2 == 1.f &&
                       __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.s2p[0])) == 0x3f800000;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int cg = 16 * cb + 4 * kq + r;
    const bool cok = cg < Cout;
    const int co = cok ? cg : 0;
    float row[4][4];       // [output row 2 a + py][output column 2 c + px]
    {
      float S[3][2];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) S[i][c] = acc[3 * i + c][r] + acc[3 * i + c + 1][r];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          row[2 * a][2 * c] = S[a][c] + S[a + 1][c];
          row[2 * a][2 * c + 1] = acc[9 + 2 * a + c][r] + acc[9 + 2 * (a + 1) + c][r];
          row[2 * a + 1][2 * c] = acc[15 + 3 * a + c][r] + acc[15 + 3 * a + c + 1][r];
          row[2 * a + 1][2 * c + 1] = acc[21 + 2 * a + c][r];
        }
    }
    const float os = osp[co * oss];
    if (only_os) {   // the up-convs of the path carry the demodulation scale only: one multiply per output
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) row[i][j] *= os;
    } else {
      const float cs = p.csp[co * css], cbv = p.cbp[co * cbs], b1 = p.b1p[co * b1s], b2 = p.b2p[co * b2s], sl2 = p.s2p[co * s2s];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = row[i][j] * os * cs + cbv + b1;
          v = (v > 0.f ? v : v * s1) * g1 + b2;
          row[i][j] = (v > 0.f ? v : v * sl2) * g2;
        }
    }
    if (!cok) continue;
    float* yc = yb + (int64_t)co * y_plane + ybase;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= nrow) continue;
      float* yr = yc + i * p.y_w;
      if (ncol == 4) {
        *reinterpret_cast<tw_f4u*>(yr) = tw_f4u{row[i][0], row[i][1], row[i][2], row[i][3]};
      } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < ncol) yr[j] = row[i][j];
      }
    }
  }
}

}  // namespace

// what the fused transposed Winograd kernel serves of a launch conv_front has filled (the output extent was checked by the transposed-mode
// normalisation): one group, Cin % 4 == 0, the style scale but no affine shift, 16-byte aligned weight image and output planes, 32-bit buffer offsets
bool tconvw_eligible(const ConvK& q) {
  if (q.G != 1 || q.Cin % 4 != 0 || q.KH != 3 || q.KW != 3) return false;
  if (q.wsh_cs != 0 || q.wc_cs != 0) return false;
  if (!vsp::aligned16(q.w) || !quad_planes_ok(q, false)) return false;
  if ((int64_t)q.Cin * q.H * q.W * 4 >= 0x7fffff00ll) return false;
  if ((int64_t)(q.Cin / 4) * TW_SLAB * 4 >= 0x7fffff00ll) return false;
  return true;
}

size_t tconvw_weight_floats(int cin, int cout) {
  return (size_t)((cout + 15) / 16) * (size_t)((cin + 3) / 4) * TW_SLAB;
}

int tconvw_weight_launch(float* U, const float* wp, int cin, int cout, float scale, hipStream_t stream) {
  const int nks = (cin + 3) / 4;
  const int64_t units = (int64_t)((cout + 15) / 16) * nks;
  tconvw_weight_kernel<<<(unsigned)((units + 3) / 4), 256, 0, stream>>>(U, wp, cin, cout, nks, units, scale);
  return VSP_OK;
}

// q.w = the U image (tconvw_weight_launch)
int tconvw_launch(const ConvK& q, hipStream_t stream) {
  TwPlan pl;
  pl.ntx = (q.W + 2) / 2;                       // ceil((W + 1) / 2) tiles of two positions
  const int nty = (q.H + 2) / 2;
  pl.ntiles = pl.ntx * nty;
  pl.nwn = (pl.ntiles + 63) / 64;
  pl.ncb = (q.cout_g + 15) / 16;
  pl.nks = q.Cin / 4;
  const int64_t nwg = (int64_t)q.B * pl.nwn * pl.ncb;
  if (nwg > 0x7fffffff) return vsp::fail(VSP_EINVAL, "conv_transpose2d_s2_wino: too many tiles");
  conv_tconv_wino_kernel<<<(unsigned)nwg, TW_THR, 0, stream>>>(q, pl);
  return VSP_OK;
}

}  // namespace vspconv

// The algebra of Winograd F(4x4, 3x3) as both fp32 forms use it (conv_wino4.hip: transform + GEMM pair; conv_wino4f.hip: fused in registers),
// stated once -- the conditioning fence (tests/wino_ref.py) models ONE set of points for both.
//
// Interpolation points 0, +-a, +-b, infinity with a = 3/4, b = 3/2 (not the textbook 0, +-1, +-2): every constant of B^T and A^T is a dyadic
// rational, exact in fp32 (the choice and its error figures: conv_wino4.hip header, tools/wino4_points.py).
//   B^T rows:  [a2b2, 0, -(a2+b2), 0, 1, 0]            (a2b2 = 81/64, a2+b2 = 45/16)
//              (d4 - b2 d2) +- a (d3 - b2 d1)           (b2 = 9/4)
//              (d4 - a2 d2) +- b (d3 - a2 d1)           (a2 = 9/16)
//              [0, a2b2, 0, -(a2+b2), 0, 1]
//   A^T rows:  [1, 1, 1, 1, 1, 0], [0, a, -a, b, -b, 0], [0, a2, a2, b2, b2, 0], [0, a3, -a3, b3, -b3, 1]
//   G rows  :  [64/81, 0, 0], [-128/243, -+32/81, -8/27], [32/243, +-16/81, 8/27], [0, 0, 1]      (U = G g G^T in fp64, rounded once)
// Winograd position = 6 xi + nu (row xi, column nu of the 6 x 6 transformed tile).
#pragma once
#include "conv_kernel.h"

namespace vspconv {

constexpr float W4_A = 0.75f, W4_B = 1.5f, W4_A2 = 0.5625f, W4_B2 = 2.25f, W4_A2B2 = 1.265625f, W4_SUM2 = 2.8125f;
constexpr float W4_A3 = 0.421875f, W4_B3 = 3.375f;

// One row of G against a 3-vector with the roundings written out: the first product rounded, the other two fused.  Left to the compiler's
// contraction the choice of the rounded product changes with the surrounding code -- and with it, now and then, the last bit of U.
__device__ __forceinline__ double w4_dot3(const double (&g)[3], double x, double y, double z) { return fma(g[2], z, fma(g[1], y, g[0] * x)); }

// U = G g G^T of the pair (ci, co) of the packed weights wp [tap][cin][cout] (zeros outside them): fp64 sums rounded once, u[position]
__device__ __forceinline__ void w4_weight_u(const float* __restrict__ wp, int cin, int cout, int ci, int co, float (&u)[36]) {
  const double Gm[6][3] = {{64.0 / 81.0, 0.0, 0.0},           {-128.0 / 243.0, -32.0 / 81.0, -8.0 / 27.0}, {-128.0 / 243.0, 32.0 / 81.0, -8.0 / 27.0},
                           {32.0 / 243.0, 16.0 / 81.0, 8.0 / 27.0}, {32.0 / 243.0, -16.0 / 81.0, 8.0 / 27.0},  {0.0, 0.0, 1.0}};
  const bool in = ci < cin && co < cout;
  double gk[3][3];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) gk[tap / 3][tap % 3] = in ? (double)wp[((int64_t)tap * cin + ci) * cout + co] : 0.0;
  double r[6][3];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int x = 0; x < 3; ++x) r[i][x] = w4_dot3(Gm[i], gk[0][x], gk[1][x], gk[2][x]);
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) u[6 * i + j] = (float)w4_dot3(Gm[j], r[i][0], r[i][1], r[i][2]);
}

__device__ __forceinline__ void w4_bt(const float (&d)[6], float (&o)[6]) {   // one 6-vector through B^T
  const float e1 = fmaf(-W4_B2, d[2], d[4]), o1 = fmaf(-W4_B2, d[1], d[3]);
  const float e2 = fmaf(-W4_A2, d[2], d[4]), o2 = fmaf(-W4_A2, d[1], d[3]);
  o[0] = fmaf(W4_A2B2, d[0], fmaf(-W4_SUM2, d[2], d[4]));
  o[1] = fmaf(W4_A, o1, e1);
  o[2] = fmaf(-W4_A, o1, e1);
  o[3] = fmaf(W4_B, o2, e2);
  o[4] = fmaf(-W4_B, o2, e2);
  o[5] = fmaf(W4_A2B2, d[1], fmaf(-W4_SUM2, d[3], d[5]));
}

// Y = A^T M A of one tile and channel in two steps: Z = A^T M down the rows (xi) -- m(position) reads M wherever the caller keeps it --,
// then one output row Y[i] = Z[i] A along the columns (nu), so that a caller may finish and store row i before it forms row i + 1
template <class M>
__device__ __forceinline__ void w4_at_rows(M&& m, float (&z)[4][6]) {
#pragma unroll
  for (int nu = 0; nu < 6; ++nu) {
    const float m0 = m(nu), m1 = m(6 + nu), m2 = m(12 + nu), m3 = m(18 + nu), m4 = m(24 + nu), m5 = m(30 + nu);
    const float s1 = m1 + m2, d1 = m1 - m2, s2 = m3 + m4, d2 = m3 - m4;
    z[0][nu] = m0 + s1 + s2;
    z[1][nu] = fmaf(W4_B, d2, W4_A * d1);
    z[2][nu] = fmaf(W4_B2, s2, W4_A2 * s1);
    z[3][nu] = fmaf(W4_B3, d2, fmaf(W4_A3, d1, m5));
  }
}
__device__ __forceinline__ void w4_at_col(const float (&zi)[6], float (&y)[4]) {
  const float s1 = zi[1] + zi[2], d1 = zi[1] - zi[2], s2 = zi[3] + zi[4], d2 = zi[3] - zi[4];
  y[0] = zi[0] + s1 + s2;
  y[1] = fmaf(W4_B, d2, W4_A * d1);
  y[2] = fmaf(W4_B2, s2, W4_A2 * s1);
  y[3] = fmaf(W4_B3, d2, fmaf(W4_A3, d1, zi[5]));
}

}  // namespace vspconv

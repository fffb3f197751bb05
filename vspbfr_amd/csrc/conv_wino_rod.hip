// Winograd F(2x2, 3x3), row-owner form (conv_wino_ro.hip) for the DILATION GROUPS of the SMART layers: up to four groups over one shared
// input, dilation = padding = 1, 2, 4 or 8 per group (reference models/RestoreNet.py:205-215, 604-668).
//
// Geometry of conv_wino.hip's dilated variant: row-polyphase -- a workgroup owns the rows ry, ry + d, ... of one residue class
// (consecutive patch rows) and a DENSE run of 16 columns with a halo of d; its 8 tile columns are the d column residues x 8 / d tile
// positions (tile tx: residue tx % d, first column residue + 2 d (tx / d)), the window columns lie d apart.  What changes against the
// task-list kernel is what conv_wino_ro.hip changes: wave w owns the positions (xi, nu) = (w / 2, 2 (w % 2) + {0, 1}) and computes its own B
// fragments from the staged patch (two window rows x four words d apart per N-block: ds_read_b32), no V image, no transform tasks;
// patch rows staged as aligned 16-byte segments (columns ox0 - max(d, 4) ...); scale / affine at commit time.
// LDS banks (4-byte reads: bank = dword mod 32, 32-lane groups = two channels x (8 tile columns x 2 tile rows)): the tile columns of a
// group occupy dwords c0(tx) in [0, 16) -- every second one for d = 1, pairs for d = 2, ... -- so the row pitch puts the second tile row
// 16 banks away (pitch == 8 mod 16: 24, or 40 for the 32-column rows of d = 8) and the channel pitch shifts the second channel by d
// (pitch == d mod 32): the four 8-dword sets of an access tile the 32 banks.
#include "conv_wino2.h"

namespace vspconv {

namespace {

constexpr int RD_NTHR = 512;
constexpr int RD_IVC = WINO2_RO_IVC;

template <int MBW>
struct RDG : Wino2Tile<MBW> {
  using T = Wino2Tile<MBW>;
  static constexpr int TLX = 8;
  static constexpr int TLY = T::NTILE / TLX;
  static constexpr int PR = 2 * TLY + 2;
  static constexpr int NLD = (PR * 8 + 63) / 64;                       // wave loads per channel plane at the widest rows (d = 8: 8 segments)
  static constexpr int PPMAX = (PR * 40 + 1 + 31) / 32 * 32 + 8;      // largest channel pitch (d = 8)
  static constexpr int LDS_P = RD_IVC * PPMAX;                        // floats per sub-stage buffer
  static constexpr int LDS_FLOATS = 2 * LDS_P > T::LDS_M ? 2 * LDS_P : T::LDS_M;
};

template <int MBW>
__global__ __launch_bounds__(RD_NTHR, 4) void conv_wino_rod_kernel(const ConvK p) {
  using Gm = RDG<MBW>;
  constexpr int NBW = Gm::NBW, WCO = Gm::WCO, TLX = Gm::TLX, TLY = Gm::TLY, PR = Gm::PR;
  constexpr int LDS_P = Gm::LDS_P, UF = Gm::UF, NLD = Gm::NLD, IVC = RD_IVC, KS = 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* Pl = smem;   // 2 x [IVC][channel pitch of this group]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, kq = lane >> 4;
  // ---- work order (conv_wino2.h): region-major for shared-input dilation groups (order 4), pixel-tile-major (1) or dispatch order
  int b = blockIdx.z, bx = blockIdx.x, by = blockIdx.y;
  int reg_ry = -1, reg_ty = 0, reg_tx = 0;
  if (p.wg_order == 4) decode_region_major(p, xcd_linear_id(), b, by, reg_ry, reg_ty, reg_tx);
  else if (p.wg_order) decode_pixel_major(xcd_linear_id(), b, bx, by);
  const int g = by / p.co_tiles, ct = by - g * p.co_tiles;
  const int d = p.dil[g];                                       // 1, 2, 4 or 8
  int ry, tx_i, ty_i;
  if (!wino2_tile<TLX, TLY>(p, d, bx, reg_ry, reg_ty, reg_tx, ry, ty_i, tx_i)) return;
  const int oy0 = ty_i * (2 * TLY), ox0 = tx_i * (2 * TLX);     // sub-image rows, image columns
  const int hl = d > 4 ? d : 4;                                 // staged halo: whole segments
  const int SEG = (2 * TLX + 2 * hl) / 4;                       // 6 (d <= 4) or 8 segments per row
  const int PCP = d == 8 ? 40 : 24;                             // row pitch (== 8 mod 16)
  const int PPITCH = (PR * PCP + 1 + 31) / 32 * 32 + d;         // channel pitch (== d mod 32)
  const int co0 = ct * WCO;
  const int chw = p.H * p.W;
  const float* xb = p.x + (int64_t)b * p.x_ch * chw;
  const int nstage = (p.Cin + IVC - 1) / IVC;
  const int nchunk4 = (p.Cin + 3) / 4;

  // ---- patch staging: one channel plane per wave and sub-stage; a lane owns segment (row, seg) = (l / SEG, l % SEG), l = lane + 64 i
  //      (lanes past the plane repeat segment 0: same address, same value)
  int p_voff[NLD], p_dst[NLD];
  unsigned p_ok = 0;
#pragma unroll
  for (int i = 0; i < NLD; ++i) {
    const int l = lane + 64 * i;
    const bool live = l < PR * SEG;
    const int r = live ? l / SEG : 0, sg = live ? l - r * SEG : 0;
    const int sy = oy0 - 1 + r, ix = ox0 - hl + 4 * sg;
    const int iy = sy * d + ry;
    const bool in = sy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
    p_voff[i] = in ? (iy * p.W + ix) * 4 : 0x7ffffff0;   // padding: a lane offset past the resource, the load returns zeros
    p_ok |= in ? (1u << i) : 0u;
    p_dst[i] = 1 + r * PCP + 4 * sg;
  }
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(xb), 0, p.x_ch * chw * 4, 0x00020000);   // this image (the range check compares the lane offset with size - scalar offset)
  f32x4v preg[NLD];
  auto load_plane = [&](int j) { wino2_load_plane<NLD>(xrsrc, p_voff, j, nstage, wave, p.Cin, chw, preg); };
  const float* wt_b = p.wtp + b * p.wt_bs;
  const float* wc_b = p.wcp + b * p.wc_bs;
  const bool affine = p.wc_cs != 0 || p.wsh_cs != 0 || p.wc_bs != 0;
  auto commit_plane = [&](float* Pdst, int j) { wino2_commit_plane<NLD>(p, wt_b, wc_b, affine, Pdst, PPITCH, j, wave, p_ok, p_dst, preg); };

  // ---- U fragments (wino2_load_u_half): resource = this channel tile's slice
  const float* utile = p.w + ((int64_t)g * p.co_tiles + ct) * nchunk4 * (8 * 64 * UF);
  const __amdgpu_buffer_rsrc_t ursrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(utile), 0, nchunk4 * (8 * 64 * UF) * 4, 0x00020000);
  const int u_voff = ((wave * 2 * 64 + lane) * MBW) * 4;
  auto load_u = [&](int c, float (&u)[UF]) {
    wino2_load_u_half<MBW>(ursrc, u_voff, c, nchunk4, 0, u);
    wino2_load_u_half<MBW>(ursrc, u_voff, c, nchunk4, 1, u);
  };

  // ---- this wave's row of the transformed tile
  const int xi = wave >> 1, nuh = wave & 1;
  const int rA = xi == 0 ? 0 : (xi == 2 ? 2 : 1);
  const int rB = xi == 0 ? 2 : (xi == 1 ? 2 : (xi == 2 ? 1 : 3));
  const float sgn = xi == 1 ? 1.f : -1.f;
  // lane's window origin: tile = lr + 16 nb -> (ty, tx) = (2 nb + lr / 8, lr % 8); first window column (patch coordinates) hl - d + c0(tx)
  const int wty = lr >> 3, wtx = lr & 7;
  const int c0 = (wtx % d) + 2 * d * (wtx / d);
  const int nbstep = 4 * PCP;                                   // the next N-block lies two tile rows down
  const int woffA = kq * PPITCH + (2 * wty + rA) * PCP + 1 + (hl - d) + c0;
  const int woffB = kq * PPITCH + (2 * wty + rB) * PCP + 1 + (hl - d) + c0;
  auto fragments = [&](const float* Psrc, int ks, float (&bv)[2][NBW]) {
    const float* base = Psrc + ks * (4 * PPITCH);
#pragma unroll
    for (int n0 = 0; n0 < NBW; n0 += 2) {
      float wa[2][4], wb[2][4];
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          wa[n][k] = base[woffA + (n0 + n) * nbstep + k * d];
          wb[n][k] = base[woffB + (n0 + n) * nbstep + k * d];
        }
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const float w0 = fmaf(wb[n][0], sgn, wa[n][0]), w1 = fmaf(wb[n][1], sgn, wa[n][1]);
        const float w2 = fmaf(wb[n][2], sgn, wa[n][2]), w3 = fmaf(wb[n][3], sgn, wa[n][3]);
        bv[0][n0 + n] = nuh ? w2 - w1 : w0 - w2;
        bv[1][n0 + n] = nuh ? w1 - w3 : w1 + w2;
      }
    }
  };

  f32x4 acc[2][MBW][NBW];
#pragma unroll
  for (int pp = 0; pp < 2; ++pp)
#pragma unroll
    for (int mb = 0; mb < MBW; ++mb)
#pragma unroll
      for (int nb = 0; nb < NBW; ++nb) acc[pp][mb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto multiply_pp = [&](int pp, const float (&u)[UF], const float (&bv)[2][NBW]) {
#pragma unroll
    for (int mb = 0; mb < MBW; ++mb)
#pragma unroll
      for (int nb = 0; nb < NBW; ++nb)
        acc[pp][mb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(u[pp * MBW + mb], bv[pp][nb], acc[pp][mb][nb], 0, 0, 0);
  };

  // ---- pipeline (conv_wino_ro.hip, barrier period 1)
  float ua[UF], ub[UF];
  float bva[2][NBW], bvb[2][NBW];
  load_u(0, ua);
  load_plane(0);
  commit_plane(Pl, 0);
  load_plane(1);
  __syncthreads();
  constexpr int SB = 0x2 | 0x4 | 0x80 | 0x100 | 0x200;   // VALU, SALU, LDS may cross; MFMAs and vector-memory instructions may not
  for (int j = 0; j < nstage; ++j) {
    const float* Pcur = Pl + (j & 1) * LDS_P;
    float* Pnxt = Pl + ((j + 1) & 1) * LDS_P;
    fragments(Pcur, 0, bva);
    load_u(j * KS + 1, ub);
    __builtin_amdgcn_sched_barrier(SB);
    multiply_pp(0, ua, bva);
    __builtin_amdgcn_sched_barrier(SB);
    commit_plane(Pnxt, j + 1);
    load_plane(j + 2);
    __builtin_amdgcn_sched_barrier(SB);
    fragments(Pcur, 1, bvb);
    multiply_pp(1, ua, bva);
    __builtin_amdgcn_sched_barrier(SB);
    load_u(j * KS + 2, ua);
    __builtin_amdgcn_sched_barrier(SB);
    multiply_pp(0, ub, bvb);
    __builtin_amdgcn_sched_barrier(SB);
    multiply_pp(1, ub, bvb);
    __builtin_amdgcn_sched_barrier(SB);
    __syncthreads();
  }

  // ---- epilogue (conv_wino2.h); the pixels of a tile lie d apart
  wino2_epilogue<RD_NTHR, MBW, NBW, TLX, Gm::ETILE, Gm::EMB, Gm::EP>(p, smem, acc, b, g, co0, oy0, ox0, d, ry, tid, wave, lr, kq);
}

template <int MBW>
int launch_rod(ConvK q, hipStream_t stream) {
  using Gm = RDG<MBW>;
  static vsp::LdsAttrOnce attr;
  const size_t lds = (size_t)Gm::LDS_FLOATS * sizeof(float);
  if (int rc = attr.ensure(reinterpret_cast<const void*>(conv_wino_rod_kernel<MBW>), (int)lds, "conv2d_winograd (row-owner, dilation groups)")) return rc;
  q.co_tiles = (q.cout_g + Gm::WCO - 1) / Gm::WCO;
  int blocks = wino2_group_blocks(q, Gm::TLX, Gm::TLY);
  q.wg_order = q.H * q.W <= 1024 ? 1 : 0;
  if (q.G >= 2 && q.x_gs == 0 && !(q.dbg & 0x800000)) wino2_region_major(q, Gm::TLY, Gm::TLX, &blocks);
  dim3 grid((unsigned)blocks, (unsigned)(q.co_tiles * q.G), (unsigned)q.B);
  conv_wino_rod_kernel<MBW><<<grid, RD_NTHR, lds, stream>>>(q);
  return VSP_OK;
}

}  // namespace

// dilation-group launches the row-owner form serves: dilations 1, 2, 4, 8, rows of whole 16-byte segments, 32 or more channels per group
bool wino_rod_eligible(const ConvK& q) {
  for (int g = 0; g < q.G; ++g)
    if (q.dil[g] != 1 && q.dil[g] != 2 && q.dil[g] != 4 && q.dil[g] != 8) return false;
  return q.cout_g > 16 && wino2_rows_are_segments(q);
}

int wino_rod_launch(ConvK q, int mbw, hipStream_t stream) { return mbw == 4 ? launch_rod<4>(q, stream) : launch_rod<2>(q, stream); }

}  // namespace vspconv

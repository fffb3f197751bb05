/*
 * vspbfr_hip.h -- C ABI of libvspbfr_hip.so: the MI355X (gfx950) device kernels behind the VSPBFR
 * restoration inference path.
 *
 * Boundary contract
 * -----------------
 *  - plain C: device pointers, sizes, scalars and an opaque stream handle (a hipStream_t); no torch types.
 *  - every entry point ENQUEUES work on `stream` and returns immediately (no host sync), exactly like the
 *    reference's two native ops which launch on at::cuda::getCurrentCUDAStream()
 *    (reference op/fused_bias_act_kernel.cu:73, op/upfirdn2d_kernel.cu:215).
 *  - tensors are dense, row-major, fp32 (VSP_F32).  Pointers are borrowed; outputs are caller-allocated
 *    (the reference allocates with torch::empty_like / at::empty inside the op -- the Python mirror in
 *    vspbfr_amd/op does that allocation so that the ABI stays torch-free).
 *  - return value: 0 on success, a negative VSP_E* code otherwise; vsp_last_error() returns a
 *    thread-local human-readable message.  The Python mirror raises RuntimeError (what TORCH_CHECK raises
 *    in the reference: op/fused_bias_act.cpp:10-16, op/upfirdn2d.cpp:9-15).
 *
 * What each entry point replaces in the reference is cited on the declaration.
 */
#ifndef VSPBFR_HIP_H
#define VSPBFR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSP_ABI_VERSION 4

#define VSP_OK 0
#define VSP_EINVAL (-1)   /* bad argument (shape / null pointer / unsupported combination) */
#define VSP_ELAUNCH (-2)  /* hipLaunchKernel / HIP runtime failure */
#define VSP_ENOTSUP (-3)  /* valid request that this build has no kernel for */

typedef void* vsp_stream_t; /* hipStream_t; NULL = the default stream */

int vsp_abi_version(void);
const char* vsp_last_error(void);
/* number of HIP devices visible, or a negative VSP_E* code (used by the loader's self-check). */
int vsp_device_count(void);
/* sizeof of an ABI struct (0 = vsp_fir_epilogue, 1 = vsp_conv_params, 2 = vsp_gemm_params,
 * 3 = vsp_tacc_block, 4 = vsp_tacc_chain_params, 5 = vsp_conv_wgrad_params, 6 = vsp_degrade_item, 7 = vsp_resample_item,
 * 8 = vsp_face_item, 9 = vsp_face_tile, 10 = vsp_face_aa_item, 11 = vsp_jpeg_item, 12 = vsp_jpeg_dec_item,
 * 13 = vsp_resample_dst, 14 = vsp_png_item, 15 = vsp_det_src, 16 = vsp_det_face,
 * 17 = vsp_sr_item): lets a binding in
 * another language check its own struct layout when it loads the library. */
int vsp_struct_size(int which);

/* ------------------------------------------------------------------------------------------------
 * fused bias + activation  -- replaces `fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale)`
 * (reference op/fused_bias_act.cpp:18-31, kernel op/fused_bias_act_kernel.cu:19-65).
 *   out[i] = f(x[i] + bias[(i / step_b) % size_b]) * scale
 *   act*10+grad: 10,11 -> f = identity; 30 -> leaky-relu(alpha); 31 -> (ref[i] > 0 ? v : v*alpha);
 *   12, 32 -> 0.  bias == NULL means "no bias" (reference: empty tensor), ref likewise.
 * n = number of elements; step_b = product of dims after dim 1 (1 for 2-D input).
 * ---------------------------------------------------------------------------------------------- */
int vsp_fused_bias_act_f32(float* out, const float* x, const float* bias, const float* ref, int64_t n,
                           int step_b, int size_b, int act, int grad, float alpha, float scale,
                           vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * upfirdn2d -- replaces `upfirdn2d_op.upfirdn2d(input[major,H,W,minor], kernel[kh,kw], up_x, up_y,
 * down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)` (reference op/upfirdn2d.cpp:17-31, kernels
 * op/upfirdn2d_kernel.cu:49-207, CPU definition op/upfirdn2d.py:365-406).
 * out dims: out_h = (in_h*up_y + pad_y0 + pad_y1 - kh + down_y) / down_y (likewise out_w); the caller
 * allocates out[major, out_h, out_w, minor].  Negative pads crop, as in the reference.
 *
 * The optional epilogue (all pointers may be NULL) fuses what the reference runs as separate ops right
 * after the blur of an up-sampling StyledConv (models/RestoreNet.py:599-603, e4e stylegan2/model.py:337-341):
 *   v = fir(x)
 *   v = v * plane_scale[plane]                 (per (b,c) demodulation coefficient)
 *   v = v + noise[b, oy, ox] * noise_w[0]      (NoiseInjection; noise is [B,1,out_h,out_w])
 *   v = lrelu(v + act_bias[c], slope) * gain   (FusedLeakyReLU; only if act != 0)
 *   v = v + res1[...] + res2[...]              (same layout as out)
 * `channels` gives c = plane % channels, b = plane / channels (minor must be 1 when an epilogue is used).
 * ---------------------------------------------------------------------------------------------- */
typedef struct vsp_fir_epilogue {
  const float* plane_scale; /* [major] or NULL */
  const float* noise;       /* [major/channels, out_h, out_w] or NULL */
  const float* noise_w;     /* device scalar, required iff noise != NULL */
  const float* act_bias;    /* [channels] or NULL (treated as 0) */
  const void* res1;         /* [major, out_h, out_w] or NULL; element type of out (float, or bf16 with vsp_upfirdn2d_bf16) */
  const void* res2;         /* likewise */
  int channels;             /* C (>=1) */
  int act;                  /* 0 none, 1 leaky-relu */
  float slope;              /* 0.2 */
  float gain;               /* sqrt(2) */
  int flags;                /* VSP_FIR_SEPARABLE: the LAST tap is not zero, kernel[kh-1][kw-1] != 0, and
                             *   kernel[ky][kx] == kernel[ky][kw-1] * kernel[kh-1][kx] / kernel[kh-1][kw-1]   for every ky, kx
                             * (an outer product written with its last row and column, as every blur of the path is: make_kernel([1,3,3,1]),
                             * models/RestoreNet.py:38-48) -- the caller's promise.  The kernels work on the flipped taps and DIVIDE by that
                             * corner: an outer product whose last tap is zero (outer([1,3,3,0], .)) must not be flagged.  The blur kernels
                             * may then run a row pass and a column pass (8 multiply-adds per output instead of 16); the result differs from
                             * the 2-D form by rounding only.  0 = general taps. */
} vsp_fir_epilogue;
#define VSP_FIR_SEPARABLE 1

int vsp_upfirdn2d_f32(float* out, const float* x, const float* kernel, int major, int in_h, int in_w,
                      int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0,
                      int pad_x1, int pad_y0, int pad_y1, const vsp_fir_epilogue* epi /* may be NULL */,
                      vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * conv2d as an fp32-MFMA implicit GEMM -- replaces the conv2d_gradfix.conv2d / conv_transpose2d / F.conv2d
 * calls of the path (reference op/conv2d_gradfix.py:22-92, models/RestoreNet.py:125-131,373-416,510-553,
 * e4e/models/stylegan2/model.py:116,259-274, e4e/models/encoders/helpers.py:98-113) together with the
 * element-wise work the reference wraps around them (modulation, demodulation, bias, noise, activation,
 * residual adds, eval-mode BatchNorm, PReLU).
 *
 *   acc[b,co,oy,ox] = sum_{ci,ky,kx} Wp[g][ky*KW+kx][ci][co_g] *
 *                     xin(b, ci, oy*stride_y + ky*dil[g] - pad[g], ox*stride_x + kx*dil[g] - pad[g])
 *   xin(b,ci,iy,ix) = 0 outside the image, else x[b,ci,iy,ix] * in_scale[b*in_scale_bstride + ci] + in_shift[ci]
 * with g = co / cout_g (output-channel groups: either groups that differ only in dilation/padding and share the
 * input -- the four dilated branches of SMART_layer in one launch -- or true convolution groups with their own
 * input-channel slice, see x_group_stride), then per output element, in this order:
 *   v = acc * out_scale[b*Cout + co]                     (demodulation, models/RestoreNet.py:376-379)
 *   v = v * ch_scale[co] + ch_bias[co]                   (conv bias / folded eval BatchNorm)
 *   act1: v = lrelu(v + bias1[co], slope1) * gain1       (FusedLeakyReLU of `fusion`, RestoreNet.py:1176-1177)
 *   v = v + noise[b,oy,ox] * noise_w[0]                  (NoiseInjection, RestoreNet.py:564-569)
 *   act2: 1: v = lrelu(v + bias2[co], slope2) * gain2    (FusedLeakyReLU `activate`)
 *         2: v = v >= 0 ? v : v * prelu[co]              (nn.PReLU)
 *   v = v + res1[b,co,oy,ox] + res2[b,co,oy,ox]
 *   y[b, y_coff + co, oy*osy + ooy, ox*osx + oox] = v    (y has y_ch channels, y_h x y_w pixels)
 * The output stride/offset (osy, osx, ooy, oox) lets a stride-2 transposed conv run as four sub-pixel phase
 * convolutions writing one (2H+1)x(2W+1) tensor (same MACs as conv_transpose2d).
 * Wp is the launch's weight, packed by the host once at model-load time:
 *   Wp[g][tap][ci][co_g], co_g contiguous (see hip_ops.pack_weight in vspbfr_amd/hip_ops.py).
 * ---------------------------------------------------------------------------------------------- */
typedef struct vsp_conv_params {
  const float* x;  /* [B, Cin, H, W] */
  const float* w;  /* packed [G][KH*KW][Cin][cout_g] */
  float* y;        /* [B, y_ch, y_h, y_w] */
  int B, Cin, H, W;
  int G, cout_g;   /* Cout = G * cout_g */
  int OH, OW;      /* number of output positions computed per image */
  int KH, KW;
  int stride_y, stride_x;
  int dil[4];      /* per group */
  int pad_y[4];    /* per group */
  int pad_x[4];    /* per group */
  int y_ch, y_coff, y_h, y_w;
  int osy, osx, ooy, oox;
  /* prologue */
  const float* in_scale; /* NULL or [.., Cin]; grouped input (x_group_stride > 0): [.., x_ch], group g reads [g * x_group_stride, + Cin) */
  int in_scale_bstride;  /* Cin for per-sample styles, 0 for per-channel constants */
  const float* in_shift; /* NULL or [Cin] */
  /* epilogue */
  const float* out_scale; /* NULL or [B, Cout] */
  const float* ch_scale;  /* NULL or [Cout] */
  const float* ch_bias;   /* NULL or [Cout] */
  int act1;               /* 0 none, 1 lrelu */
  const float* bias1;     /* NULL or [Cout] */
  float slope1, gain1;
  const float* noise;     /* NULL or [B, OH, OW] */
  const float* noise_w;   /* device scalar */
  int act2;               /* 0 none, 1 lrelu, 2 prelu */
  const float* bias2;     /* NULL or [Cout] */
  const float* prelu;     /* [Cout] when act2 == 2 */
  float slope2, gain2;
  const float* res1;      /* NULL or same layout as the y region written (see res_* below) */
  const float* res2;
  int res_ch, res_coff;   /* residual tensors are [B, res_ch, y_h, y_w], read at channel res_coff + co */
  int tile_hint;          /* 0 = let the library choose; n > 0 = configuration n-1, an error if it does not fit (tests / tuning);
                             n < 0 = prefer configuration -n-1, fall back to the library's choice if it does not fit */
  /* grouped input (true grouped convolution, e.g. the 18 map2style heads of the e4e encoder run as one launch per stage):
   * x has x_ch channels per image (0 = Cin) and group g reads channels [g*x_group_stride, g*x_group_stride + Cin).
   * x_group_stride = 0: all groups read the same Cin channels (the dilation groups of SMART_layer).  With G > 4 every
   * group uses dil[0] / pad_y[0] / pad_x[0]. */
  int x_ch, x_group_stride;
  /* transposed = 1: y = conv_transpose2d(xin, W, stride 2, padding 0) for a 3x3 kernel in ONE launch (all four
   * sub-pixel phases; reference models/RestoreNet.py:530-532, e4e stylegan2/model.py:259).  w is the ordinary packed
   * [1][9][Cin][Cout] weight (W[co][ci][ky][kx], not flipped); y must be [B, y_ch, 2H+1, 2W+1]; KH = KW = 3, G = 1;
   * stride / dilation / padding / OH / OW / os* / oo* fields are ignored; prologue scaling and the epilogue's
   * per-channel terms apply, noise and residuals are not available (they follow the blur in the reference). */
  int transposed;
  /* io_bf16 = 1 (vsp_conv2d_bf16 only): x, y, res1 and res2 hold bf16 elements (raw 16-bit words, same dense NCHW shapes) --
   * the bf16-ACTIVATION configuration of BASELINE configs[2]: 2 B per element through HBM instead of 4.  Every other operand
   * (noise, scales, biases) and the accumulation stay fp32; y is rounded to nearest even once, after the epilogue chain. */
  int io_bf16;
  /* dil_by_input_quarter = 1 (vsp_conv2d_f32 only): the DATA GRADIENT of four dilated branches over one input (the SMART / LargeConv
   * layers, reference models/RestoreNet.py:205-215, 742-750) in one pass:  y = sum_q conv(x[:, q Cin/4 : (q+1) Cin/4], W_q, dil[q]),
   * pad = dil.  G = 4 and x_group_stride = 0 as in the forward dilation-group call, but the four "groups" are the four blocks of
   * cout_g output channels of ONE convolution over all Cin input channels (w = [4][9][Cin][cout_g], cout_g <= 16 per launch row),
   * and dil[q] / pad[q] belong to input-channel quarter q.  3x3, stride 1, Cin a multiple of 16; served by the pipelined kernels
   * only (VSP_ENOTSUP when no configuration fits). */
  int dil_by_input_quarter;
  /* w_bstride != 0 (vsp_conv2d_bf16 with io_bf16 = 1 only; every other entry requires 0): PER-IMAGE weights -- image b reads the weight set at
   * (char*)w + b * w_bstride (bytes, a multiple of 16), each in the layout of vsp_conv2d_bf16.  This is the reference's own "fused" modulated
   * convolution (models/RestoreNet.py:381-416: weight * style per sample): vsp_modulate_weight_bf16 builds bf16(W * style[b]) once per layer and
   * batch, in_scale / in_shift must then be NULL, and the kernel stages bf16 pixels into LDS with no arithmetic at all. */
  int64_t w_bstride;
} vsp_conv_params;

int vsp_conv2d_f32(const vsp_conv_params* p, vsp_stream_t stream);
/* Number of tile configurations compiled in, and a description of configuration i ("64x256 ..."). */
/* The same convolution contract for 3x3 / stride 1 / padding = dilation layers (G = 1, or up to four dilation groups over
 * one shared input: x_group_stride = 0) through Winograd F(2x2,3x3); a dilation d is served as d*d polyphase sub-images.
 * `w` must hold the TRANSFORMED weights U = G g G^T (G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]) in the kernel's
 * fragment order.  With CK = vsp_conv2d_winograd_chunk() input channels per chunk, MB = vsp_conv2d_winograd_mbw(cout_g)
 * 16-channel blocks per workgroup, Cin zero-padded to a multiple of CK and cout_g to a multiple of 16*MB:
 *     w[((((((g * ntile + tile) * nchunk + chunk) * 8 + wave) * 2 + pp) * 64 + lane) * MB + mb]
 *         = U_g[position 2*wave + pp][ci = CK*chunk + (lane >> 4)][co = 16*MB*tile + 16*mb + (lane & 15)]
 * (a wave owns two Winograd positions; its A fragments of one position and chunk are one contiguous run: a wave-wide load reads
 * consecutive memory).
 * Every prologue / epilogue field of vsp_conv_params keeps its meaning.  tile_hint names the kernel FORM (tests / tuning): 0 = the
 * library chooses; 1 = task list (conv_wino.hip), 2 = row owner (conv_wino_ro.hip / conv_wino_rod.hip), 3 = register-resident U with
 * polyphase staging (conv_wino_rs.hip: Cin <= 64, W % 4 == 0, no in_shift -- the 64 -> 4 x 16 dilation groups of the SMART layers,
 * reference models/RestoreNet.py:179-244); a named form that does not serve the launch returns VSP_ENOTSUP.  16 multiplies per 2x2
 * output tile instead of 36; fp32 error ~1e-6 relative on top of the direct kernel's summation-order noise. */
int vsp_conv2d_winograd_f32(const vsp_conv_params* p, vsp_stream_t stream);
int vsp_conv2d_winograd_chunk(void);
int vsp_conv2d_winograd_mbw(int cout_g);
/* The same contract through Winograd F(4x4,3x3) for the DEEP stride-1 3x3 layers (one group, dilation 1, padding 1, no in_shift;
 * Cin a multiple of 4, H and W multiples of 4, dense 16-byte aligned output / noise / residual planes: VSP_ENOTSUP otherwise --
 * reference layers models/RestoreNet.py:213-244,410-416, e4e/models/stylegan2/model.py:268-276 at 256 / 512 channels): 36 multiplies
 * per 4x4 output tile instead of 144.  Two launches: the input transform V = B^T d B (in_scale applied) into `work`
 * (vsp_conv2d_winograd4_work_floats(p) floats, fragment order of the GEMM), then a barrier-free GEMM with both operands fetched from
 * L2 straight into MFMA fragments and the fused epilogue of vsp_conv2d_f32.  Interpolation points 0, +-3/4, +-3/2, infinity: all
 * transform constants are dyadic, fp32 error = the direct kernel's (rms 1.5e-6 at unit scale).  `w` = vsp_winograd4_weight_f32:
 *     w[((((tile * nchunk + chunk) * 12 + wave) * 3 + q) * 64 + lane) * 4 + mb]
 *         = U[position 3*wave + q][ci = 4*chunk + (lane >> 4)][co = 64*tile + 16*mb + (lane & 15)],   U = G g G^T
 * (one wave-wide 16-byte load = 1 KiB of consecutive memory). */
int vsp_conv2d_winograd4_f32(const vsp_conv_params* p, float* work, size_t work_floats, vsp_stream_t stream);
/* Winograd F(4x4,3x3), FUSED form (round 5, conv_wino4f.hip): the layer class of vsp_conv2d_winograd4_f32 (3x3, stride 1, fp32, style scale
 * `in_scale` but no `in_shift`, dense same-size output) without a work buffer -- the input transform runs in registers in the MFMA's
 * fragment layout, the transformed input never exists in memory.  Serves Cin % 8 == 0 (<= 512), W >= 16 and
 *   - one group with padding = dilation in {1, 2, 4, 8}, H and W multiples of 4 x dilation: dilation 1 = the 32 / 64-channel layers on maps
 *     >= 128^2 (reference e4e/models/stylegan2/model.py:268-276, models/RestoreNet.py:421-555), where the two-kernel form's V round trip
 *     costs more than it saves; a dilated layer runs on its polyphase sub-images (tiles of 4 x 4 outputs `dilation` apart, windows read
 *     from an LDS-staged region);
 *   - G = 2..4 dilation groups over ONE shared input (x_group_stride = 0; the SMART branches models/RestoreNet.py:179-244), each group's
 *     geometry as above, in one launch: group g writes channels y_coff + g * cout_g ..., and every per-channel operand (out_scale, ch_scale,
 *     biases, prelu) and the residuals are indexed g * cout_g + channel -- the convention of vsp_conv2d_f32 for G > 1.
 * `w` = vsp_winograd4f_weight_f32's output, per group and the groups one after the other: U = G g G^T (the same 36 values per (ci, co) as
 * vsp_winograd4_weight_f32) in the order
 * [co / 32][ci / 4][position pair 18][lane 64][4]: lane = 16 (ci % 4) + (co % 16), element e = position 2 pp + (e >> 1), co block (e & 1).
 * VSP_ENOTSUP for a launch it does not serve (the caller falls back to vsp_conv2d_winograd_f32). */
size_t vsp_winograd4f_weight_floats(int cin, int cout);
int vsp_winograd4f_weight_f32(float* U, const float* wp, int cin, int cout, vsp_stream_t stream);
int vsp_conv2d_winograd4f_f32(const vsp_conv_params* params, vsp_stream_t stream);

/* The stride-2 transposed 3x3 convolution (`transposed` = 1: the launch of vsp_conv2d_f32's transposed mode, same operands, output extents,
 * y_coff and epilogue chain) as a fused Winograd F(2x2,2x2) phase kernel (conv_tconv_wino.hip): a tile of 2 x 2 positions = 4 x 4 outputs takes
 * 9 + 6 + 6 + 4 = 25 products per (ci, co) where the direct form takes 36; every transform constant is 0 or +-1.  Serves one group, fp32,
 * Cin % 4 == 0, the style scale `in_scale` but no `in_shift`, 16-byte aligned output planes.  VSP_ENOTSUP for a launch it does not serve:
 * nothing is written and the caller falls back to vsp_conv2d_f32.
 * `w` = vsp_tconvw_weight_f32's output: the 16 distinct transformed weights the 25 products read (g_0 = tap 2, g_1 = tap 2 + tap 0, g_2 = tap 0
 * on a 2-tap axis; fp64 sums of the packed weights times `scale`, rounded once) as U[3 i + j] = gy_i gx_j W (phase (0,0)), U[9 + i] = gy_i W[., 1],
 * U[12 + j] = gx_j W[1, .], U[15] = W[1, 1], in the order [co / 16][ci / 4][quad 4][lane 64][4]: lane = 16 (ci % 4) + (co % 16), element e of
 * quad q = U[4 q + e]; channels past Cin / Cout are zeros. */
size_t vsp_tconvw_weight_floats(int cin, int cout);
int vsp_tconvw_weight_f32(float* U, const float* wp, int cin, int cout, float scale, vsp_stream_t stream);
int vsp_conv_transpose2d_s2_wino_f32(const vsp_conv_params* params, vsp_stream_t stream);

size_t vsp_conv2d_winograd4_work_floats(const vsp_conv_params* p);
size_t vsp_winograd4_weight_floats(int cin, int cout);
int vsp_winograd4_weight_f32(float* U, const float* wp, int cin, int cout, vsp_stream_t stream);
/* 1x1 convolution, stride 1, on small maps as one GEMM (the bottleneck 1x1 layers of the identity loss network at 7x7 / 4x4,
 * Loss/id_loss.py:13,27-41): y[b][co][p] = act(sum_ci w[co][ci] x[b][ci][p] + bias[co]); w row-major (Cout, Cin) = the OIHW
 * weight as it lies; Cin a multiple of 16; bias may be NULL; act: 0 none, 1 leaky relu (slope) times gain. */
int vsp_conv1x1_small_f32(float* y, const float* w, const float* x, const float* bias, int B, int Cout, int Cin, int P, int act,
                          float slope, float gain, vsp_stream_t stream);
/* Weight re-layout on the device (a trained weight is re-packed every iteration: restoration_train.py:123-131, 207-212 step the
 * optimizers between passes).  vsp_pack_weight_f32: OIHW weight (G*cout_g, cin, KH, KW) -> the layout of vsp_conv_params.w,
 * wp[g][tap][ci][co_g] = scale * w[g*cout_g + co_g][ci][tap'] with tap' = KH*KW-1-tap when `flip`.  `adjoint` (G = 1) packs the
 * weight of the data gradient instead: the roles of the channels exchanged, wp[tap][i = co][o = ci] = scale * w[co][ci][tap']
 * (replaces weight.transpose(0,1).flip(2,3) + packing in the reference's conv2d_gradfix.py:152-190 backward).
 * vsp_winograd_weight_f32: packed weight -> the transformed weight of vsp_conv2d_winograd_f32 in its fragment order
 * (vsp_winograd_weight_floats() floats); sums in fp64, rounded once. */
int vsp_pack_weight_f32(float* wp, const float* w, int G, int cout_g, int cin, int KH, int KW, int adjoint, int flip, float scale,
                        vsp_stream_t stream);
size_t vsp_winograd_weight_floats(int G, int cin, int cout_g);
int vsp_winograd_weight_f32(float* U, const float* wp, int G, int cin, int cout_g, vsp_stream_t stream);
int vsp_conv2d_num_configs(void);
const char* vsp_conv2d_config_name(int i);

/* The same convolution contract on the BF16 matrix pipe (v_mfma_f32_32x32x16_bf16, fp32 accumulate): the "bf16 kernels"
 * configuration of the path (BASELINE configs[2]).  Served layers, all 3x3:
 *   - stride 1, padding = dilation: G = 1, up to four dilation groups over one shared input, or true groups (x_group_stride);
 *   - stride 2, dilation 1, padding 0 or 1: G = 1 or true groups (StyledConv_down after its blur, IR-SE down-convs, the
 *     batched e4e style heads);
 *   - transposed = 1: the stride-2 transposed conv of the up-sampling StyledConvs in one pass (fields as for vsp_conv2d_f32).
 * x, y and every prologue / epilogue operand stay fp32: the kernel scales the input by the style in fp32, rounds to bf16 (RNE)
 * while staging and runs the fp32 epilogue chain of vsp_conv2d_f32 on the fp32 accumulators.  `w` must hold the weights
 * rounded to bf16 in the kernel's LDS image order; with Cin zero-padded to a multiple of 16, co_pad = cout_g rounded up to 32
 * and nchunk = ceil(Cin / 16):
 *     w[(((((g * nchunk + chunk) * 9 + tap) * 2 + octet) * co_pad + co) * 8 + j]      (uint16 bf16 bit patterns)
 *         = bf16( W_g[tap][ci = 16*chunk + 8*octet + j][co] )
 * (one 16-byte row per (tap, channel octet, co): what one lane feeds v_mfma as its A fragment; a workgroup copies its rows
 * global -> LDS with global_load_lds_dwordx4).  tile_hint selects the tile variant (0 = automatic, see conv_bf16.hip).
 * Error vs the fp32 kernels: 2^-9 relative per operand, ~2.5e-3 of the output range per layer on random data -- this entry is
 * a throughput configuration, not the parity path. */
int vsp_conv2d_bf16(const vsp_conv_params* p, vsp_stream_t stream);

/* The split-precision form of vsp_conv2d_bf16 ("bf16x3") for the stride-1 and stride-2 layers: both operands are carried as
 * hi + lo bf16 pairs (hi = bf16(v), lo = bf16(v - hi): 16 significant bits) and every product is evaluated as
 * a_hi*b_hi + a_hi*b_lo + a_lo*b_hi into the same fp32 accumulator -- three MFMAs per tile pair on the bf16 pipe, relative
 * error ~2^-16 per product instead of 2^-8: fp32-grade results for layers that the fp32 matrix pipe (1/16 of the bf16 rate)
 * bounds.  Same contract and operands as vsp_conv2d_bf16; `w` holds BOTH weight parts, chunk by chunk:
 *     w[((((((g * nchunk + chunk) * 2 + part) * 9 + tap) * 2 + octet) * co_pad + co) * 8 + j]
 *         part 0 = bf16(W), part 1 = bf16(W - float(bf16(W)))   (hip_ops.bf16x3_weight). */
int vsp_conv2d_bf16x3(const vsp_conv_params* p, vsp_stream_t stream);

/* The "row-vector K" form of vsp_conv2d_bf16 for the low-channel, large-map stride-1 layers of the bf16-activation
 * configuration (32 -> 32 at 1024^2, 64 -> 64 at 512^2, 128 -> 128 at 256^2 ...; conv_bf16_rv.hip): a lane's eight k-values are two
 * channels x four consecutive pixels of an input row (three horizontal taps + one zero weight), so the NCHW bf16 image is
 * staged as it lies in HBM and the output leaves the accumulators as packed pixel pairs.  Serves io_bf16 = 1, G = 1, 3x3,
 * stride 1, dilation = padding = 1, Cin % 8 == 0, Cout % 32 == 0, W % 64 == 0, 16-byte aligned x, images below 1 GiB; returns
 * VSP_ENOTSUP for any other launch (the caller falls back to vsp_conv2d_bf16).  Same operands and epilogue as vsp_conv2d_bf16;
 * `w` in this kernel's order (hip_ops.bf16rv_weight), nchunk = Cin / 8:
 *     w[(((((chunk * 3 + ky) * 2 + quad) * 2 + half) * Cout + co) * 8 + e]              (uint16 bf16 bit patterns)
 *         = bf16( W[tap = 3*ky + kx][ci = 8*chunk + 4*quad + 2*half + (e >> 2)][co] ),  kx = e & 3;  0 for kx = 3.
 * tile_hint: 0 = automatic, 1 = 32-channel tiles (16 rows x 64 pixels), 2 = 64-channel tiles (8 rows x 64 pixels). */
int vsp_conv2d_bf16rv(const vsp_conv_params* p, vsp_stream_t stream);
/* The dilation groups of a SMART branch launch with bf16 activations (io_bf16 = 1; reference models/RestoreNet.py:179-244, 270-418): up to four
 * groups (dilation = padding = 1, 2, 4, 8) of at most 16 output channels over ONE shared input of at most 64 channels (a multiple of 8), W a
 * multiple of 8, no in_shift.  `w` is the PACKED FP32 weight of vsp_conv2d_f32 (the kernel rounds w * in_scale to bf16 once per image and keeps
 * it in registers); patch channel-last and polyphase in LDS, v_mfma_f32_16x16x32_bf16, fp32 accumulation and epilogue chain, bf16 output.
 * VSP_ENOTSUP when the launch is not one it serves (conv_bf16_dg.hip). */
int vsp_conv2d_bf16dg(const vsp_conv_params* p, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Strided, batched small GEMM on fp32 MFMA -- replaces F.linear / torch.matmul of the path
 * (EqualLinear: models/RestoreNet.py:161-171; TACC_block / spatial_attention: models/CodeDiffuser.py:35-47,
 * 86-116).
 *   C[z][m][n] = epi( alpha * sum_k A[z][m][k] * B[z][n][k] )
 *   element addresses: A + z*a_zs + m*a_ms + k*a_ks   (same for B with n), C + z*c_zs + m*c_ms + n
 *   epi(v): v += bias[z*bias_zs + n] * bias_scale (bias may be NULL); act==1: v = lrelu(v, slope) * gain;
 *           act==2: v = sigmoid(v)
 * ---------------------------------------------------------------------------------------------- */
typedef struct vsp_gemm_params {
  const float* A;
  const float* Bm;
  float* C;
  int Z, M, N, K;
  int64_t a_zs, a_ms, a_ks;
  int64_t b_zs, b_ns, b_ks;
  int64_t c_zs, c_ms;
  float alpha;
  const float* bias;
  float bias_scale;
  int act;
  float slope, gain;
  int64_t bias_zs; /* bias stride between batches (0 = one bias vector for all z) */
} vsp_gemm_params;

int vsp_gemm_f32(const vsp_gemm_params* p, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Row-wise helpers of Code_diffuser / the style MLPs (reference models/CodeDiffuser.py:7-12,41,101,31,73;
 * models/RestoreNet.py:24-29).  x and out are [rows, cols] row-major unless stated otherwise.
 * ---------------------------------------------------------------------------------------------- */
/* out[z, r, c] = x[z,r,c] * rsqrt(mean_r(x[z,:,c]^2) + eps): PixelNorm over dim=1 of a [Z,R,C] tensor. */
int vsp_pixelnorm_dim1_f32(float* out, const float* x, int Z, int R, int C, float eps, vsp_stream_t stream);
/* LayerNorm over the last dim (biased variance, eps inside sqrt); gamma/beta may be NULL;
 * optional fused pre-add: normalises (x + add).  post: 0 none, 1 lrelu(slope)*gain. */
int vsp_layernorm_f32(float* out, const float* x, const float* add, const float* gamma, const float* beta,
                      int rows, int cols, float eps, int post, float slope, float gain, vsp_stream_t stream);
/* softmax over the last dim of [rows, cols]. */
int vsp_softmax_lastdim_f32(float* out, const float* x, int rows, int cols, vsp_stream_t stream);
/* softmax over dim=1 of [Z, R, C] (column-wise within each z). */
int vsp_softmax_dim1_f32(float* out, const float* x, int Z, int R, int C, vsp_stream_t stream);
/* out = h * (1 + gamma) + beta (TACC_block tail, models/CodeDiffuser.py:114). */
int vsp_film_f32(float* out, const float* h, const float* gamma, const float* beta, int64_t n,
                 vsp_stream_t stream);
/* out = a * x + b * y with a, b read from device arrays at index idx (DDPM posterior mean,
 * ldm/ddpm.py:348-352: coef1[t]*x0 + coef2[t]*x_t). */
int vsp_axpby_idx_f32(float* out, const float* x, const float* y, const float* a, const float* b, int idx,
                      int64_t n, vsp_stream_t stream);
/* demodulation coefficients: out[b, co] = rsqrt(wscale^2 * sum_ci style[b,ci]^2 * wsq[co,ci] + eps)
 * (models/RestoreNet.py:376-379 with the tap sum hoisted: wsq[co,ci] = sum_taps W[co,ci,:,:]^2). */
int vsp_demod_f32(float* out, const float* style, const float* wsq, int B, int Cin, int Cout, float wscale,
                  float eps, vsp_stream_t stream);
/* Every style modulation of a network for one latent in two launches (round 5): per modulated layer l the modulation vector
 * mod_l[b, ci] = alpha_l * sum_k src[b * bstride + src_off_l + k] * w_l[ci, k] + bias_l[ci] * bias_scale_l   (EqualLinear,
 * models/RestoreNet.py:142-171, evaluated at models/RestoreNet.py:211,467 once per layer) and, where wsq_l is given, the demodulation
 * coefficients demod_l[b, co] = rsqrt(wscale2_l * sum_ci mod_l[b, ci]^2 * wsq_l[co, ci] + eps) (models/RestoreNet.py:376-379).  `table`
 * is a DEVICE array of L entries; src_off is the element offset of the layer's style row inside the latent tensor (row b of the view
 * latent[:, i] starts at src + b * bstride + src_off).  K a multiple of 256 (>= 512), B <= 16, 16-byte aligned rows.  Results are
 * bit-identical to vsp_gemm_f32 (few-row form) followed by vsp_demod_f32 per layer. */
typedef struct {
  const float* w;      /* (cin, K) EqualLinear weight */
  const float* bias;   /* (cin) or NULL */
  const float* wsq;    /* (cout, cin) sum of squared taps, or NULL: no demodulation */
  float* mod;          /* out (B, cin) */
  float* demod;        /* out (B, cout) or NULL */
  int64_t src_off;
  int cin, cout;
  float alpha, bias_scale, wscale2;
  int pad_;
} vsp_style_layer;
int vsp_style_plan_f32(const vsp_style_layer* table, int L, const float* src, int B, int64_t bstride, int K, int max_cin, int max_cout,
                       float eps, vsp_stream_t stream);
/* The same coefficients under autograd (training rows; reference models/RestoreNet.py:376-379 differentiated by torch): forward from
 * the weight w[Cout, Cin, K] (K taps) -- wsq[co, ci] = sum_k w^2 is written for the backward -- and the gradient of a loss through
 * `out` with respect to the style and the weight:  t = -0.5 wscale^2 out^3 g;  dstyle[b, ci] = 2 style[b, ci] sum_co t[b, co] wsq[co, ci];
 * dw[co, ci, k] = 2 w[co, ci, k] sum_b t[b, co] style[b, ci]^2 (overwritten, not accumulated; either output may be NULL).  B <= 16. */
int vsp_demod_weight_f32(float* out, float* wsq, const float* style, const float* w, int B, int Cin, int Cout, int K, float wscale,
                         float eps, vsp_stream_t stream);
int vsp_demod_weight_bwd_f32(float* dstyle, float* dw, const float* g, const float* out, const float* style, const float* wsq,
                             const float* w, int B, int Cin, int Cout, int K, float wscale, vsp_stream_t stream);
/* ... with a row pitch for g AND out (column windows of wider [B, g_stride] tensors: the four branches of a SMART layer share one
 * concatenated demodulation tensor) and `accumulate` = 1: dstyle / dw are ADDED to what the buffers hold (the convolution's own style and
 * weight gradients), so that one tensor per operand leaves the layer's backward. */
int vsp_demod_weight_bwd_acc_f32(float* dstyle, float* dw, const float* g, int g_stride, const float* out, const float* style,
                                 const float* wsq, const float* w, int B, int Cin, int Cout, int K, float wscale, int accumulate,
                                 vsp_stream_t stream);
/* 2x2 mean pooling of [planes, 2*OH, 2*OW] (F.interpolate bilinear 512->256 with align_corners=False is
 * exactly this, Loss/e4e_embedding.py:97; AdaptiveAvgPool2d 1024->512, e4e/models/psp.py:246). */
int vsp_avgpool2x2_f32(float* out, const float* x, int64_t planes, int OH, int OW, vsp_stream_t stream);
/* bilinear resize, align_corners=True, then add: out = resize(x -> [OH,OW]) + y
 * (_upsample_add, e4e/models/encoders/helpers.py:123-140). */
int vsp_upsample_add_f32(float* out, const float* x, const float* y, int64_t planes, int IH, int IW, int OH,
                         int OW, vsp_stream_t stream);
/* global average pool: out[plane] = mean(x[plane, :]) (SEModule, helpers.py:57-73). */
int vsp_plane_mean_f32(float* out, const float* x, int64_t planes, int hw, vsp_stream_t stream);
/* out = x * gate[plane] + y (SE excitation + shortcut add, helpers.py:72,112). y may be NULL. */
int vsp_scale_add_f32(float* out, const float* x, const float* gate, const float* y, int64_t planes, int hw,
                      vsp_stream_t stream);
/* strided gather of y[b,c,::s,::s] (MaxPool2d(1, stride) shortcut, helpers.py:101). */
int vsp_subsample_f32(float* out, const float* x, int64_t planes, int IH, int IW, int s, vsp_stream_t stream);
/* 8-bit image quantiser of torchvision.utils.save_image(normalize=True, value_range=(lo, hi)) fused with the
 * NCHW -> NHWC transpose a PNG encoder wants (reference restoration_test.py:138-157; torchvision 0.13 utils.py):
 *   t = (clamp(x, lo, hi) - lo) / max(hi - lo, 1e-5);  out[b,y,x,c] = (uint8) clamp(t * 255 + 0.5, 0, 255) */
int vsp_quantize_u8_nhwc(uint8_t* out, const float* x, int B, int C, int H, int W, float lo, float hi,
                         vsp_stream_t stream);
/* Pair statistics of two 8-bit images a, b of shape (B, H, W, C), dense, C = 1 or 3 -- the bytes a PNG writer puts on disk
 * (vsp_quantize_u8_nhwc) -- from which PSNR and SSIM of every image pair follow:
 *   sse[i]  = sum over pixels and channels of (a - b)^2, exact.  PSNR = 10 log10(255^2 H W C / sse[i]), formed by the
 *             caller in float64 (the reference's my_lpips.psnr(p0, p1, 255.), my_lpips/__init__.py:57-58).
 *   ssim[i] = mean over channels and over the VALID window positions ((H - w + 1) x (W - w + 1): scikit-image's crop by
 *             (w - 1) / 2) of ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), C1 = (0.01 * 255)^2,
 *             C2 = (0.03 * 255)^2, with the window
 *     VSP_WIN_UNIFORM7: 7 x 7 box, sample covariance (x 49 / 48): scikit-image's structural_similarity defaults, i.e. what
 *                       the reference's my_lpips.dssim(p0, p1, range=255.) measures (dssim = (1 - ssim) / 2, :60-61);
 *     VSP_WIN_GAUSS11:  11 x 11 separable Gaussian, sigma 1.5, taps normalised to sum 1, population covariance (Wang et al.
 *                       2004; scikit-image with gaussian_weights=True, use_sample_covariance=False).
 * Box-window moments are exact 32-bit integers up to one fp32 ratio per position; Gaussian moments are fp32 around the
 * tile's mean; positions are added in float64 in a fixed order.  Image i gets the same bits for every B and on every launch.
 * `work`: vsp_pair_stats_work_bytes(B, H, W, C, window) bytes of device memory, 8-byte aligned, private to the call until
 * it has finished on `stream` (0 is returned for arguments vsp_pair_stats_u8 refuses).
 * VSP_EINVAL: H or W below the window, C not 1 or 3, unknown window, null pointer, B > 65535, H or W > 32768. */
#define VSP_WIN_UNIFORM7 7
#define VSP_WIN_GAUSS11 11
size_t vsp_pair_stats_work_bytes(int B, int H, int W, int C, int window);
int vsp_pair_stats_u8(unsigned long long* sse, double* ssim, const uint8_t* a, const uint8_t* b, int B, int H, int W, int C,
                      int window, void* work, vsp_stream_t stream);
/* F.interpolate(x, (OH, OW), mode="bilinear", align_corners=False) on `planes` = B*C planes (the resize to 256^2 in front of the
 * e4e encoder, reference Loss/e4e_embedding.py:91-100, for inputs that are not 512^2 -- there it is the 2x2 mean above). */
int vsp_resize_bilinear_f32(float* out, const float* x, int64_t planes, int IH, int IW, int OH, int OW, vsp_stream_t stream);
/* Latent plumbing of a batch as single launches (the reference runs it as repeat / cat / flip / add on (B, 18, 512) tensors):
 *   e4e_codes:   codes[b,t,:] = heads[t,b,:] + (t > 0 ? heads[0,b,:] : 0) + latent_avg[t,:]  -- the 18 map2style outputs (T, B, D) to
 *                W+ codes (B, T, D) (psp_encoders.py:188-199 w0 + delta_i, psp.py:159-165 latent_avg; latent_avg may be NULL)
 *   rows_concat: out[b,t,:] = [seg_0 | seg_1 | seg_2], seg_k = src_k[b*batch_stride_k + tt*token_stride_k + 0..width_k), tt = t or
 *                T-1-t (flip_k); token_stride 0 broadcasts one row over the tokens (Restoration_net's latent = [W+ code | mapped z],
 *                its flipped copy and the decoder styles [latent | x_global], models/RestoreNet.py:1000-1025).  Host arrays. */
int vsp_e4e_codes_f32(float* out, const float* heads, const float* latent_avg, int B, int T, int D, vsp_stream_t stream);
int vsp_rows_concat_f32(float* out, int B, int T, int nseg, const float* const* src, const int* batch_stride, const int* token_stride,
                        const int* width, const int* flip, vsp_stream_t stream);
/* out = a + b + c (c may be NULL). */
int vsp_add3_f32(float* out, const float* a, const float* b, const float* c, int64_t n, vsp_stream_t stream);

/* 1x1 convolution with at most 4 channels on one side, as an HBM stream (no MFMA tile, no padding of the tiny side):
 *   Cout <= 4 (ToRGB: modulated 1x1 conv without demodulation + bias + FIR-upsampled skip, models/RestoreNet.py:647-666):
 *       y[b,co,p] = sum_ci x[b,ci,p] * w[co,ci] * in_scale[b,ci] + ch_bias[co] + res[b,co,p] + up(up_src)[b,co,p]
 *       up(.) = upfirdn2d(up_src (B,Cout,H/2,W/2), up_kernel (4x4), up = 2, pad = (2,1)), the `Upsample` of the RGB skip
 *       (models/RestoreNet.py:100-118), evaluated inside the kernel: the skip image is never materialised at full size
 *   Cin <= 4 (the 3 -> 64 input layer, two FusedLeakyReLUs in the epilogue, models/RestoreNet.py:725-787 with k = 1):
 *       y[b,co,p] = act2(act1(sum_ci x[b,ci,p] * w[co,ci] * in_scale[b,ci] + ch_bias[co])),  act_i(v) = lrelu(v + bias_i[co], 0.2) * sqrt2
 * x (B,Cin,HW), y / res (B,Cout,HW) dense, W = row length; in_scale, ch_bias, bias1, bias2, res, up_src may be NULL.
 * The weights of a launch sit in 64 KB of LDS: Cout * Cin <= 16384 on the few-output side (Cin <= 4096 at Cout = 4), Cout * (Cin + 3)
 * <= 16384 on the few-input side (Cout <= 2340 at Cin = 4); anything wider is VSP_EINVAL before any launch. */
int vsp_pointwise_f32(float* y, const float* x, const float* w, const float* in_scale, const float* ch_bias,
                      const float* bias1, int act1, const float* bias2, int act2, const float* res, const float* up_src,
                      const float* up_kernel, int W, int B, int Cin, int Cout, int64_t HW, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fused TACC_block step of Code_diffuser (reference models/CodeDiffuser.py:86-116 and :35-47), 18 tokens x 512
 * channels.  P is the [B*18, ldp] projection buffer of one block: columns [k_off, v_off, q2_off, v2_off) + 512 hold
 * K, V, q (spatial_attention) and v (spatial_attention) of pixelnorm(x).  The Linear(513 -> 512) layers that read the
 * condition c = [embd, t/T] are supplied split: e* = embd @ W[:, :512]^T (step independent, [B*18, 512]) and the last
 * weight column w* (w*[d * stride]); tfrac = t/T is shared by the batch (the sampler's case).
 *   scores:    score[b,i,j] = softmax_j( K[b,i,:] . (eQ[b,j,:] + tfrac*wq) / sqrt(18) )
 *   chan_attn: A = softmax over rows of ((ek[b] + tfrac*wk)^T q2 / sqrt(512));  t[b] = v2[b] @ A
 *   tail:      (token attention folded in: score as above) y = LN(score @ V + LN(t)) * (1 + gamma) + beta;
 *              if xold: y = c1[idx]*y + c2[idx]*xold (DDPM posterior
 *              mean, ldm/ddpm.py:348-352);  pn = PixelNorm over the 18 tokens of y (may be NULL)
 *   head_pre:  out[s,m,:] = lrelu(LN(e[m,:] + (s/t_div)*wcol) * ln_w + ln_b, 0.2) * sqrt(2) for s = 0..S-1
 *              (first half of the gamma_/beta_ heads for every step of the chain at once)
 * ---------------------------------------------------------------------------------------------- */
int vsp_tacc_scores_f32(float* score, const float* P, int ldp, int k_off, const float* eQ, const float* wq,
                        int wq_stride, float tfrac, int B, int n_tok, int dim, vsp_stream_t stream);
int vsp_tacc_chan_attn_f32(float* t, const float* P, int ldp, int q2_off, int v2_off, const float* ek,
                           const float* wk, int wk_stride, float tfrac, int B, int n_tok, int dim,
                           vsp_stream_t stream);
int vsp_tacc_tail_f32(float* y, float* pn, const float* P, int ldp, int k_off, int v_off, const float* eQ,
                      const float* wq /* contiguous [512] */, float tfrac, const float* t, const float* gamma,
                      const float* beta, const float* xold, const float* c1, const float* c2, int idx, int B, int n_tok,
                      int dim, vsp_stream_t stream);
int vsp_tacc_head_pre_f32(float* out, const float* e, const float* wcol, int w_stride, const float* ln_w,
                          const float* ln_b, int S, int M, int dim, float t_div, vsp_stream_t stream);

/* The whole sampler chain of Code_diffuser behind one call (replaces the Python loops ldm/ddpm.py:400-429 p_sample_loop /
 * ldm/ddim.py:130-180 ddim_sampling around models/CodeDiffuser.py:118-140): for s in 0..n_steps-1, with t = step[s]:
 *   x0 = denoiser(x, cond, t)  (n_blocks TACC blocks);   x <- c1[k] * x0 + c2[k] * x,  k = coef_idx[s] (or t when NULL)
 * (c1 == c2 == NULL: x <- x0).  `blocks`, `step`, `coef_idx` are HOST arrays; every pointer inside is a device pointer.
 * Per block: wcat = [Wk; Wv; Wq2; Wv2] rows (2048 x 512), eQ / ek = condition halves of the two Linear(513) layers
 * ((B*18) x 512), wq / wk = their contiguous t-columns (512), gamma / beta = FiLM heads of steps 0..head_steps-1
 * (head_steps x (B*18) x 512, from vsp_tacc_head_pre_f32 + vsp_gemm_f32).  x is updated in place; `work` holds
 * vsp_tacc_chain_work_floats(B) floats of scratch.  3 launches per block and step, nothing synchronises. */
typedef struct vsp_tacc_block {
  const float* wcat;
  const float* eQ;
  const float* ek;
  const float* wq;
  const float* wk;
  const float* gamma;
  const float* beta;
  /* optional (NULL: read wcat): the same [4D, D] matrix in MFMA FRAGMENT order -- [n / 16][k / 16][lane = 16 (k % 16 / 4) + n % 16][k % 4]
   * -- so that a wavefront's 16-byte-per-lane load is 1 KiB of consecutive memory (read row-major, the 16 lanes of a quarter wave hit
   * 16 different cache lines for 16 bytes each: the projection was bound by the texture-address path, not by its MFMAs) */
  const float* wcat_frag;
} vsp_tacc_block;

typedef struct vsp_tacc_chain_params {
  int B, n_tok, dim, n_blocks;
  const vsp_tacc_block* blocks;
  float* x;
  float* work;
  size_t work_floats;
  int n_steps;
  const int* step;
  const int* coef_idx;
  const float* c1;
  const float* c2;
  float t_div;     /* t enters the condition as t / t_div (Code_diffuser.max_period) */
  int head_steps;
} vsp_tacc_chain_params;

size_t vsp_tacc_chain_work_floats(int B);
int vsp_tacc_chain_f32(const vsp_tacc_chain_params* p, vsp_stream_t stream);
/* (A persistent single-launch form of this chain -- clusters of 1 ... 16 workgroups per image, two cluster barriers per block --
 * was built and parity-tested in round 3 and measured SLOWER than the three launches per block (46 vs 27.5 us per block at batch 8):
 * retired to the branch `experiments/persistent-chain` in round 4; DESIGN section 4 keeps the accounting.) */

/* ------------------------------------------------------------------------------------------------
 * bf16 activations in HBM (BASELINE configs[2] "bf16 kernels"; the fp32 path above is the parity path).  A bf16 tensor is
 * the raw 16-bit words of its fp32 twin rounded to nearest even, same dense NCHW shape.  Arithmetic stays fp32.
 *   vsp_convert_*      tensor conversion at the boundary between bf16-I/O kernels and fp32 ones (maps of 16^2 and smaller)
 *   vsp_upfirdn2d_bf16 the `Blur` form of vsp_upfirdn2d_f32 (up = down = 1, minor = 1, 2x2 / 3x3 / 4x4 taps, out_w >= 16) with
 *                      x, out and the epilogue's res1 / res2 in bf16 (kernel taps, noise, scales, biases fp32); VSP_ENOTSUP otherwise
 *   vsp_pointwise_bf16 vsp_pointwise_f32 with the WIDE side in bf16: x when Cout <= 4 (ToRGB reads bf16 features, writes the
 *                      fp32 image), y when Cin <= 4 (the 3 -> 64 input layer reads the fp32 image, writes bf16 features)
 * ---------------------------------------------------------------------------------------------- */
int vsp_convert_f32_to_bf16(uint16_t* out, const float* x, int64_t n, vsp_stream_t stream);
int vsp_convert_bf16_to_f32(float* out, const uint16_t* x, int64_t n, vsp_stream_t stream);
int vsp_upfirdn2d_bf16(uint16_t* out, const uint16_t* x, const float* kernel, int major, int in_h, int in_w, int minor,
                       int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0,
                       int pad_y1, const vsp_fir_epilogue* epilogue, vsp_stream_t stream);
/* Per-image modulated weights for vsp_conv2d_bf16 (w_bstride): out[b] = bf16(wp * style[b][ci]) in the kernel's LDS-image order
 * [group][chunk][tap][octet 2][co_pad][8] (ci = 16 chunk + 8 octet + j; Cin zero-padded to 16, cout_g to 32), wp = the packed fp32 weights
 * [G][9][Cin][cout_g] of vsp_conv2d_f32, style = (B, Cin) rows `style_bstride` floats apart (shared by the groups of a dilation-group launch).
 * One rounding per weight (the kernel's own path rounds W and x * style separately).  Returns the byte size of one image's set through
 * vsp_modulate_weight_bf16_bytes.  Reference: models/RestoreNet.py:381-383 (weight = scale * weight * style), without the demodulation,
 * which stays an fp32 (B, Cout) vector in the epilogue. */
size_t vsp_modulate_weight_bf16_bytes(int G, int cin, int cout_g);
int vsp_modulate_weight_bf16(uint16_t* out, const float* wp, const float* style, int B, int64_t style_bstride, int G, int cin, int cout_g,
                             vsp_stream_t stream);
int vsp_pointwise_bf16(void* y, const void* x, const float* w, const float* in_scale, const float* ch_bias,
                       const float* bias1, int act1, const float* bias2, int act2, const float* res, const float* up_src,
                       const float* up_kernel, int W, int B, int Cin, int Cout, int64_t HW, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Convolution backward (the training step; reference op/conv2d_gradfix.py:104-227, which on current torch is
 * autograd of F.conv2d / F.conv_transpose2d, :78-92).
 *   data gradient   = the forward kernels: conv with the flipped, channel-transposed weight (stride 1), the one-pass
 *                     transposed conv (adjoint of the stride-2 conv) and the stride-2 conv (adjoint of the transposed conv)
 *   weight gradient = vsp_conv2d_wgrad_f32:
 *     dw[g][co][ci][ky][kx] = sum_{b,oy,ox} dy[b, g*Cout_g+co, oy, ox] * dy_scale[b, .] * x[b, g*Cin_g+ci, oy*stride+ky*dil-pad, ox*stride+kx*dil-pad] * x_scale[b, .]
 *     dw is (G*Cout_g, Cin_g, KH, KW) dense (torch's weight layout), overwritten; x (B, G*Cin_g, H, W), dy (B, G*Cout_g, OH, OW);
 *     x_scale (B, G*Cin_g) / dy_scale (B, G*Cout_g) may be NULL (the per-sample style / demodulation vectors of a
 *     modulated layer in its modulate-input / demodulate-output form); 3x3 or 1x1, stride 1 or 2.  G = B with batch 1 is
 *     the reference's groups=batch form (models/RestoreNet.py:373-383).  A transposed conv's weight gradient is the same
 *     call with x and dy exchanged (and the result read as (ci, co)).
 *   vsp_plane_dot_f32: out[p] = sum_i a[p,i]*b[p,i] -- the gradients of the two per-sample scale vectors.
 * ---------------------------------------------------------------------------------------------- */
typedef struct vsp_conv_wgrad_params {
  const float* x;
  const float* dy;
  float* dw;
  const float* x_scale;
  const float* dy_scale;
  int B, Cin_g, H, W, G, Cout_g, OH, OW, KH, KW, stride, dil, pad;
  /* ABI 3 (all zero = the plain call above): channel windows into larger tensors, a shared input with per-group geometry (the four
   * dilated SMART branches: G = 4, x_shared = 1, per_group_geometry = 1, dil_g = pad_g = {1, 2, 4, 8}), accumulation into dw */
  int x_ch, x_coff;        /* channels of the x tensor (0: G*Cin_g, or Cin_g when shared) and first channel used */
  int dy_ch, dy_coff;      /* channels of the dy tensor (0: G*Cout_g) and first channel used */
  int x_shared;            /* 1: every group reads the same Cin_g input channels */
  int per_group_geometry;  /* 1: group g uses dil_g[g] / pad_g[g] (G <= 4) instead of dil / pad */
  int dil_g[4], pad_g[4];
  int accumulate;          /* 1: add to dw instead of overwriting it */
  float* work;             /* optional workspace: the split-K partial sums go to private copies of dw (plain stores) and a second
                            * kernel adds them up, instead of fp32 atomics into dw (25 % of the kernel's time at 512 channels);  */
  size_t work_floats;      /* floats in `work`: at least one copy of dw, vsp_conv2d_wgrad_work_floats() for the full split */
  float dw_scale;          /* 0 = 1: the sum is multiplied by it before it is stored / added (the layer's equalized-lr factor, so that dw is
                            * the gradient of the PARAMETER: reference models/RestoreNet.py:131, 150 `weight * self.scale`) */
} vsp_conv_wgrad_params;
/* workspace size (floats) with which vsp_conv2d_wgrad_f32 runs its preferred split for these parameters */
size_t vsp_conv2d_wgrad_work_floats(const vsp_conv_wgrad_params* p);
int vsp_conv2d_wgrad_f32(const vsp_conv_wgrad_params* p, vsp_stream_t stream);
int vsp_plane_dot_f32(float* out, const float* a, const float* b, int64_t planes, int64_t n, vsp_stream_t stream);
/* out[p] = sum_i a[p,i]*b[p,i] and, in the same pass, a[p,:] *= scale[p] (d/ds and d/dx of a modulated layer from d/d(x s)) */
int vsp_plane_dot_scale_f32(float* out, float* a, const float* b, const float* scale, int64_t planes, int64_t n, vsp_stream_t stream);
/* NoiseInjection + FusedLeakyReLU of a styled layer as one stream (training forward; reference models/RestoreNet.py:558-569 then
 * op/fused_act.py:199-233):  y[b,c,p] = lrelu(x[b,c,p] + noise_w[0] * noise[b,p] + bias[c], slope) * gain;  bias may be NULL.
 * vsp_noise_dot_f32: out[0] = sum_{b,c,p} gx[b,c,p] * noise[b,p] -- the gradient of the scalar noise weight. */
int vsp_noise_bias_act_f32(float* y, const float* x, const float* noise, const float* noise_w, const float* bias, int B, int C,
                           int64_t hw, float slope, float gain, vsp_stream_t stream);
int vsp_noise_dot_f32(float* out, const float* gx, const float* noise, int B, int C, int64_t hw, vsp_stream_t stream);
/* Backward of the tail of a SMART layer (reference models/RestoreNet.py:220-244: FusedLeakyReLU(bias1) -> NoiseInjection ->
 * FusedLeakyReLU(bias2); the forward is the fusion conv's epilogue: act1 / bias1 / noise / act2 / bias2 of vsp_conv_params) from the
 * final output y alone: g1 = gradient entering the conv, db1[c], db2[c], dnw[0] (the three are zeroed here, then accumulated). */
int vsp_smart_tail_bwd_f32(float* g1, float* db1, float* db2, float* dnw, const float* g, const float* y, const float* noise,
                           const float* noise_w, const float* bias2, int B, int C, int64_t hw, float slope, float gain,
                           vsp_stream_t stream);
/* out[c] = sum over b and the plane of x[b, c, :] (x (B, C, hw) dense): bias gradients of the training step */
int vsp_channel_sum_f32(float* out, const float* x, int B, int C, int64_t hw, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * ADA augmentation primitives (reference non_leaking.py:857-934).
 *   vsp_affine_sample_f32      out = F.grid_sample(x, F.affine_grid(theta, (B,C,OH,OW), align_corners=False), "bilinear", "zeros",
 *                              align_corners=False); theta (B, 2, 3) fp32 on the device; the grid is never materialised
 *   vsp_affine_sample_bwd_f32  gx = adjoint of the above w.r.t. x applied to gout (gx (B,C,IH,IW) is overwritten)
 *   vsp_color_affine_f32       y[b,c,p] = sum_k M[b,c,k] x[b,k,p] + t[b,c] on 3-channel images (apply_color, :910-918); M (B,3,3),
 *                              t (B,3) or NULL
 * ---------------------------------------------------------------------------------------------- */
int vsp_affine_sample_f32(float* out, const float* x, const float* theta, int B, int C, int IH, int IW, int OH, int OW,
                          vsp_stream_t stream);
int vsp_affine_sample_bwd_f32(float* gx, const float* gout, const float* theta, int B, int C, int IH, int IW, int OH, int OW,
                              vsp_stream_t stream);
int vsp_color_affine_f32(float* y, const float* x, const float* M, const float* t, int B, int64_t HW, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Operators of the training losses (BASELINE configs[4]: LPIPS-VGG + ArcFace identity; reference restoration_train.py:236-245).
 *   vsp_maxpool2d_f32 / _bwd   F.max_pool2d(x, k, s, p) in floor mode on `planes` = B*C planes (torchvision 0.13 vgg16.features
 *                              2x2/2, resnet101 3x3/2 pad 1); the backward recomputes each window's arg-max (first maximum in
 *                              row-major order, the LAST NaN if there is one: ATen's rule) from x; dx is overwritten
 *   vsp_lpips_layer_f32        out[b] = mean_p sum_c w[c] (f0/(|f0|_c + 1e-10) - f1/(|f1|_c + 1e-10))^2  -- normalize_tensor,
 *                              squared difference, the 1x1 `lin` layer and spatial_average of one LPIPS level in one stream
 *                              (my_lpips/networks_basic.py:73-83, my_lpips/__init__.py:44-46); f0, f1 (B,C,HW), w (C), out (B)
 *   vsp_lpips_layer_ws_f32     the same with a caller's work buffer (contents irrelevant before, undefined after): every workgroup stores
 *                              its sum there and one more launch adds them in a fixed order -- the same bits in every run.  The form
 *                              without it adds one atomic per workgroup onto out[b]: up to 2048 serial float additions, an error of up
 *                              to 2e-6 of the result at the widest grid, in an order that changes from run to run
 *   vsp_lpips_layer_bwd_f32    df1 = gout[b] * d out[b] / d f1   (the reference calls forward(target, pred): my_lpips/__init__.py:42)
 *   vsp_resize_bilinear_bwd_f32  adjoint of vsp_resize_bilinear_f32 (F.interpolate(size=112) in Loss/id_loss.py:37-41); dx overwritten
 * ---------------------------------------------------------------------------------------------- */
int vsp_maxpool2d_f32(float* out, const float* x, int64_t planes, int H, int W, int OH, int OW, int k, int s, int p,
                      vsp_stream_t stream);
int vsp_maxpool2d_bwd_f32(float* dx, const float* dy, const float* x, int64_t planes, int H, int W, int OH, int OW, int k, int s,
                          int p, vsp_stream_t stream);
int vsp_lpips_layer_f32(float* out, const float* f0, const float* f1, const float* w, int B, int C, int HW, vsp_stream_t stream);
#define VSP_LPIPS_WORK_BLOCKS 2048   /* the widest grid per sample: work of B * VSP_LPIPS_WORK_BLOCKS floats always suffices */
int vsp_lpips_layer_ws_f32(float* out, float* work, int64_t work_floats, const float* f0, const float* f1, const float* w, int B, int C, int HW,
                           vsp_stream_t stream);
int vsp_lpips_layer_bwd_f32(float* df1, const float* f0, const float* f1, const float* w, const float* gout, int B, int C, int HW,
                            vsp_stream_t stream);
int vsp_resize_bilinear_bwd_f32(float* dx, const float* dy, int64_t planes, int IH, int IW, int OH, int OW, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Keyed random tensors -- replaces the path's global-RNG draws: one `image.new_empty(B,1,H,W).normal_()` per NoiseInjection
 * (reference models/RestoreNet.py:564-569, e4e/models/stylegan2/model.py:287-292), `torch.randn(shape)` for x_T
 * (ldm/ddpm.py:423), `torch.randn(batch, latent_dim)` for z (restoration_test.py:77-82) and the synthetic LQ batch of the
 * benchmark.  ONE launch fills n_seg tensors laid out back to back in `out`, segment s = [B][seg_elems[s]] floats;
 *   value(s, b, e) = f( Philox4x32-10( key = seed, counter = (e / 4, seg_ids[s], image_index0 + b) ) word e % 4 ),
 * dist 0: standard normal (Box-Muller), dist 1: uniform(-1, 1).  The value depends on the GLOBAL image index only, so a
 * batch sharded over ranks draws what a single GPU would (SURVEY 8e "per-rank RNG streams derived from (seed, global image
 * index)").  seg_elems / seg_ids are HOST arrays; n_seg <= VSP_NOISE_MAX_SEGMENTS. */
#define VSP_NOISE_MAX_SEGMENTS 64
int vsp_keyed_fill_f32(float* out, int B, const int64_t* seg_elems, const int32_t* seg_ids, int n_seg, uint64_t seed,
                       int64_t image_index0, const int64_t* image_index0_dev, int dist, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Training degradations -- the low-quality (LQ) synthesis of the reference's training datasets on the device:
 * `ImageFolder_restore_free_form.degrade_img` (reference dataset.py:327-373, behind restoration_train.py:454-461) and the same chain
 * without the haze step in `ImageFolder_restore.__getitem__` (dataset.py:83-127, behind code_diffuser_train.py:365-386).  The
 * reference runs it on the host with cv2 / numpy, one image at a time; here each stage is ONE launch over a ragged batch of n items
 * (one item = one LQ image made from gt image `src`), every item with its own parameters in a device table of vsp_degrade_item.
 *
 *   gt       (B, 3, H, W) fp32 in [0, 1]; blurred / out (n, 3, H, W) fp32
 *   lq       uint8, item i's three planes of dh*dw samples at element offset pix_off (channel order of the gt)
 *   noise / pre (optional) fp32, item i's (dh, dw, 3) values at element offset pix_off (numpy's randn(h, w, 3) order)
 *   work     uint8, item i's JPEG planes at byte offset jpg_off: Y (ph*pw), Cb, Cr (ph/2*pw/2 each), ph / pw = dh / dw rounded up to 16
 * The caller sizes every buffer from the table it uploads; the kernels clamp what they derive from an entry but do not check
 * offsets against buffer sizes (they cannot see them): vspbfr_amd/degrade.py builds and checks the table.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_DEGRADE_MAX_KSIZE 41      /* blur taps per side (odd) */
#define VSP_DEGRADE_MAX_SIZE 2048     /* image side, gt and downsampled */
#define VSP_DEGRADE_MAX_ITEMS 1024    /* items per launch */
#define VSP_DEGRADE_HAZE 1            /* flags: x * alpha + (1 - alpha) after the blur (dataset.py:341-344) */
#define VSP_DEGRADE_GREY 2            /* flags: cv2 BGR2GRAY of the final LQ (dataset.py:303-308) */
#define VSP_DEGRADE_NOISE_KEY 0x44475244u /* xor-ed into the low key word of the noise draws ("DGRD") */

typedef struct vsp_degrade_item {
  int64_t tap_off;   /* float offset of the ksize*ksize taps (row-major, correlation order) in `taps` */
  int64_t pix_off;   /* element offset of the item in lq / noise / pre */
  int64_t jpg_off;   /* byte offset of the item's JPEG planes in `work` */
  int64_t sample;    /* global sample index (noise key) */
  int32_t src;       /* gt image of the batch */
  int32_t ksize;     /* blur taps per side, odd, <= VSP_DEGRADE_MAX_KSIZE */
  int32_t dh, dw;    /* downsampled size: (int(h // scale), int(w // scale)) (dataset.py:347-348) */
  int32_t quality;   /* JPEG quality 1..100 (my_degradations.py:681-710) */
  int32_t flags;     /* VSP_DEGRADE_HAZE | VSP_DEGRADE_GREY */
  int32_t mcu0;      /* index of the item's first 16x16 MCU in the batch (running sum of ceil(dh/16) * ceil(dw/16)) */
  int32_t slot;      /* LQ slot of the sample, 0..3 (noise key) */
  float alpha;       /* haze alpha */
  float sigma;       /* noise standard deviation on the 0..255 scale (my_degradations.py:386-400) */
} vsp_degrade_item;

/* gt: out (B, 3, H, W) = hwc (B, H, W, 3) uint8 / 255 (dataset.py:277 `np.array(img) / 255`), or = in (B, 3, H, W) fp32 (in == out
 * allowed); exactly one of hwc / in.  grey (device int32 [B] or NULL): cv2 BGR2GRAY of image b where grey[b] != 0 (dataset.py:303-311). */
int vsp_degrade_gt_f32(float* out, const uint8_t* hwc, const float* in, const int32_t* grey, int B, int H, int W, vsp_stream_t stream);
/* blur: blurred[i] = cv2.filter2D(gt[src_i], -1, taps_i) (correlation, anchor at the centre, BORDER_REFLECT_101; dataset.py:337-338,
 * my_degradations.py:295-356), then the haze of dataset.py:341-344 where flagged. */
int vsp_degrade_blur_f32(float* out, const float* gt, const float* taps, const vsp_degrade_item* items, int n, int B, int H, int W,
                         vsp_stream_t stream);
/* down: cv2.resize(blurred[i], (dw, dh), INTER_LINEAR) (dataset.py:347-348), + noise * sigma / 255, clip to [0, 1] (my_degradations.py
 * :386-400, :483-492), saturate_cast to uint8 (round half to even) as cv2.imencode does (:681-710).  noise: injected values, or NULL
 * for  Philox4x32-10 (key = (seed_lo ^ VSP_DEGRADE_NOISE_KEY, seed_hi), counter = (e / 4, step << 2 | slot, sample_lo, sample_hi))
 * with Box-Muller as vsp_keyed_fill_f32, element e of the item's (dh, dw, 3) draw.  pre (optional): the resized values before the
 * noise.  max_pixels >= every item's dh * dw. */
int vsp_degrade_down_u8(uint8_t* lq, float* pre, const float* blurred, const float* noise, const vsp_degrade_item* items, int n, int H,
                        int W, int max_pixels, uint64_t seed, int64_t step, vsp_stream_t stream);
/* jpeg: in place, the pixel values of cv2.imdecode(cv2.imencode('.jpg', img, quality)) (my_degradations.py:681-710) at libjpeg's
 * defaults -- 4:2:0, ISLOW DCT, baseline quality tables, fancy upsampling -- with channel 0 read as blue (cv2's BGR).  Bit-exact.
 * Two launches: per-MCU transform into `work`, then upsampling + colour back into lq.  total_mcus = sum of the items' MCUs. */
int vsp_degrade_jpeg_u8(uint8_t* lq, uint8_t* work, const vsp_degrade_item* items, int n, int total_mcus, int max_pixels,
                        vsp_stream_t stream);
/* up: out[i] = np.clip(round(cv2.resize(lq_i / 255, (W, H), INTER_LINEAR) * 255), 0, 255) / 255 (dataset.py:356, :370), then cv2
 * BGR2GRAY where flagged (dataset.py:303-306). */
int vsp_degrade_up_f32(float* out, const uint8_t* lq, const vsp_degrade_item* items, int n, int H, int W, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Device-side ingest: Pillow's 8-bit LANCZOS resize (Image.resize(size, LANCZOS)) and a crop, for a ragged batch of decoded RGB images
 * of different sizes, bit for bit (csrc/resample.hip).  Pillow's resampler is integer arithmetic: per axis and output coordinate a
 * first source coordinate `xmin`, a tap `count` and fixed-point taps round(k * 2^22); a horizontal then a vertical pass of
 * clip8((2^21 + sum(pixel * k)) >> 22) with a uint8 image between them.  The tables need libm's sin in float64 and are built on the
 * host (vspbfr_amd/resample.py lanczos_coeffs); the device does the integer multiply-adds.
 *
 *   src      packed source bytes; item i's (sh, sw, 3) uint8 image at byte offset src_off, rows of 3 * sw bytes without padding
 *   coef     int32; a table for (in, out) at int32 offset o is  xmin[out], count[out], taps[ksize][out]  (tap-major), ksize =
 *            (int)ceil(3 * max(1, in / out)) * 2 + 1
 *   work     the uint8 image between the passes: item i's rows row0..row1 of the horizontally resized crop columns at byte offset
 *            work_off, row stride vsp_lanczos_work_bytes(1, W); private to the call until it has finished on `stream`
 *   out_u8   (n, H, W, 3) uint8 and / or  out_f32  (n, 3, H, W) fp32 = ((v / 255) - 0.5) / 0.5, three separately rounded operations
 *            (torchvision's ToTensor + Normalize(0.5, 0.5)); either may be NULL, not both
 * Only the crop window [x0, x0 + W) x [y0, y0 + H) of the resized (nw, nh) image is computed, and only source rows row0..row1 (the
 * rows the window's vertical taps read) go through the horizontal pass.  `items` is the table in HOST memory: every entry is checked
 * (sizes, crop, tap counts, all offsets against src_bytes / coef_ints / work_bytes) before anything is launched; `items_dev` is the
 * same table in device memory, which the kernels read.  VSP_EINVAL: null pointer, zero size, crop outside the resized image, an
 * offset outside its buffer.  VSP_ENOTSUP: a side above VSP_RESAMPLE_MAX_SIDE or more than VSP_RESAMPLE_MAX_TAPS taps (a reduction
 * above 16x): the caller resizes such an image on the host and passes it as a VSP_RESAMPLE_COPY item.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_RESAMPLE_PRECISION_BITS 22 /* Pillow's PRECISION_BITS (32 - 8 - 2) */
#define VSP_RESAMPLE_MAX_TAPS 97       /* taps per output coordinate: reductions up to 16x */
#define VSP_RESAMPLE_MAX_SIDE 8192     /* source, resized and output side */
#define VSP_RESAMPLE_MAX_ITEMS 65535   /* items per launch */
#define VSP_RESAMPLE_FLIP 1            /* flags: the source is read mirrored (column sw - 1 - x): transpose(FLIP_LEFT_RIGHT) first */
#define VSP_RESAMPLE_COPY 2            /* flags: the source already has the output size and is copied (sw == nw == W, sh == nh == H) */

typedef struct vsp_resample_item {
  int64_t src_off;   /* byte offset of the source image in `src` */
  int64_t work_off;  /* byte offset of the item's intermediate rows in `work`, a multiple of 4 */
  int64_t hco, vco;  /* int32 offsets of the horizontal (sw -> nw) and the vertical (sh -> nh) table in `coef` */
  int32_t sw, sh;    /* source size */
  int32_t nw, nh;    /* resized size */
  int32_t x0, y0;    /* crop origin inside the resized image */
  int32_t row0, row1;/* first and last source row the crop's vertical pass reads: ymin[y0] .. ymin[y0+H-1] + count[y0+H-1] - 1 */
  int32_t hk, vk;    /* ksize of the two tables */
  int32_t flags;     /* VSP_RESAMPLE_FLIP | VSP_RESAMPLE_COPY */
  int32_t pad_;
} vsp_resample_item;

/* bytes of `work` for `rows` intermediate rows of an output of width W (0 for arguments outside the limits) */
size_t vsp_lanczos_work_bytes(int rows, int W);
int vsp_lanczos_resize_u8(uint8_t* out_u8, float* out_f32, const uint8_t* src, size_t src_bytes, const int32_t* coef, size_t coef_ints,
                          uint8_t* work, size_t work_bytes, const vsp_resample_item* items, const vsp_resample_item* items_dev, int n,
                          int H, int W, vsp_stream_t stream);

/* The same resize for a batch whose items each have a window of their own, written into one packed buffer: item i computes the
 * dst[i].W x dst[i].H window at (x0, y0) of its resized image and writes it as packed (H_i, W_i, 3) uint8 at byte dst[i].out_off of
 * `out` (any byte offset: 3 W H may be odd); its intermediate rows in `work` have the stride vsp_lanczos_work_bytes(1, W_i).  Bytes
 * of `out` outside the windows are not written.  `items` / `dst` are the tables in HOST memory, `items_dev` / `dst_dev` the same in
 * device memory.  Checked before anything is launched: all that vsp_lanczos_resize_u8 checks, per item against its own window (a
 * VSP_RESAMPLE_COPY item has sw == nw == W_i and sh == nh == H_i); every destination inside out_bytes; destinations ascending and
 * disjoint.  VSP_EINVAL / VSP_ENOTSUP as there. */
typedef struct vsp_resample_dst {
  int64_t out_off;   /* byte offset of the item's (H, W, 3) window in `out` */
  int32_t W, H;      /* the window: columns x0 .. x0 + W - 1 and rows y0 .. y0 + H - 1 of the resized image */
} vsp_resample_dst;

int vsp_lanczos_resize_ragged_u8(uint8_t* out, size_t out_bytes, const uint8_t* src, size_t src_bytes, const int32_t* coef, size_t coef_ints,
                                 uint8_t* work, size_t work_bytes, const vsp_resample_item* items, const vsp_resample_item* items_dev,
                                 const vsp_resample_dst* dst, const vsp_resample_dst* dst_dev, int n, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Device-side PNG encoder: row filters + deflate of a (B, H, W, C) uint8 batch (csrc/png.hip), 8 bits per sample, C = 3 (colour type
 * 2) or 1 (colour type 0), no interlace.  The device writes each image's zlib payload in pieces; the host puts the two-byte zlib header
 * in front, the combined Adler-32 behind, and frames the PNG chunks (vspbfr_amd/png.py assemble).  tests/png_ref.py restates every step
 * in NumPy; the device output equals it byte for byte.
 *
 *   filters    per row the filter type 0..4 with the smallest sum of |residual as int8|, ties to the lowest type; the row above a
 *              segment's first row is the image's real previous row
 *   segments   the filtered stream (H rows of 1 + C * W bytes) is cut into segments of VSP_PNG_SEG_ROWS rows.  A segment is compressed on
 *              its own into ONE deflate block: dynamic Huffman, or a stored block when the coded segment would not be smaller.  A
 *              non-final segment ends with an empty stored block (3 zero bits, padding, 00 00 FF FF) and so on a byte boundary; the
 *              last segment's block carries BFINAL.  The zlib payload is the concatenation of the segments
 *   tokens     literals and distance-1 matches of length 3..258: a maximal stretch of bytes equal to their predecessor inside the
 *              segment is cut into chunks of 258 from its start; a chunk below 3 is literals
 *   codes      literal/length code limited to 15 bits, code-length code to 7: symbols sorted by (count, symbol), Huffman's two-queue
 *              merge taking a leaf before an internal node of equal weight, depths clipped and repaired as zlib does, lengths handed
 *              out longest first in sorted order, canonical codes.  One distance symbol (0) of length 1, or 0 when there is no match
 *   out        image i at byte i * out_capacity, its segment k at k * vsp_png_segment_bound(VSP_PNG_SEG_ROWS, W, C) inside it,
 *              seg_bytes[i * nseg + k] bytes long (never above vsp_png_segment_bound(rows of that segment, W, C): the stored form);
 *              nseg = ceil(H / VSP_PNG_SEG_ROWS).  Bytes of a slot behind a segment's end, rounded up to 4, are not written
 *   seg_adler  [2 * (i * nseg + k)] = sum of the segment's n filtered bytes, [+ 1] = sum of (n - j) * byte[j], both mod 65521; in order
 *              b = (b + n * a + part1) mod 65521, a = (a + part0) mod 65521 from (a, b) = (1, 0) gives zlib's Adler-32 b << 16 | a
 * src is the contiguous (B, H, W, C) tensor; out, seg_bytes, seg_adler and out_capacity are 4-byte aligned; out_capacity >=
 * vsp_png_bound(H, W, C).  Every size is checked on the host before the single launch.  VSP_ENOTSUP: C * W above VSP_PNG_MAX_ROW_BYTES,
 * H above VSP_PNG_MAX_H or B above VSP_PNG_MAX_BATCH (the caller encodes such images on the host); VSP_EINVAL: C not 1 or 3, a zero
 * size, a null or misaligned pointer, out_capacity below the bound.  The bounds return 0 for arguments outside the limits.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_PNG_SEG_ROWS 8           /* rows per segment: 8 x 3073 filtered bytes, the bit buffer and the code tables fit 64 KB of LDS */
#define VSP_PNG_MAX_ROW_BYTES 3072   /* C * W: W <= 1024 for RGB */
#define VSP_PNG_MAX_H 32768
#define VSP_PNG_MAX_BATCH 65535
size_t vsp_png_segment_bound(int rows, int W, int C);
size_t vsp_png_bound(int H, int W, int C);
int vsp_png_encode_u8(uint8_t* out, size_t out_capacity, int32_t* seg_bytes, uint32_t* seg_adler, const uint8_t* src, int B, int H, int W,
                      int C, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Device-side PNG encoder for whole photos: a ragged batch of packed (h, w, C) uint8 images of any width (csrc/png.hip, DESIGN 21;
 * tests/png_ragged_ref.py restates it, the device output equals it byte for byte).  Filters, tokens, codes, the stored-block rule,
 * the empty stored block behind a non-final segment and the Adler parts are those of vsp_png_encode_u8 above; what differs is the cut:
 *
 *   segments   image i's filtered stream, n = h (1 + C w) bytes, is cut into segments of VSP_PNG_RAGGED_SEG_BYTES bytes, the last one
 *              shorter: ceil(n / VSP_PNG_RAGGED_SEG_BYTES) of them.  A boundary may fall inside a row, inside a pixel, on a filter-type
 *              byte or right behind one; a run of equal bytes is cut there.  So the files of this entry differ in bytes from those of
 *              vsp_png_encode_u8 for the same pixels; both are valid PNG streams of those pixels
 *   items      given twice: in host memory, checked before anything is launched, and the same table in device memory.  seg0 = the
 *              segments of the items before (item 0: 0), row0 = the rows of the items before
 *   work       vsp_png_ragged_work_bytes(segments, rows of the call) bytes, 4-byte aligned: global segment j's slot at byte
 *              j * VSP_PNG_RAGGED_SLOT_BYTES, then int32 seg_bytes[segments], then one filter-type byte per row
 *   out        image i's zlib payload, its segments back to back, at out + out_off, idat_bytes[i] bytes long (at most
 *              vsp_png_ragged_image_bound(h, w, C) = n + 10 per segment); no byte behind it is written.  out_off need not be aligned
 *   seg_adler  [2 j], [2 j + 1] of global segment j, as above
 * Three launches on the caller's stream, no host synchronisation.  VSP_EINVAL, nothing launched: a null or misaligned pointer, C not 1
 * or 3, n < 0, a size below 1, an image that leaves `src` or starts below the end of the one before it, an output range (out_off, the
 * image bound) that leaves `out` or starts below the end of the one before it, a wrong seg0 or row0, a `work` too small.
 * VSP_ENOTSUP, nothing launched: C w above VSP_PNG_RAGGED_MAX_ROW_BYTES, src, out or work of 2 GiB or more, more than
 * VSP_PNG_RAGGED_MAX_IMAGES images or VSP_PNG_RAGGED_MAX_SEGMENTS segments.  n = 0 returns VSP_OK.  The size helpers return 0 for
 * arguments outside the limits.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_PNG_RAGGED_SEG_BYTES 24576          /* <= 8 x 3073, 48 bytes per thread of 512, a stored block below 65536 */
#define VSP_PNG_RAGGED_SLOT_BYTES 24588         /* SEG_BYTES + 10, rounded up to a dword */
#define VSP_PNG_RAGGED_MAX_ROW_BYTES (1 << 20)  /* C w */
#define VSP_PNG_RAGGED_MAX_IMAGES 4096
#define VSP_PNG_RAGGED_MAX_SEGMENTS 65535       /* 1.5 GiB of filtered bytes per call */

typedef struct vsp_png_item {
  int64_t src_off;   /* byte offset of the (h, w, C) image in `src`, rows of C w bytes without padding */
  int64_t out_off;   /* byte offset of its zlib payload in `out` */
  int32_t h, w;
  int32_t seg0;      /* index of its first segment among all segments of the call */
  int32_t row0;      /* index of its first row among all rows of the call */
} vsp_png_item;

int vsp_png_ragged_segments(int H, int W, int C);
size_t vsp_png_ragged_image_bound(int H, int W, int C);
size_t vsp_png_ragged_work_bytes(int64_t segments, int64_t rows);
int vsp_png_encode_ragged_u8(uint8_t* out, size_t out_bytes, int32_t* idat_bytes, uint32_t* seg_adler, uint8_t* work, size_t work_bytes,
                             const uint8_t* src, size_t src_bytes, const vsp_png_item* items, const vsp_png_item* items_dev, int n, int C,
                             vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * No-reference quality: the NIQE features (Mittal, Soundararajan, Bovik 2013) of B uint8 RGB images (B, H, W, 3), one launch,
 * no host synchronisation (csrc/niqe.hip).
 *   luma       Y = round-half-even(16 + (65.481 R + 128.553 G + 24.966 B) / 255), exact in integers; crop_border pixels are cut
 *              from every side, then the image is cut at the top left to multiples of 96: nby x nbx blocks, nblk = nby * nbx >= 2
 *   scales     s = 1: Y, blocks of 96; s = 2: the bicubic antialiased half-size image, taps [-3 -9 29 111 111 29 -9 -3] / 256 at
 *              input rows 2i - 3 .. 2i + 4, symmetric reflection (-1 -> 0), rows then columns, blocks of 48
 *   MSCN       mu = 7 x 7 Gaussian (sigma 7/6, normalised, separable), edge replicate on that scale's own image;
 *              sigma_loc = sqrt|G * x^2 - mu^2|; v = (x - mu) / (sigma_loc + 1)
 *   maps       per block and scale five maps: v, and v * roll(v, s) for s = (0,1), (1,0), (1,1), (1,-1), the roll circular in the block
 *   moments    per map six raw moments in float64: n-, sum- v^2, n+, sum+ v^2, sum |v|, sum v^2 (a zero lies on neither side);
 *              moments (B, nblk, 2, 5, 6), may be NULL
 *   features   (B, nblk, 36) float64, scale 1 then scale 2, per scale [alpha, (bl + br) / 2] of v and [alpha, (br - bl) *
 *              G(2/alpha) / G(1/alpha), bl, br] of each product, from the asymmetric generalised Gaussian fit by moments:
 *              ls = sqrt(sum- / n-), rs = sqrt(sum+ / n+), g = ls / rs, rhat = mean|v|^2 / mean v^2,
 *              rnorm = rhat (g^3 + 1)(g + 1) / (g^2 + 1)^2, alpha = the grid point whose r is nearest rnorm (the first of equals),
 *              b = std * sqrt(G(1/alpha) / G(3/alpha)).  A map with an empty side gives NaN
 *   sharpness  (B, nblk) float: the mean sigma_loc of the scale-1 block (what the pristine-model fit selects blocks by)
 *   rgam_table 4 x 9801 float64 on the device, built once by the caller for gamma_k = 0.2 + 0.001 k: gamma, r(gamma) = G(2/gamma)^2 /
 *              (G(1/gamma) G(3/gamma)), sqrt(G(1/gamma) / G(3/gamma)), G(2/gamma) / G(1/gamma)
 *   work       vsp_niqe_work_bytes(...) bytes; 0 in this version (every reduction ends in the block's own workgroup), may be NULL
 * A block's bits depend on its own pixels only: not on B, the position in the batch, or the launch.
 * VSP_EINVAL, nothing written: crop_border < 0, fewer than two blocks left, a null features / sharpness / img / rgam_table.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_NIQE_BLOCK 96
#define VSP_NIQE_FEATURES 36
#define VSP_NIQE_GAMMAS 9801
size_t vsp_niqe_work_bytes(int B, int H, int W, int crop_border);
int vsp_niqe_features_u8(double* features, double* moments_or_null, float* sharpness, const uint8_t* img, int B, int H, int W,
                         int crop_border, const double* rgam_table, void* work, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Faces inside whole photos (csrc/face_warp.hip): the aligned S x S crop of every face of a ragged batch of packed RGB
 * photos, and the feathered paste-back of the restored crops into the output photos.  Integer fixed point throughout, so the bytes
 * equal tests/photo_ref.py.  The host (vspbfr_amd/photo.py) turns a face's float64 2 x 3 matrix M, destination -> source, into
 * int32 tables for the destination columns x and rows y it covers (rne = round half to even):
 *     ax[x] = rne(M00 x 1024)   bx[x] = rne(M10 x 1024)   cx[y] = rne((M01 y + M02) 1024) + 16   cy[y] = rne((M11 y + M12) 1024) + 16
 *     X = (cx[y] + ax[x]) >> 5,  Y = (cy[y] + bx[x]) >> 5        Q5 source coordinates (arithmetic shifts)
 *     ix = X >> 5, fx = X & 31, iy = Y >> 5, fy = Y & 31
 *     v  = (sum_{i,j in {0,1}} 32 (i ? fx : 32 - fx)(j ? fy : 32 - fy) p(ix + i, iy + j) + 16384) >> 15     (the weights sum to 2^15)
 * A face's tables lie at int32 offset tab_off of `tables` as ax[nx], bx[nx], cx[ny], cy[ny].  `tables`, `items`, `tiles`, `tile_faces`
 * and `ramp` are given twice: in HOST memory, where every entry is checked before anything is launched, and in device memory, which
 * the kernels read.  VSP_EINVAL, nothing launched: a null pointer, a table entry of magnitude 2^30 or more, an offset outside its
 * buffer, a size above the limits, a buffer of 2 GiB or more.
 *
 * vsp_face_crop_u8   src: the packed photos, face i's (h, w, 3) photo at byte offset src_off, rows of 3 w bytes without padding;
 *                    M = A^-1 (crop -> photo), nx = ny = S; a tap outside the photo reads the border colour.
 *                    out_u8 (n, S, S, 3) uint8 and / or out_f32 (n, 3, S, S) fp32 = ((v / 255) - 0.5) / 0.5, three separately rounded
 *                    operations as vsp_lanczos_resize_u8 writes them; either may be NULL, not both.
 * vsp_face_paste_u8  in place on `photos`, the packed output photos.  Face i's source is the restored crop at byte offset src_off of
 *                    `crops` (h = w = S); M = P (output photo -> crop); its tables cover the columns x0 .. x0 + nx - 1 and the rows
 *                    y0 .. y0 + ny - 1 of its bounding box in the output photo.  One workgroup per tile of VSP_FACE_TILE^2 pixels; the
 *                    tiles ascend strictly by (photo, y0, x0), so a pixel belongs to one thread.  A pixel walks its tile's faces
 *                    (tile_faces[face0 .. face0 + nfaces - 1], ascending face indices) in order:
 *                        d = min(X, Y, (S - 1) 32 - X, (S - 1) 32 - Y);  d < 0: the face does not touch the pixel; otherwise
 *                        w = ramp[min(d >> 2, ramp_len - 1)],  f = v of the crop with tap indices clamped to S - 1,
 *                        out = (w f + (256 - w) bg + 128) >> 8,  bg the running result.
 *                    ramp: uint16 0..256 indexed by the distance from the crop border in 1/8 px, ramp[0] = 0 (else VSP_EINVAL).
 * ---------------------------------------------------------------------------------------------- */
#define VSP_FACE_TILE 32          /* paste tile side; tile origins are multiples of it */
#define VSP_FACE_MAX_SIDE 8192    /* crop side S and the extents of one face's tables */
#define VSP_FACE_MAX_ITEMS 65535  /* faces per launch */
#define VSP_FACE_MAX_RAMP 65536   /* ramp entries */

typedef struct vsp_face_item {
  int64_t src_off;   /* crop: byte offset of the face's photo in `src`; paste: byte offset of its restored crop in `crops` */
  int64_t tab_off;   /* int32 offset of its tables in `tables`: ax[nx], bx[nx], cx[ny], cy[ny] */
  int32_t h, w;      /* size of the image at src_off (paste: S, S) */
  int32_t x0, y0;    /* paste: origin of the clipped bounding box in the output photo; crop: 0, 0 */
  int32_t nx, ny;    /* destination columns and rows the tables cover (crop: S, S) */
} vsp_face_item;

typedef struct vsp_face_tile {
  int64_t dst_off;   /* byte offset of the tile's output photo in `photos` */
  int32_t h, w;      /* size of that photo */
  int32_t x0, y0;    /* tile origin in the photo, multiples of VSP_FACE_TILE */
  int32_t face0;     /* first entry of the tile's faces in `tile_faces` */
  int32_t nfaces;    /* >= 1 */
} vsp_face_tile;

int vsp_face_crop_u8(uint8_t* out_u8, float* out_f32, const uint8_t* src, size_t src_bytes, const int32_t* tables, const int32_t* tables_dev,
                     size_t table_ints, const vsp_face_item* items, const vsp_face_item* items_dev, int n, int S, int border_r, int border_g,
                     int border_b, vsp_stream_t stream);
int vsp_face_paste_u8(uint8_t* photos, size_t photo_bytes, const uint8_t* crops, size_t crop_bytes, const int32_t* tables,
                      const int32_t* tables_dev, size_t table_ints, const vsp_face_item* items, const vsp_face_item* items_dev, int n, int S,
                      const vsp_face_tile* tiles, const vsp_face_tile* tiles_dev, int ntiles, const int32_t* tile_faces,
                      const int32_t* tile_faces_dev, size_t tile_face_ints, const uint16_t* ramp, const uint16_t* ramp_dev, int ramp_len,
                      vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Anti-aliased face crop and paste-back (csrc/face_warp.hip; bytes equal tests/photo_aa_ref.py).  Supersets of the two
 * entries above: an item with reach == 0 is resampled by the four bilinear taps exactly as there, an item with reach > 0 by a tent
 * filter one DESTINATION pixel wide along the destination's axes, evaluated at source lattice points.  For F (2 x 3, source ->
 * destination; crop: A, paste: P^-1) the host builds forward tables over the source columns qx = sx0 .. sx0 + snx - 1 and rows
 * qy = sy0 .. sy0 + sny - 1 (the range may start below 0 and end past the image), at int32 offset fwd_off of `fwd` as fu[snx],
 * fv[snx], gu[sny], gv[sny]:
 *     fu[qx] = rne(F00 qx 1024)   fv[qx] = rne(F10 qx 1024)   gu[qy] = rne((F01 qy + F02) 1024)   gv[qy] = rne((F11 qy + F12) 1024)
 *     U = fu[qx] + gu[qy], V = fv[qx] + gv[qy];  for the destination pixel (x, y) in absolute destination coordinates
 *     tu = max(0, 1024 - |U - 1024 x|), tv = max(0, 1024 - |V - 1024 y|), w = (tu tv) >> 8
 *     v_c = (sum w p_c(qx, qy) + (W >> 1)) / W,  W = sum w   (floor division)
 * summed over the window qx = ix - reach .. ix + reach + 1, qy = iy - reach .. iy + reach + 1 around the centre cell (ix, iy) = (X >> 5,
 * Y >> 5) of the destination -> source tables; with reach = ceil(|M00| + |M01| + 0.125), M = F^-1, every tap outside the window has
 * weight 0.  Crop: a point outside the photo reads the border colour; paste: the pixel at the index clamped to 0 .. S - 1.
 * Checked on the host before anything is launched, beyond what the entries above check: reach < 0 is VSP_EINVAL and reach >
 * VSP_FACE_AA_MAX_REACH (a minification above 16) VSP_ENOTSUP; for reach > 0 the forward tables lie inside `fwd` with every entry
 * below 2^30 in magnitude, the destination stays below 2^20 pixels a side, and the source range contains the window of every pixel the
 * item serves.  That last check takes the extremes of the centre tables: every centre column lies between (min cx + min ax) >> 10 and
 * (max cx + max ax) >> 10 (rows: cy, bx), and the range must hold those - reach .. + reach + 1.  `fwd` / `fwd_dev` may be NULL when no
 * item has reach > 0.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_FACE_AA_MAX_REACH 23         /* ceil(16 sqrt(2) + 0.125): a minification of 16 at any turn */
#define VSP_FACE_AA_MAX_RANGE (1 << 18)  /* source columns / rows one item's forward tables may cover */

typedef struct vsp_face_aa_item {
  int64_t src_off;   /* as vsp_face_item */
  int64_t tab_off;
  int64_t fwd_off;   /* int32 offset of the forward tables in `fwd`: fu[snx], fv[snx], gu[sny], gv[sny] */
  int32_t h, w;
  int32_t x0, y0;
  int32_t nx, ny;
  int32_t sx0, sy0;  /* first source column / row the forward tables cover (may be negative) */
  int32_t snx, sny;  /* columns / rows they cover (0 with reach == 0) */
  int32_t reach;     /* 0: four-tap bilinear; 1 .. VSP_FACE_AA_MAX_REACH: the filter over a (2 reach + 2)^2 window */
  int32_t pad_;
} vsp_face_aa_item;

int vsp_face_crop_aa_u8(uint8_t* out_u8, float* out_f32, const uint8_t* src, size_t src_bytes, const int32_t* tables, const int32_t* tables_dev,
                        size_t table_ints, const int32_t* fwd, const int32_t* fwd_dev, size_t fwd_ints, const vsp_face_aa_item* items,
                        const vsp_face_aa_item* items_dev, int n, int S, int border_r, int border_g, int border_b, vsp_stream_t stream);
int vsp_face_paste_aa_u8(uint8_t* photos, size_t photo_bytes, const uint8_t* crops, size_t crop_bytes, const int32_t* tables,
                         const int32_t* tables_dev, size_t table_ints, const int32_t* fwd, const int32_t* fwd_dev, size_t fwd_ints,
                         const vsp_face_aa_item* items, const vsp_face_aa_item* items_dev, int n, int S, const vsp_face_tile* tiles,
                         const vsp_face_tile* tiles_dev, int ntiles, const int32_t* tile_faces, const int32_t* tile_faces_dev,
                         size_t tile_face_ints, const uint16_t* ramp, const uint16_t* ramp_dev, int ramp_len, vsp_stream_t stream);

/* The two paste entries with a face-parsing mask: the arguments, checks and arithmetic of vsp_face_paste_u8 /
 * vsp_face_paste_aa_u8, and `mask_dev`: face i's (S, S) uint16 paste weights 0 .. 256 at element i S S of a device buffer of mask_elems
 * elements (vsp_parse_blur_u16 writes them; the host never reads them).  At a pixel with Q5 crop coordinates (X, Y) the mask is sampled
 * with the four 5-bit taps of the colour, wm = (sum 32 wx wy m + 16384) >> 15, taps past the crop clamped, and the blend weight is
 * w = (ramp[...] wm + 128) >> 8; a mask of all 256 gives the bytes of the unmasked entry.  The anti-aliased entry keeps the tent filter
 * for the colour and the four taps for the mask; wm is clamped to 256, so a weight above 256 acts as 256.  VSP_EINVAL besides the
 * unmasked entries': a null or misaligned mask, fewer than n S S elements.  VSP_ENOTSUP: a mask of 2 GiB or more. */
int vsp_face_paste_mask_u8(uint8_t* photos, size_t photo_bytes, const uint8_t* crops, size_t crop_bytes, const int32_t* tables,
                           const int32_t* tables_dev, size_t table_ints, const vsp_face_item* items, const vsp_face_item* items_dev, int n, int S,
                           const vsp_face_tile* tiles, const vsp_face_tile* tiles_dev, int ntiles, const int32_t* tile_faces,
                           const int32_t* tile_faces_dev, size_t tile_face_ints, const uint16_t* ramp, const uint16_t* ramp_dev, int ramp_len,
                           const uint16_t* mask_dev, size_t mask_elems, vsp_stream_t stream);
int vsp_face_paste_mask_aa_u8(uint8_t* photos, size_t photo_bytes, const uint8_t* crops, size_t crop_bytes, const int32_t* tables,
                              const int32_t* tables_dev, size_t table_ints, const int32_t* fwd, const int32_t* fwd_dev, size_t fwd_ints,
                              const vsp_face_aa_item* items, const vsp_face_aa_item* items_dev, int n, int S, const vsp_face_tile* tiles,
                              const vsp_face_tile* tiles_dev, int ntiles, const int32_t* tile_faces, const int32_t* tile_faces_dev,
                              size_t tile_face_ints, const uint16_t* ramp, const uint16_t* ramp_dev, int ramp_len, const uint16_t* mask_dev,
                              size_t mask_elems, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Colour fix for restored faces (csrc/color_fix.hip; bytes equal tests/color_fix_ref.py).  crop, restored, out: packed
 * uint8 (F, S, S, 3) on the device; out may be `restored` itself (any other overlap of out with an input is VSP_EINVAL).  Integer
 * arithmetic only, per face and channel, shifts arithmetic, // floor division:
 *
 *   validity  pixel (x, y) of face i is valid iff the centre cell of its crop tables lies inside its photo:
 *                 0 <= (cx[y] + ax[x]) >> 10 < w  and  0 <= (cy[y] + bx[x]) >> 10 < h      (items[i], vsp_face_crop_u8's tables)
 *             -- the same rule for the bilinear and the anti-aliased crop.  items == tables == NULL: every pixel is valid.
 *   VSP_COLOR_FIX_WAVELET (levels L = 1 .. VSP_COLOR_FIX_MAX_LEVELS)
 *                 d = valid ? (c - r) 64 : 0
 *                 for l = 0 .. L - 1, s = 2^l, indices clamped to [0, S - 1]:
 *                     d = (d[x - s] + 2 d[x] + d[x + s] + 2) >> 2 along x over the whole plane, then the same along y
 *                 out = clamp(r + ((d + 32) >> 6), 0, 255)
 *   VSP_COLOR_FIX_STATS   N valid pixels, sums over them, 64-bit:  S1c = sum c, S2c = sum c^2, S1r, S2r likewise
 *                 vc = ((N S2c - S1c^2) 256) // N^2,  vr likewise;  g = clamp(isqrt((vc << 24) // max(vr, 1)), 1024, 16384)
 *                 mc = (S1c 256 + N // 2) // N,  mr likewise;  out = clamp((g (r 256 - mr) + mc 4096 + 2^19) >> 20, 0, 255)
 *                 N = 0: out = r.  `levels` is checked and otherwise unused.  S above VSP_COLOR_FIX_STATS_MAX_SIDE: VSP_ENOTSUP
 *                 (the 64-bit products above hold up to there).
 *
 * scratch: device memory, 16-byte aligned, that the call may overwrite: 12 F S^2 bytes for the wavelet (two int16 (F, 3, S, S)
 * planes), 128 F bytes for the statistics (sixteen 64-bit sums per face, zeroed by the call).  Nothing is copied to the host.
 * `items` / `tables` are read on the host for the checks, `items_dev` / `tables_dev` are the same data in device memory.
 * VSP_EINVAL, nothing launched: a null pointer, F < 0, S < 1 or above VSP_FACE_MAX_SIDE, levels outside 1 .. 6, an unknown mode, a
 * buffer of 2 GiB or more, a scratch too small or misaligned, only some of the four item / table pointers given, an item whose table
 * extents are not S x S, whose photo size is not positive or whose tables leave `tables`, a table entry of magnitude 2^30 or more.
 * F = 0 returns VSP_OK.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_COLOR_FIX_STATS 0
#define VSP_COLOR_FIX_WAVELET 1
#define VSP_COLOR_FIX_MAX_LEVELS 6
#define VSP_COLOR_FIX_STATS_MAX_SIDE 1024

int vsp_color_fix_u8(const uint8_t* crop, const uint8_t* restored, uint8_t* out, int F, int S, int mode, int levels,
                     const vsp_face_item* items, const vsp_face_item* items_dev, const int32_t* tables, const int32_t* tables_dev,
                     size_t table_ints, void* scratch, size_t scratch_bytes, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Device-side JPEG encoder: the entropy-coded segments of a ragged batch of packed RGB uint8 images (csrc/jpeg.hip).
 * Baseline sequential DCT, 8 bits, YCbCr, 4:4:4 or 4:2:0, the Annex K quantisation tables scaled by `quality` as libjpeg's
 * jpeg_set_quality(q, TRUE) scales them, the Annex K Huffman tables, a restart interval of `restart` MCUs.  The host frames the file
 * (vspbfr_amd/jpeg.py assemble: SOI, JFIF APP0, 2 DQT, SOF0, 4 DHT, DRI, SOS, the segment, EOI); tests/jpeg_ref.py restates every
 * step in NumPy and the files equal Pillow's save(quality, subsampling, restart_marker_blocks = restart) byte for byte.
 *
 *   pixels     jccolor's 16-bit fixed point RGB -> YCbCr; 4:2:0 chroma = h2v2 box with the alternating 1 / 2 bias; columns and rows
 *              past the image repeat the last one, a chroma row past the last downsampled row repeats that row (csrc/jpeg_common.h)
 *   blocks     ISLOW forward DCT, quantised by round-half-away(c / (8 q)).  4:2:0 MCU = 16 x 16 pixels: Y00 Y01 Y10 Y11 Cb Cr; a luma
 *              block that starts past ceil(w / 8) columns or ceil(h / 8) rows is a dummy as the compressor makes it: AC zero, DC that
 *              of the previous block of the MCU.  4:4:4 MCU = 8 x 8 pixels: Y Cb Cr
 *   intervals  image i has M = MCUs across x down, ceil(M / restart) intervals; interval k codes the MCUs k restart .. in raster
 *              order with the DC predictors reset to 0, is padded with 1-bits to a byte, and `FF` bytes are followed by `00`.
 *              The kernel codes every interval on its own into a slot of `work` (global interval j at byte j * slot, slot =
 *              vsp_jpeg_interval_bound(min(restart, largest M of the call), subsampling)), then a scan and a gather write image i's
 *              segment at out + out_off: interval 0, FF D0, interval 1, FF D1, ... the marker number cycling 0..7, none behind the
 *              last interval.  totals[i] = bytes of that segment (at most vsp_jpeg_image_bound(h, w, restart, subsampling))
 *   items      given twice: in host memory, checked before anything is launched, and the same table in device memory.  interval0 =
 *              the number of intervals of the items before it (item 0: 0)
 *   interval_ws  2 x (intervals of the call) int32 of device memory: byte counts, then offsets
 * VSP_EINVAL, nothing launched: a null pointer, n outside 0 .. VSP_JPEG_MAX_ITEMS, quality outside 1..100, a subsampling other than
 * VSP_JPEG_444 / VSP_JPEG_420, restart outside 1..65535, h or w outside 1..65535, an image outside `src`, a segment bound outside
 * `out`, a wrong interval0, a `work` too small.  VSP_ENOTSUP: src, out or work of 2 GiB or more (the caller encodes on the host).
 * n = 0 returns VSP_OK.  The bounds return 0 for arguments outside the limits.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_JPEG_444 0            /* Pillow's subsampling numbers */
#define VSP_JPEG_420 2
#define VSP_JPEG_MAX_ITEMS 65535
#define VSP_JPEG_BLOCK_BOUND 416  /* bytes one coded block can take: (22 + 63 x 26) bits, every byte stuffed */

typedef struct vsp_jpeg_item {
  int64_t src_off;     /* byte offset of the (h, w, 3) image in `src`, rows of 3 w bytes without padding */
  int64_t out_off;     /* byte offset of its entropy-coded segment in `out` */
  int32_t h, w;
  int32_t interval0;   /* index of its first restart interval among all intervals of the call */
  int32_t pad_;
} vsp_jpeg_item;

/* restart intervals of one image (0 for arguments outside the limits) */
int vsp_jpeg_intervals(int h, int w, int restart, int subsampling);
/* bytes of the slot of an interval of `mcus` MCUs */
size_t vsp_jpeg_interval_bound(int mcus, int subsampling);
/* bytes an image's segment can take, markers included */
size_t vsp_jpeg_image_bound(int h, int w, int restart, int subsampling);
int vsp_jpeg_encode_u8(uint8_t* out, size_t out_bytes, int32_t* totals, uint8_t* work, size_t work_bytes, int32_t* interval_ws,
                       const uint8_t* src, size_t src_bytes, const vsp_jpeg_item* items, const vsp_jpeg_item* items_dev, int n,
                       int quality, int subsampling, int restart, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Device-side JPEG decoder: a ragged batch of baseline scans -> packed (h, w, 3) RGB uint8 images (csrc/jpeg_decode.hip).
 * The host reads the markers in front of the scan (vspbfr_amd/jpeg.py parse) and hands over, per image, the entropy-coded bytes (from
 * the byte behind the SOS header to the end of the file), the three quantisation tables and the six Huffman tables its components
 * select.  Served: SOF0, 8 bits, Y Cb Cr, 4:4:4 or 4:2:0, one interleaved scan, any 8-bit quantisers, any Huffman tables, a restart
 * interval or none.  tests/jpeg_dec_ref.py restates every step in NumPy; the pixels equal Pillow's Image.open(f).convert("RGB")
 * (libjpeg's default decode: ISLOW inverse DCT, fancy h2v2 upsampling, jdcolor) byte for byte.
 *
 *   unstuff    the scan ends at the first marker other than RSTm; `00` behind a data `FF`, `FF` fill bytes and the RSTm markers are
 *              dropped, every RSTm opens the next restart interval.  An image without a restart interval is one interval
 *   entropy    an interval is cut into subsequences of `sub_bytes` clean bytes.  The decoder's state between two symbols is (block of
 *              the MCU, zig-zag position).  Round 0 decodes every subsequence from its first bit in state (0, 0) until the bit position
 *              reaches the subsequence's end and records the exit (bit position, state, blocks completed).  Round r + 1 decodes
 *              subsequence i + 1 from the exit of i that round r recorded, if round r changed it.  The rounds end when one changed
 *              nothing (at most: subsequences + 1); rounds[i] = the largest number of rounds, round 0 and the unchanged one included,
 *              that an interval of image i took (1 for a single subsequence).  The true pass then stores the coefficients
 *   symbols    the first length 1..16 at which the prefix is a code; none: one bit is consumed.  The symbol's low nibble s is the
 *              number of value bits (consumed whatever s is).  DC: symbol > 11 is a bad category.  AC: s = 0 with run 15 skips 16
 *              positions, any other s = 0 ends the block (a run with it is an error); otherwise k += run, and k > 63 ends the block
 *              without a store.  Bits past the interval's end read as 1; in the interval's last subsequence fewer than 8 remaining bits,
 *              all 1, in state (0, 0) are the padding.  Blocks past the interval's expected count are not stored
 *   pixels     DC prediction per component within the interval, dequantisation, ISLOW inverse DCT + range limit; 4:2:0: fancy
 *              upsampling over the ceil(w / 2) x ceil(h / 2) real chroma samples (the last real row / column repeats), plain 2 x 2
 *              replication where ceil(w / 2) <= 2, as jdsample.c chooses; jdcolor
 *   status[i]  0, or the OR of VSP_JPEG_DEC_*: the caller decodes such an image on the host.  Events of the speculative rounds do
 *              not count, only those of the true pass
 *   items      given twice: in host memory, checked before anything is launched, and the same table in device memory; so are the
 *              tables: per image VSP_JPEG_DEC_TABLE_BYTES = 3 x 64 quantisers (uint8, natural order, component 0 1 2), then 6 x
 *              (16 BITS + 256 HUFFVAL): DC and AC table of component 0, of 1, of 2.  interval0 = the intervals of the items before,
 *              work_off = the sum of vsp_jpeg_decode_work_bytes of the items before
 * VSP_EINVAL, nothing launched: a null pointer (rounds may be null), n outside 0 .. VSP_JPEG_MAX_ITEMS, sub_bytes not a multiple of 4 in
 * 4..4096, h or w outside 1..65535, a subsampling other than VSP_JPEG_444 / VSP_JPEG_420, restart outside 0..65535, a scan of less than
 * 1 or more than VSP_JPEG_DEC_MAX_SCAN_BYTES bytes, an item outside `in` or `out`, an out_off below the end of the item before (the images
 * ascend in `out` and do not overlap), a wrong interval0 or work_off, a BITS array with more than 256 codes or one that fills or
 * overfills the code space (the all-ones code must stay free: the 1-bit padding of an interval is told from a code by it), a `work` too small or not 16-byte aligned.  VSP_ENOTSUP: in, out or work of
 * 2 GiB or more.  n = 0 returns VSP_OK.  vsp_jpeg_decode_work_bytes returns 0 for arguments outside the limits.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_JPEG_DEC_TABLE_BYTES 1824
#define VSP_JPEG_DEC_MAX_SCAN_BYTES 0x0FFFFFFF   /* bit positions stay below 2^31 */
#define VSP_JPEG_DEC_COEF_LIMIT 16383            /* twice what 8-bit samples can give a dequantised coefficient */
#define VSP_JPEG_DEC_NO_EOI 1          /* the data ends without a marker */
#define VSP_JPEG_DEC_STRAY_MARKER 2    /* the scan ends at a marker other than EOI */
#define VSP_JPEG_DEC_RST_ORDER 4       /* an RSTm number that does not cycle 0..7 */
#define VSP_JPEG_DEC_RST_COUNT 8       /* intervals other than ceil(MCUs / restart) */
#define VSP_JPEG_DEC_BAD_CODE 16       /* a prefix that matches no code */
#define VSP_JPEG_DEC_BAD_CATEGORY 32   /* a category above 11 (DC) or 10 (AC) */
#define VSP_JPEG_DEC_RUN 64            /* a run that carries k past 63, or a run beside an end of block */
#define VSP_JPEG_DEC_BLOCK_COUNT 128   /* an interval that does not end on its last block's last bit (+ padding) */
#define VSP_JPEG_DEC_COEF_RANGE 256    /* a dequantised coefficient beyond VSP_JPEG_DEC_COEF_LIMIT */

typedef struct vsp_jpeg_dec_item {
  int64_t in_off;      /* byte offset of the entropy-coded data in `in` */
  int64_t out_off;     /* byte offset of the (h, w, 3) image in `out`, rows of 3 w bytes without padding */
  int64_t work_off;    /* byte offset of its work area in `work` */
  int32_t in_len;      /* bytes of entropy-coded data (up to the end of the file: the kernel finds the EOI) */
  int32_t h, w;
  int32_t subsampling; /* VSP_JPEG_444 or VSP_JPEG_420 */
  int32_t restart;     /* MCUs per restart interval, 0 = none */
  int32_t interval0;   /* index of its first restart interval among all intervals of the call */
} vsp_jpeg_dec_item;

/* bytes of one image's work area (a multiple of 16) */
size_t vsp_jpeg_decode_work_bytes(int h, int w, int in_len, int subsampling, int restart, int sub_bytes);
int vsp_jpeg_decode_u8(uint8_t* out, size_t out_bytes, int32_t* status, int32_t* rounds, uint8_t* work, size_t work_bytes, const uint8_t* in,
                       size_t in_bytes, const vsp_jpeg_dec_item* items, const vsp_jpeg_dec_item* items_dev, const uint8_t* tables,
                       const uint8_t* tables_dev, int n, int sub_bytes, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Face detection for whole photos: RetinaFace with the MobileNet-0.25 backbone in fp32 and its post-processing (csrc/detect.hip,
 * vspbfr_amd/detect.py).  Activations are NCHW fp32; BatchNorm is folded into weight and bias on the host.  `act`: 0 = none,
 * 1 = x < 0 ? slope x : x (slope 0 is ReLU).  tests/detect_ref.py restates the network in torch (float64 / float32) and the
 * post-processing in NumPy.
 *
 *   entry      the first layer on the u8 photos: y (B, 8, ceil(Hc/2), ceil(Wc/2)) = act(conv3x3 stride 2 pad 1 of the canvas + b).  The
 *              canvas (B, 3, Hc, Wc) is never stored: item i's (h, w, 3) RGB photo lies at the top-left of canvas `slot`, channel c of
 *              the canvas is photo channel 2 - c minus mean (104, 117, 123)[c], and everything outside the photo is 0.  w is
 *              [ci 3][tap 9][co 8].  A call writes the slots of its items in full and no other; items are given in host and device memory
 *   sep        one depthwise-separable block: t = act(dw3x3 stride s pad 1 of x + bd), y = act(pw1x1 of t + bp), slope for both; t stays
 *              in LDS.  wd is [Cin][9], wp [Cin][Cout].  Cin 1..256, Cout a multiple of 16 up to 256, stride 1 or 2,
 *              OH = (H - 1) / s + 1
 *   conv3x3    dense 3x3 stride 1 pad 1, w [Cin][9][Cout], Cin a multiple of 8, Cout 16, 32 or 64; y has y_ch channels and the result
 *              goes to channels y_coff .. y_coff + Cout - 1 (the SSH concatenation)
 *   lateral    y = act(conv1x1 of x + b) + up[b][co][floor(oy h2 / H)][floor(ox w2 / W)] (up may be null: no addition);
 *              w [Cin][64], Cout = 64
 *   heads      one level: 32 channels = conv1x1 of x (B, 64, H, W) with w [64][32] + b, channels 0..3 class, 4..11 box, 12..31
 *              landmarks, written for cell p and anchor a as prior p0 + 2 p + a of conf (B, P, 2), loc (B, P, 4), lm (B, P, 10)
 *   decode_nms per image, one workgroup: priors from the index -- level k = 0, 1, 2 has step 8, 16, 32, ceil(Hc / step)
 *              x ceil(Wc / step) cells in raster order, two anchors of size (16, 32), (64, 128), (256, 512) per cell, centre
 *              ((j + 0.5) step, (i + 0.5) step) --; score = 1 / (1 + exp(l0 - l1)); box centre c + loc[0:2] 0.1 m, size m exp(0.2
 *              loc[2:4]); landmark k = c + lm[2k:2k+2] 0.1 m; all in canvas pixels.  Candidates: score > threshold with a finite box
 *              and landmarks; the first max_candidates in the order (score descending, prior ascending) survive; greedy NMS in that
 *              order, suppressed when IoU (plain areas) with a kept one > nms; the first max_faces kept ones are written to
 *              faces[b * max_faces ..].  info[4 b ..] = faces written, status (VSP_DET_*), candidates before the cap, non-finite dropped.
 *              No loop is bounded by data and none waits for another thread's write outside a barrier.
 * VSP_EINVAL, nothing launched: a null pointer, a dimension outside the limits above, B < 0, an item outside `src` or a slot outside
 * 0 .. B - 1, threshold outside [0, 1), nms outside [0, 1], max_candidates outside 1 .. VSP_DET_MAX_CANDIDATES, max_faces < 1, a `work`
 * too small or not 16-byte aligned.  VSP_ENOTSUP: a tensor or buffer of 2 GiB or more.  B = 0 (n = 0) returns VSP_OK.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_DET_MAX_CANDIDATES 2048
#define VSP_DET_MAX_SIDE 8192          /* canvas side */
#define VSP_DET_CAND_CAPPED 1          /* more than max_candidates candidates */
#define VSP_DET_FACES_CAPPED 2         /* more than max_faces faces survive the NMS */
#define VSP_DET_NONFINITE 4            /* a candidate with a non-finite box or landmark was dropped */

typedef struct vsp_det_src {
  int64_t off;         /* byte offset of the (h, w, 3) RGB photo in `src`, rows of 3 w bytes without padding */
  int32_t h, w;
  int32_t slot;        /* image of the canvas batch it goes to */
  int32_t pad_;
} vsp_det_src;

typedef struct vsp_det_face {
  float box[4];        /* x1 y1 x2 y2, canvas pixels */
  float score;
  float lm[10];        /* x y of left eye, right eye, nose, left and right mouth corner */
  int32_t prior;
} vsp_det_face;

int vsp_det_entry_u8(float* y, const uint8_t* src, size_t src_bytes, const vsp_det_src* items, const vsp_det_src* items_dev, int n,
                     const float* w, const float* b, int B, int Hc, int Wc, int act, float slope, vsp_stream_t stream);
int vsp_det_sep_f32(float* y, const float* x, const float* wd, const float* bd, const float* wp, const float* bp, int B, int Cin, int Cout,
                    int H, int W, int stride, float slope, vsp_stream_t stream);
int vsp_det_conv3x3_f32(float* y, const float* x, const float* w, const float* b, int B, int Cin, int Cout, int H, int W, int y_ch,
                        int y_coff, int act, float slope, vsp_stream_t stream);
int vsp_det_lateral_f32(float* y, const float* x, const float* w, const float* b, const float* up, int B, int Cin, int H, int W, int h2,
                        int w2, int act, float slope, vsp_stream_t stream);
int vsp_det_heads_f32(float* conf, float* loc, float* lm, const float* x, const float* w, const float* b, int B, int H, int W, int P,
                      int p0, vsp_stream_t stream);
/* priors of a canvas (0 for sides outside 1 .. VSP_DET_MAX_SIDE) */
int vsp_det_priors(int Hc, int Wc);
/* bytes of `work` for one call (0 for arguments outside the limits) */
size_t vsp_det_work_bytes(int B, int Hc, int Wc, int max_candidates);
int vsp_det_decode_nms_f32(vsp_det_face* faces, int32_t* info, uint8_t* work, size_t work_bytes, const float* conf, const float* loc,
                           const float* lm, int B, int Hc, int Wc, float threshold, float nms, int max_candidates, int max_faces,
                           vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Background upscaling for whole photos (csrc/sr.hip): Real-ESRGAN's compact network (SRVGGNetCompact, 64 features) with
 * f16 operands and fp32 accumulation.  Activations are (h, w, 64) _Float16 per item, the items of a group back to back in a buffer of
 * act_bytes; one launch per layer serves the whole ragged group through the item table (`items` on the host for the checks,
 * `items_dev` the same bytes on the device).  The tile list (VSP_SR_TILE_H rows x VSP_SR_TILE_W columns) runs across the items:
 * items[i].tile0 = sum over j < i of ceil(h_j / VSP_SR_TILE_H) ceil(w_j / VSP_SR_TILE_W).
 *   head   y = PReLU(conv3x3(src / 255) + b): 3 -> 64, zero padding, fp32 fmaf; w is (27, 64) fp32, row (3 ky + kx) 3 + c.
 *   body   y = PReLU(conv3x3(x) + b): 64 -> 64 on v_mfma_f32_16x16x32_f16; b, slope fp32 (64); y must not be x.
 *          w_img: the f16 image of upscale.pack_body_weight, 18 x NB x 64 x 8 halves (NB = 4): element j of lane l of block nb of
 *          K-step s = w[co = 16 nb + (l & 15)][ci = 32 (s & 1) + 8 (l >> 4) + j][ky = (s >> 1) / 3][kx = (s >> 1) % 3].
 *   tail   v = conv3x3(x) + b + src / 255 of the pixel the output pixel lies in: 64 -> 3 scale^2, channel c scale^2 + dy scale + dx ->
 *          output pixel (scale y + dy, scale x + dx), colour c; w_img as the body's with NB = 1 (scale 2) or 3 (scale 4), the channels
 *          past 3 scale^2 zero, b padded to 16 NB.  out byte = rintf(255 clamp(v, 0, 1)); rows keep0 .. keep0 + keepn - 1 of the item
 *          are written, row keep0 at out_off, rows of 3 scale w bytes.  A non-finite v is written as 0 and ORs VSP_SR_NONFINITE into
 *          info[slot] (the caller zeroes info).  out_f32 (or null): v itself at the same element index as the byte.
 * VSP_EINVAL, nothing launched: a null pointer, a scale other than 2 or 4, h or w < 1, an item outside one of its buffers, rows outside
 * the item, a slot outside 0 .. n_info - 1, a tile0 that is not the running tile count, more than VSP_SR_MAX_ITEMS items, a buffer
 * that is not 16-byte aligned.  VSP_ENOTSUP: a buffer of 2 GiB or more.  n = 0 returns VSP_OK.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_SR_TILE_H 8
#define VSP_SR_TILE_W 32
#define VSP_SR_MAX_ITEMS 65536
#define VSP_SR_NONFINITE 1             /* info bit: a value was not finite before the clamp */

typedef struct vsp_sr_item {
  int64_t src_off;     /* byte offset of the item's (h, w, 3) RGB rows in `src`, rows of 3 w bytes without padding */
  int64_t act_off;     /* pixel offset of the item's (h, w, 64) activation in the activation buffers */
  int64_t out_off;     /* tail: byte offset in `out` of output row scale keep0 of the item */
  int32_t h, w;
  int32_t keep0, keepn; /* tail: the item's rows that are written (a band's rows without its halo) */
  int32_t tile0;       /* first tile of the item in the launch's tile list */
  int32_t slot;        /* tail: index of the item's info word */
} vsp_sr_item;

int vsp_sr_head_u8(void* y, size_t act_bytes, const uint8_t* src, size_t src_bytes, const vsp_sr_item* items, const vsp_sr_item* items_dev,
                   int n, const float* w, const float* b, const float* slope, vsp_stream_t stream);
int vsp_sr_body_f16(void* y, const void* x, size_t act_bytes, const vsp_sr_item* items, const vsp_sr_item* items_dev, int n,
                    const void* w_img, const float* b, const float* slope, vsp_stream_t stream);
int vsp_sr_tail_u8(uint8_t* out, size_t out_bytes, float* out_f32, int32_t* info, int n_info, const void* x, size_t act_bytes,
                   const uint8_t* src, size_t src_bytes, const vsp_sr_item* items, const vsp_sr_item* items_dev, int n, const void* w_img,
                   const float* b, int scale, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Face-parsing paste masks for whole photos (csrc/parse.hip): facexlib's ParseNet with f16 operands and fp32 accumulation,
 * and the integer blur that turns its class map into paste weights.  Activations are (F, H, W, C) _Float16, the faces of a call back
 * to back; every convolution is 3x3 behind a reflection padding of 1 (index -1 -> 1, H -> H - 2), so H, W >= 2 everywhere.
 *   head   y = conv3x3((crops / 255 - 0.5) / 0.5) + b: 3 -> 64, fp32 fmaf; crops (F, H, W, 3) u8; w (27, 64) fp32, row (3 ky + kx) 3 + c.
 *   conv   y = [res2 +] [res1 +] [LeakyReLU 0.2] (conv3x3(x) + b) on v_mfma_f32_16x16x32_f16, one rounding to f16.  x is (F, H, W, Cin);
 *          with VSP_PARSE_UP the convolution sees its nearest x2, (y >> 1, x >> 1), reflected in the upsampled domain.  The output is
 *          (F, OH, OW, Cout), OH = (Hd - 1) / stride + 1 over the domain Hd = H or 2 H.  Cin and Cout are multiples of 64.  w_img: the
 *          f16 image of parse.pack_conv_weight, (Cout / 64, Cin / 64, 18, 4, 64, 8): element j of lane l of block nb of K-step s of
 *          input chunk kc of output block cb = w[co = 64 cb + 16 nb + (l & 15)][ci = 64 kc + 32 (s & 1) + 8 (l >> 4) + j]
 *          [ky = (s >> 1) / 3][kx = (s >> 1) % 3].  b: fp32 (Cout).  res1, res2 (or null): f16 tensors of the output's shape; either
 *          may BE y, no tensor may overlap y otherwise.
 *   mask   logits = conv3x3(x) + b: 64 -> VSP_PARSE_CLASSES in fp32 (w_img (1, 1, 18, 2, 64, 8), the channels past 19 zero; b padded to
 *          32); cls = argmax, a tie to the lowest class; keep = keep_table[cls] (a HOST table of 19 bytes, each 0 or 1); logits (or null)
 *          takes the (F, H, W, 19) fp32 values.  A pixel with a non-finite logit gets class 0 and ORs VSP_PARSE_NONFINITE into info[f]
 *          (F words, zeroed by the caller).
 *   blur   m0 = 16384 keep; four 1-D passes (along x, y, x, y) m' = (sum_{k = -R..R} g[|k|] m[reflect101(i + k)] + 2^15) >> 16; out =
 *          (m + 32) >> 6 in 0 .. 256, the outermost `border` rows and columns 0.  keep (F, S, S) u8, out (F, S, S) u16, work 4 F S S
 *          bytes.  taps: a HOST table of R + 1 non-negative int32 with g[0] + 2 sum_{k >= 1} g[k] = 65536.
 * VSP_EINVAL, nothing launched: a null pointer, channel counts that are not served, H or W < 2, a stride other than 1 or 2, up with
 * stride 2, a buffer off 16-byte alignment, an overlap that is not the aliasing above, taps that do not sum to 65536, R outside
 * 0 .. min(VSP_PARSE_MAX_RADIUS, S - 1), 2 border > S, a work buffer too small.  VSP_ENOTSUP: a tensor of 2 GiB or more.  F = 0
 * returns VSP_OK.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_PARSE_CLASSES 19
#define VSP_PARSE_MAX_RADIUS 64
#define VSP_PARSE_NONFINITE 1          /* info bit: a logit of the face was not finite */
#define VSP_PARSE_ACT 1                /* conv flags */
#define VSP_PARSE_UP 2

int vsp_parse_head_u8(void* y, const uint8_t* crops, int F, int H, int W, const float* w, const float* b, vsp_stream_t stream);
int vsp_parse_conv_f16(void* y, const void* x, int F, int H, int W, int Cin, int Cout, int stride, int flags, const void* w_img,
                       const float* b, const void* res1, const void* res2, vsp_stream_t stream);
int vsp_parse_mask_u8(uint8_t* cls, uint8_t* keep, float* logits, int32_t* info, const void* x, int F, int H, int W, const void* w_img,
                      const float* b, const uint8_t* keep_table, vsp_stream_t stream);
int vsp_parse_blur_u16(uint16_t* out, const uint8_t* keep, uint16_t* work, size_t work_bytes, int F, int S, const int32_t* taps, int R,
                       int border, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * FID on the device (csrc/fid.hip): pytorch-fid's Inception-v3 in fp32 on v_mfma_f32_16x16x4_f32.  Activations are
 * (B, H, W, pitch) float, the images of a call back to back; a tensor is given as a pointer and a channel pitch, an output also as a
 * channel offset, so that the branches of an Inception block write their slices of the concatenated tensor.
 *   stem   y[slot] = ReLU(conv3x3 / 2 (resize(image) / 127.5 - 1) + b): 3 -> 32 without padding, fp32 fmaf.  The n images lie in `src` as
 *          (h, w, 3) u8 at items[i].off; each is resized to (TH, TW) as F.interpolate(mode = "bilinear", align_corners = False) does,
 *          without anti-aliasing (TH = h, TW = w reads the pixels themselves).  y is (B, (TH - 3) / 2 + 1, (TW - 3) / 2 + 1, 32).
 *          w (27, 32), row (3 ky + kx) 3 + c; b (32).  items: host table, items_dev the same bytes on the device.
 *   conv   out[.., c_off : c_off + Cout] = ReLU(conv(x) + bias): filter KH x KW one of 1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1, zero padding
 *          (ph, pw) below the filter extent, stride 1 or 2, Cin and Cout multiples of 16.  x is (B, H, W, x_pitch) of which the first
 *          Cin channels are read; out is (B, OH, OW, c_pitch), OH = (H + 2 ph - KH) / stride + 1.  w (KH, KW, Cin, Cout) fp32 with the
 *          BatchNorm folded in, bias (Cout).  An output element is summed over (ky, kx, ci) in that order, in fmaf chains of 128
 *          products that are then added in order: it has the same bits at any batch size and position.
 *   pool   VSP_FID_POOL_MAX_S2: max 3x3 / 2 without padding; VSP_FID_POOL_AVG_S1: mean over the in-bounds taps of 3x3 / 1 / pad 1
 *          (count_include_pad = False); VSP_FID_POOL_MAX_S1: max 3x3 / 1 / pad 1; VSP_FID_POOL_GLOBAL_AVG: (B, H, W, C) -> (B, C), the
 *          pixels added in row-major order.  No atomics.
 * VSP_EINVAL, nothing launched: a null pointer, channel counts that are not multiples of 16, a filter outside the list, a stride
 * other than 1 or 2, padding >= the filter extent, an empty output, c_pitch < c_off + Cout, x_pitch < Cin, a pitch or offset that is
 * no multiple of 4, a buffer off 16-byte alignment, an output that overlaps its input, an image outside `src`, a slot outside the
 * batch.  VSP_ENOTSUP: a tensor of 2 GiB or more.  B = 0 (n = 0) returns VSP_OK.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_FID_POOL_MAX_S2 0
#define VSP_FID_POOL_AVG_S1 1
#define VSP_FID_POOL_MAX_S1 2
#define VSP_FID_POOL_GLOBAL_AVG 3

int vsp_fid_stem_u8(float* y, const uint8_t* src, size_t src_bytes, const vsp_det_src* items, const vsp_det_src* items_dev, int n, int B,
                    int TH, int TW, const float* w, const float* b, vsp_stream_t stream);
int vsp_fid_conv_f32(float* out, const float* x, const float* w, const float* bias, int B, int H, int W, int Cin, int x_pitch, int Cout,
                     int KH, int KW, int ph, int pw, int stride, int c_off, int c_pitch, vsp_stream_t stream);
int vsp_fid_pool_f32(float* out, const float* x, int B, int H, int W, int C, int x_pitch, int mode, int c_off, int c_pitch,
                     vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Background upscaling with Real-ESRGAN's RRDBNet (csrc/rrdb.hip): x4plus / x2plus, 64 features, growth 32, f16 operands and
 * fp32 accumulation.  One call serves one unit (a photo or a row band).  Activations are (H, W, pitch) _Float16: a tensor is a pointer
 * and a channel pitch, an output also a channel offset, so a dense block is one 192-channel tensor.  Every convolution is 3x3, stride 1,
 * zero padding 1.
 *   head   y = conv_first(net_in) + b, 3 | 12 -> 64 in fp32 fmaf.  The photo lies in `src` as (h, w, 3) u8 at byte src_off.  scale 4:
 *          net_in = photo / 255, (h, w, 3).  scale 2: the photo padded by reflection to even sides (row h -> h - 2, column w -> w - 2)
 *          and pixel-unshuffled by 2, channel 4 c + 2 dy + dx, (ceil(h / 2), ceil(w / 2), 12), all as index arithmetic.  Rows
 *          row0 .. row0 + rows - 1 of the network's input map are written, row row0 at y, y_pitch halves per pixel (channels 0 .. 63).
 *          wt (9 Cin, 64) fp32, row (3 ky + kx) Cin + channel; b (64).
 *   conv   y[.., y_off : y_off + Cout] = f16(s2 (s1 v + r1) + r2), v = [LeakyReLU 0.2] (conv3x3(x[.., 0 : Cin]) + b), on
 *          v_mfma_f32_16x16x32_f16; each residual step is optional (r1 / r2 null), fmaf(s, v, r) in fp32.  x is (H, W, x_pitch); with
 *          VSP_RRDB_UP the convolution sees its nearest x2, (y >> 1, x >> 1), and the output map is (2 H, 2 W), else (H, W).
 *          Cin in {64, 96, 128, 160, 192}, Cout in {32, 64}.  y may be x itself (same pointer, same pitch, no UP) when y_off >= Cin:
 *          conv1 .. conv4 of a dense block write their slices behind the channels they read.  A residual is (ptr, pitch, scale) and
 *          reads channels 0 .. Cout - 1; it may lie in the output tensor only at the same pointer and pitch with y_off >= Cout.
 *          w_img: the f16 image of rrdb.pack_conv_weight, (Cin / 32, 9, Cout / 16, 64, 8): element j of lane l of block nb of tap t of
 *          chunk kc = w[co = 16 nb + (l & 15)][ci = 32 kc + 8 (l >> 4) + j][ky = t / 3][kx = t % 3].  b: fp32 (Cout).
 *   tail   v = conv_last(x) + b, 64 -> 3 (w_img (2, 9, 1, 64, 8), Cout zero-padded to 16; b padded to 16); byte = rintf(255 clamp(v, 0, 1)).
 *          Rows keep0 .. keep0 + keepn - 1 and columns 0 .. out_w - 1 of the (H, W) map are written, row keep0 at out + out_off, rows
 *          out_pitch bytes apart (the x2 crop is out_w < W and a keep window that ends early).  out_f32 (or null): one float per byte
 *          of out, takes v unclamped.  A non-finite v is written as 0 and ORs VSP_RRDB_NONFINITE into info[0] (zeroed by the caller).
 * VSP_EINVAL, nothing launched: a null pointer, channel counts outside the lists, a pitch below the channels used or no multiple of 4
 * halves (8 for a tensor that is read as a convolution input), a misaligned buffer (16 bytes for convolution inputs, weights and
 * biases, 8 for outputs and residuals), an output slice that overlaps the channels read, an aliased residual, a window outside the
 * unit, bytes outside src / out, h or w < 1, an odd side of 1 at scale 2.  VSP_ENOTSUP: a tensor of 2 GiB or more.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_RRDB_NONFINITE 1           /* info bit: a value was not finite before the clamp */
#define VSP_RRDB_ACT 1                 /* conv flags */
#define VSP_RRDB_UP 2

int vsp_rrdb_head_u8(void* y, int y_pitch, const uint8_t* src, size_t src_bytes, int64_t src_off, int h, int w, int scale, int row0, int rows,
                     const float* wt, const float* b, vsp_stream_t stream);
int vsp_rrdb_conv_f16(void* y, int y_pitch, int y_off, const void* x, int x_pitch, int H, int W, int Cin, int Cout, int flags,
                      const void* w_img, const float* b, const void* r1, int r1_pitch, float s1, const void* r2, int r2_pitch, float s2,
                      vsp_stream_t stream);
int vsp_rrdb_tail_u8(uint8_t* out, size_t out_bytes, int64_t out_off, int64_t out_pitch, int out_w, float* out_f32, int32_t* info,
                     const void* x, int x_pitch, int H, int W, int keep0, int keepn, const void* w_img, const float* b, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Face detection with RetinaFace's ResNet-50 network (csrc/detect_r50.hip): f16 operands, fp32 accumulation and biases.
 * Activations are (B, H, W, pitch) _Float16: a tensor is a pointer, a channel pitch and a channel offset.  The post-processing is
 * vsp_det_decode_nms_f32.
 *   stem   y[slot] = f16(relu(conv7x7/2/pad3(canvas) + b)), 3 -> 64 in fp32 fmaf, for the n photos of `items` (as vsp_det_entry_u8: u8
 *          RGB inside `src`, swapped to BGR, minus (104, 117, 123), 0 outside the photo).  y is (B, ceil(Hc / 2), ceil(Wc / 2), 64).
 *          w (147, 64) fp32, row (7 ky + kx) 3 + channel (B, G, R); b (64).
 *   pool   3x3 / 2 / pad 1 maximum over the taps inside the map: (B, H, W, C) -> (B, ceil(H / 2), ceil(W / 2), C), both dense.
 *   conv   y[.., y_off : y_off + Cout] = f16([relu](conv(x[.., x_off : x_off + Cin]) + b [+ res]) [+ up]) on v_mfma_f32_16x16x32_f16.
 *          ksize 1 (no padding) or 3 (padding 1), stride 1 or 2, output map ((H - 1) / stride + 1, (W - 1) / stride + 1); Cin and Cout
 *          multiples of 64 up to 2048.  res (ptr, pitch, offset) is read at the output pixel and may be the very window written (same
 *          pointer, pitch and offset: the bottleneck's sum replaces its identity).  up (ptr, pitch, offset) is an (OH / 2, OW / 2) map
 *          read at (oy >> 1, ox >> 1); OH and OW must be even.  The sum over taps and channels has one fixed order per output pixel:
 *          an image's result depends neither on the batch size nor on its position in the batch.
 *          w_img: the f16 image of detect_r50.pack_conv_weight, (ksize^2, Cin / 32, Cout / 16, 64, 8): element j of lane l of block nb of
 *          step kc of tap t = w[co = 16 nb + (l & 15)][ci = 32 kc + 8 (l >> 4) + j][ky = t / ksize][kx = t % ksize].  b: fp32 (Cout).
 *   heads  the class (4), box (8) and landmark (20) 1x1 heads of one level in fp32 fmaf on channels 0 .. 255 of x: cell (i, j) of image
 *          b writes priors p0 + 2 (i W + j) + {0, 1} of conf (B, P, 2), loc (B, P, 4), lm (B, P, 10).  w (256, 32), b (32) fp32.
 * VSP_EINVAL, nothing launched: a null pointer, a channel count, filter, stride or flag that is not served, a channel window outside
 * its pitch, a pitch or offset that is no multiple of 4 halves (8 for a convolution's input), a misaligned buffer (16 bytes for
 * convolution inputs, weights and biases, 8 for outputs and residuals), an output that overlaps its input, a residual that overlaps the
 * output without being its window, a coarser level that overlaps the output or an odd output map with one, a photo outside `src`,
 * a slot outside the batch, priors outside P.  VSP_ENOTSUP: a tensor of 2 GiB or more.  B = 0 (n = 0) returns VSP_OK.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_DET50_RELU 1               /* conv flags */

int vsp_det50_stem_u8(void* y, const uint8_t* src, size_t src_bytes, const vsp_det_src* items, const vsp_det_src* items_dev, int n,
                      const float* w, const float* b, int B, int Hc, int Wc, vsp_stream_t stream);
int vsp_det50_pool_f16(void* y, const void* x, int B, int H, int W, int C, vsp_stream_t stream);
int vsp_det50_conv_f16(void* y, int y_pitch, int y_off, const void* x, int x_pitch, int x_off, int B, int H, int W, int Cin, int Cout,
                       int ksize, int stride, int flags, const void* w_img, const float* b, const void* res, int res_pitch, int res_off,
                       const void* up, int up_pitch, int up_off, vsp_stream_t stream);
int vsp_det50_heads_f32(float* conf, float* loc, float* lm, const void* x, int x_pitch, const float* w, const float* b, int B, int H, int W,
                        int P, int p0, vsp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Facial landmarks with face_alignment's 2D-FAN (csrc/fan.hip): f16 operands, fp32 accumulation.  Activations are
 * (B, H, W, pitch) _Float16: a tensor is a pointer, a channel pitch and a channel offset.
 *   stem    y = f16(relu(conv7x7/2/pad3(crop) + b)), 3 -> 64 in fp32 fmaf; crop = the box (x0, y0, s) of box[3 b ..] of photo b of src,
 *           (B, H, W, 3) u8 RGB, sampled to side x side bilinearly at half-pixel centres without anti-aliasing, 0 outside the photo,
 *           divided by 255; it is never stored.  y is (B, side / 2, side / 2, 64).  w (147, 64) fp32, row (7 ky + kx) 3 + channel; b (64).
 *   pool    2x2 mean, f16(((a + b) + (c + d)) / 4) in fp32, between channel windows; H and W even.
 *   conv    v = conv(x') [+ b] [relu]; raw = f16(v) (optional); y = v [+ res1] [+ res2] [+ up], rounded once to f16 or, with
 *           VSP_FAN_OUT_F32, stored as fp32 (pitch and offset then count floats).  x' = x, or with in_a / in_b (fp32, Cin each)
 *           f16(max(fmaf(in_a[c], x, in_b[c]), 0)) -- a rounding point; a tap outside the map is 0 behind the affine.  ksize 1 or 3
 *           (padding 1), stride 1.  Cin: a multiple of 32 up to 256 (a 68-channel input is a 96-channel window whose last 28 are zero).
 *           Cout: a multiple of 32 up to 256, or 68.  res1 / res2 (ptr, pitch, offset) are read at the output pixel and may be the very
 *           window written; up is an (H / 2, W / 2) map read at (y >> 1, x >> 1), H and W even.  One fixed order of the sum per output
 *           pixel: an image's result depends neither on the batch size nor on its position in the batch.
 *           w_img: f16 (ksize^2, Cin / 32, Cp / 16, 64, 8), Cp = Cout rounded up to 32 with zero rows: element j of lane l of block nb
 *           of step kc of tap t = w[co = 16 nb + (l & 15)][ci = 32 kc + 8 (l >> 4) + j][ky = t / ksize][kx = t % ksize].  b: fp32 (Cout) or null.
 *   decode  per (image, landmark k < K) of hm (B, n, n, pitch) fp32: argmax (lowest flat index among equals; a non-finite value is
 *           flagged and never wins), lm = x0 + (px + 0.5 + dx) s / n with dx = 0.25 sign(hm[py][px + 1] - hm[py][px - 1]), 0 on the border
 *           (the same in y), peak = the maximum, flag = 1 when the map holds a non-finite value.  lm (B, K, 2), peak (B, K), flag (B, K).
 * VSP_EINVAL, nothing launched: a null pointer, a channel count, filter or flag that is not served, a channel window outside its
 * pitch, a pitch or offset that is no multiple of 4 elements (8 for an input), a misaligned buffer (16 bytes for inputs, weights, biases,
 * affines and fp32 outputs, 8 for f16 outputs and residuals), an output that overlaps its input or the other output, a residual that
 * overlaps the output without being its window, a coarser level that overlaps an output, an odd map with a coarser level or in the pool.
 * VSP_ENOTSUP: a tensor of 2 GiB or more.  B = 0 returns VSP_OK.
 * ---------------------------------------------------------------------------------------------- */
#define VSP_FAN_RELU 1                 /* conv flags */
#define VSP_FAN_OUT_F32 2

int vsp_fan_stem_u8(void* y, const uint8_t* src, const float* box, const float* w, const float* b, int B, int H, int W, int side,
                    vsp_stream_t stream);
int vsp_fan_pool_f16(void* y, int y_pitch, int y_off, const void* x, int x_pitch, int x_off, int B, int H, int W, int C, vsp_stream_t stream);
int vsp_fan_conv_f16(void* y, int y_pitch, int y_off, void* raw, int raw_pitch, int raw_off, const void* x, int x_pitch, int x_off, int B, int H,
                     int W, int Cin, int Cout, int ksize, int flags, const void* w_img, const float* b, const float* in_a, const float* in_b,
                     const void* res1, int res1_pitch, int res1_off, const void* res2, int res2_pitch, int res2_off, const void* up, int up_pitch,
                     int up_off, vsp_stream_t stream);
int vsp_fan_decode_f32(float* lm, float* peak, int32_t* flag, const float* hm, int pitch, const float* box, int B, int n, int K, vsp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VSPBFR_HIP_H */

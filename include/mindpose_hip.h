/*
 * mindpose_hip.h - C ABI of libmindpose_hip.so: the MI355X (gfx950) hot path of the
 * top-down heat-map pose pipeline.
 *
 * The reference (mindspore-lab/mindpose) has no FFI for this path: every function below
 * replaces a MindSpore-op sequence issued from a Python `construct`/`transform` method
 * (file:line cited per entry).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / HIP types in the signatures
 *     (`mp_stream_t` is a hipStream_t passed as void*; NULL = the default stream).
 *   - every pointer marked `dev` is DEVICE memory owned by the caller, contiguous, NCHW, fp32.
 *   - asynchronous on `stream`; no hidden synchronisation, no internal allocation
 *     (scratch comes from a caller-provided workspace sized by mp_*_workspace_bytes).
 *   - returns MP_OK (0) or a negative MP_ERR_* code; never throws, never aborts.
 *   - re-entrant; thread-safe for distinct streams.
 */
#ifndef MINDPOSE_HIP_H
#define MINDPOSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mp_stream_t;

#define MP_OK 0
#define MP_ERR_NULL (-1)        /* required pointer is NULL */
#define MP_ERR_SHAPE (-2)       /* non-positive / inconsistent dimension */
#define MP_ERR_UNSUPPORTED (-3) /* valid request outside what the kernels implement */
#define MP_ERR_HIP (-4)         /* HIP runtime error at launch (see mp_last_hip_error) */
#define MP_ERR_WORKSPACE (-5)   /* workspace missing or too small */

const char* mp_version(void);
const char* mp_error_string(int code);
int mp_last_hip_error(void); /* hipError_t of the most recent MP_ERR_HIP on this thread */

/* ------------------------------------------------------------------------------------------
 * Decoder: TopDownHeatMapDecoder.construct, mindpose/models/decoders/top_down_decoder.py:72-94
 *   _get_max_preds :96-116 (per-joint arg-max, first index on ties, no maxval>0 mask)
 *   _shift_coordinate :118-141 | _dark_udp_refine_coords :171-205 | _transform_preds :143-169
 * heatmap [N,K,H,W]; center,scale [N,2]; score [N] -> preds [N,K,3]=(x,y,maxval), boxes [N,6].
 * argmax_idx (optional, may be NULL): [N,K] int32 flat arg-max index (bit-exact target).
 * blur_kernel: dev [kernel_size^2] normalised Gaussian (:207-215), required for MP_REFINE_DARK.
 * ------------------------------------------------------------------------------------------ */
#define MP_REFINE_NONE 0
#define MP_REFINE_SHIFT 1 /* shift_coordinate=True */
#define MP_REFINE_DARK 2  /* dark_udp_refine=True  */

int mp_decode_topdown(const float* heatmap_dev, const float* center_dev, const float* scale_dev,
                      const float* score_dev, float* preds_dev, float* boxes_dev, int32_t* argmax_idx_dev,
                      int n, int k, int h, int w, int refine_mode, int use_udp, int to_original,
                      float pixel_std, const float* blur_kernel_dev, int kernel_size, mp_stream_t stream);

/* mp_decode_topdown in MP_REFINE_DARK mode that ALSO writes the intermediates of the refinement (top_down_decoder.py:176-204)
 * for parity tests: dark_terms_dev [N*K][16] = the 3x3 neighbourhood of log(clip(blur(heatmap))) around the arg-max, row-major
 * (rows y-1, y, y+1; zero outside the map = the reference's zero pad in log space) [0..8], dx, dy [9,10], dxx, dyy, dxy [11..13],
 * det(Hessian + 1e-7 I) [14], 0 [15].  Same kernel, same arithmetic; the product path passes no such pointer. */
int mp_decode_topdown_debug(const float* heatmap_dev, const float* center_dev, const float* scale_dev,
                            const float* score_dev, float* preds_dev, float* boxes_dev, int32_t* argmax_idx_dev,
                            int n, int k, int h, int w, int refine_mode, int use_udp, int to_original,
                            float pixel_std, const float* blur_kernel_dev, int kernel_size, float* dark_terms_dev,
                            mp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Flip-test aggregation: _MultiRunNet.construct, mindpose/engine/inferencer/topdown_inferencer.py:165-187
 *   avg = (heatmap + flip_back(flipped)[shifted]) * 0.5 ; decoder(avg, ...)
 * flip_index [K] int32 (:78-80).  avg_out (optional, may be NULL): [N,K,H,W] averaged heat-map.
 * mp_flip_aggregate_decode fuses aggregation and decode in one pass (avg never leaves registers
 * unless avg_out is given).
 * ------------------------------------------------------------------------------------------ */
int mp_flip_aggregate(const float* heatmap_dev, const float* flipped_dev, const int32_t* flip_index_dev,
                      float* avg_out_dev, int n, int k, int h, int w, int shift_heatmap, mp_stream_t stream);

int mp_flip_aggregate_decode(const float* heatmap_dev, const float* flipped_dev, const int32_t* flip_index_dev,
                             int shift_heatmap, float* avg_out_dev, const float* center_dev,
                             const float* scale_dev, const float* score_dev, float* preds_dev, float* boxes_dev,
                             int32_t* argmax_idx_dev, int n, int k, int h, int w, int refine_mode, int use_udp,
                             int to_original, float pixel_std, const float* blur_kernel_dev, int kernel_size,
                             mp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Target generation: TopDownGenerateTarget._encoding / _udp_encoding,
 * mindpose/data/transform/topdown_transform.py:324-375, :377-430 (batched over samples).
 * keypoints [N,K,3] (x,y,vis) in input-image px -> target [N,K,H,W], target_weight [N,K].
 * feat_stride_x/y: the reference's float64 feature stride (image/heatmap, or (image-1)/(heatmap-1)
 * for UDP), computed by the host mirror exactly as the reference does.
 * patch_dev: plain mode only - the precomputed un-normalised Gaussian patch [patch_side^2] fp32
 * (:335-344), built on the host with the reference's numpy expression so values are bit-identical.
 * joint_weights_dev: optional [K] float64 (use_different_joint_weights), else NULL.
 * ------------------------------------------------------------------------------------------ */
int mp_gaussian_target(const float* keypoints_dev, const float* patch_dev, int patch_side,
                       const double* joint_weights_dev, float* target_dev, float* target_weight_dev, int n,
                       int k, int h, int w, double feat_stride_x, double feat_stride_y, double sigma,
                       int use_udp, mp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Loss: JointsMSELoss.construct, mindpose/models/loss/mse.py:36-44
 *   L = mean_{n,k,h,w}( w[n,k] * (pred-target)^2 ) ; weight_dev NULL -> use_target_weight=False.
 * Deterministic two-stage fp32/fp64 reduction; workspace >= mp_joints_mse_workspace_bytes(n,k).
 * bwd: grad_pred = grad_out * 2 * w * (pred-target) / (N*K*H*W); grad_out_dev NULL means 1.0.
 * 16-byte accesses when HW % 4 == 0 and every base the launch touches is 16-byte aligned, 4-byte ones otherwise (joints_loss.hip).
 * ------------------------------------------------------------------------------------------ */
size_t mp_joints_mse_workspace_bytes(int n, int k);
int mp_joints_mse_fwd(const float* pred_dev, const float* target_dev, const float* weight_dev, float* loss_dev,
                      void* workspace_dev, size_t workspace_bytes, int n, int k, int hw, mp_stream_t stream);
int mp_joints_mse_bwd(const float* pred_dev, const float* target_dev, const float* weight_dev,
                      const float* grad_out_dev, float* grad_pred_dev, int n, int k, int hw, mp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Loss: joint MSE with online hard keypoint mining (joints_loss.hip); the reference has no counterpart.
 * pred, target: contiguous fp32 [N][K][HW]; weight_dev [N][K] or NULL (= 1); 1 <= topk <= K <= 1024.
 *   S[n,k]   = sum_i ((pred_i - target_i)^2 * w[n,k]), fp32, the arithmetic of mp_joints_mse_fwd's row pass: a function of the
 *              row's values and weight only (bit-identical rows give bit-identical sums).
 *   sel[n,k] = 1 for the topk joints of sample n that come first in this total order, else 0: a NaN sum before every number,
 *              then the larger sum, then (equal sums, -0 == +0, or two NaNs) the lower joint index.  ONE BYTE per (n, k).
 *   L        = (float)(sum_n sum_{k selected, ascending} (double)S[n,k] / ((double)N * topk * HW)), sums in fp64 in a fixed
 *              order; no atomics, bit-reproducible.  topk == K is the value of mp_joints_mse_fwd (up to the order of the sums).
 *   bwd: grad_pred[n,k,i] = grad_out * sel[n,k] * w[n,k] * 2 (pred_i - target_i) / (N * topk * HW); grad_out_dev NULL means 1.0.
 *        A row with sel == 0 is written as zeros and its pred / target are NOT read.
 * fwd writes loss_dev [1], row_sum_dev [N*K] fp32 and sel_dev [N*K] bytes in three launches (rows; a workgroup per sample;
 * one workgroup), bwd is one launch; all on `stream`, no synchronisation, capturable.  16-byte accesses when HW % 4 == 0 and
 * the bases are 16-byte aligned, 4-byte ones otherwise.  workspace: mp_joints_ohkm_workspace_bytes(n, k) bytes (N doubles,
 * 8-byte aligned).
 * Before any launch: NULL (weight_dev and grad_out_dev excepted) -> MP_ERR_NULL; n, k or hw <= 0, topk < 1, topk > k, k > 1024
 * or n * k of 2^31 or more -> MP_ERR_SHAPE; a missing, short or misaligned workspace -> MP_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------ */
size_t mp_joints_ohkm_workspace_bytes(int n, int k);
int mp_joints_ohkm_fwd(const float* pred_dev, const float* target_dev, const float* weight_dev, float* loss_dev, float* row_sum_dev,
                       unsigned char* sel_dev, void* workspace_dev, size_t workspace_bytes, int n, int k, int hw, int topk,
                       mp_stream_t stream);
int mp_joints_ohkm_bwd(const float* pred_dev, const float* target_dev, const float* weight_dev, const unsigned char* sel_dev,
                       const float* grad_out_dev, float* grad_pred_dev, int n, int k, int hw, int topk, mp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Convolution family (direct, im2col-free, LDS-tiled, fp32 MFMA v_mfma_f32_16x16x4_f32):
 *   nn.Conv2d + nn.BatchNorm2d(eval) + residual add + nn.ReLU of
 *     BasicBlock  mindpose/models/backbones/hrnet.py:66-83, Bottleneck :126-146,
 *     HRModule fuse rows :318-344 (incl. ResizeNearestNeighbor + add :333-336),
 *     transitions :440-496, stem :568-573, HRNetHead heads/hrnet_head.py:47-49,
 *     ResNet stem/blocks backbones/resnet.py:118-138,:247-264,
 *     SimpleBaselineHead heads/simple_baseline_head.py:80-90 (Conv2dTranspose k4 s2 p1 as four
 *     2x2 sub-pixel phase convolutions) and its final 1x1 conv :57-62.
 *
 * out[n,co,oy,ox] = act( conv(x,w)[n,co,y,x] * scale[co] + shift[co] (+ res1[...]) (+ res2[...]) )
 * with (oy,ox) = (y*out_mul + out_off_y + a, x*out_mul + out_off_x + b), a,b in [0,out_rep):
 *   normal conv          out_mul=1 out_rep=1
 *   nearest-upsample+add out_mul=s out_rep=s   (HRModule fuse, j>i)
 *   deconv phase (py,px) out_mul=2 out_rep=1 out_off=(py,px)
 * res1/res2 (optional) are indexed like `out` ([N,Cout,out_h,out_w]); res1 may alias out.
 * Weights are pre-packed once by mp_conv_pack_weight (device -> device).
 * ------------------------------------------------------------------------------------------ */
typedef struct mp_conv_desc {
    int32_t n, cin, h, w;          /* input [N,Cin,H,W] */
    int32_t cout, kh, kw;          /* kernel (kh == kw in {1,2,3,7}) */
    int32_t stride;                /* 1 or 2 */
    int32_t pad_top, pad_left;     /* zero padding before the first row / column */
    int32_t conv_h, conv_w;        /* conv output extent (before the output mapping) */
    int32_t out_h, out_w;          /* extent of the out / res tensors */
    int32_t out_mul, out_rep, out_off_y, out_off_x;
    int32_t relu;                  /* apply ReLU last */
    int32_t flags;                 /* MP_CONV_* bits; an unknown bit is refused (MP_ERR_UNSUPPORTED) */
} mp_conv_desc;

/* mp_conv_desc.flags: the launch will share the CUs with other kernels of the caller - a training step's BatchNorm and
 * weight-gradient launches on sibling streams.  Forms that take a CU's whole register file (the two-team Winograd
 * workgroup) are then not chosen: they are faster alone and slower in that company. */
#define MP_CONV_SHARES_CUS 1
/* fp16 family only (mp_f16_conv2d_fwd): the FOUR 2x2 sub-pixel phase convs of a stride-2 3x3 data gradient as ONE launch.  The
 * descriptor is one phase's (kh = kw = 2, stride 1, out_mul 2, out_off_* = 0; all four phases share its padding - the tap
 * alignment is in the packing, mp_f16_pack_weight mode 3); phase (py, px) writes output pixels (2 y + py, 2 x + px) and reads its
 * weights from slice 2 py + px of the packed buffer (four slices of mp_f16_packed_weight_bytes(cout, cin, 2, 2) bytes each).
 * One-tile and persistent multi-tile variants only; no residual; statistics: the backward sums (mp_f16_conv2d_fwd_stats mode 2,
 * partial slots = four times a phase's).  The same sums from four launches: mp_f16_conv2d_fwd_stats mode 2 also accepts ONE phase
 * on its own (no flag; 2x2 taps, out_mul 2, the phase in out_off_y / out_off_x, one-tile / multi-tile variants): partials_dev is
 * then the buffer of the merged launch of the same variant (4 x mp_f16_conv_stats_parts of the one-phase desc) and the launch
 * fills slots [phase x parts, (phase + 1) x parts) of every channel block. */
#define MP_CONV_PHASES4 2

/* bytes of the packed weight buffer for a (cout, cin, kh, kw) kernel */
size_t mp_conv_packed_weight_bytes(int cout, int cin, int kh, int kw);
/* Weight source layouts (`transposed` selects how w_dev is read; cout/cin/kh/kw describe the PACKED convolution):
 *   0  w_dev = [Cout,Cin,kh,kw]   forward Conv2d
 *   1  w_dev = [Cin,Cout,4,4]     Conv2dTranspose(k4,s2,p1) sub-pixel phase (py,px), kh=kw=2
 *   2  w_dev = [Cin,Cout,kh,kw]   data gradient of a stride-1 Conv2d whose forward weight is w_dev (roles swapped,
 *                                 taps mirrored): dx = conv(dz, pack2(W)) with the same padding
 *   3  w_dev = [Cin,Cout,3,3]     data gradient of a 3x3 stride-2 pad-1 Conv2d, output parity phase (py,px), kh=kw=2,
 *                                 run with pad 0 and the deconv output mapping (out_mul=2, out_off=(py,px))
 *   5 / 6  (kh=kw=3)              the Winograd forms U = G w G^T of mode 0 / mode 2, for mp_conv2d_winograd_fwd; packed_dev holds
 *                                 mp_conv_winograd_packed_weight_bytes (also as jobs of mp_conv_pack_weight_batch: units_j =
 *                                 Cin_pad4 * Cout_pad16, a thread writes the 16 values of one (cin, cout) pair) */
int mp_conv_pack_weight(const float* w_dev, float* packed_dev, int cout, int cin, int kh, int kw,
                        int transposed, int phase_y, int phase_x, mp_stream_t stream);
int mp_conv2d_fwd(const mp_conv_desc* desc, const float* x_dev, const float* packed_w_dev,
                  const float* scale_dev, const float* shift_dev, const float* res1_dev, const float* res2_dev,
                  float* out_dev, mp_stream_t stream);

/* Same as mp_conv2d_fwd / mp_plan_add_conv with the tile variant forced (0..7 = cout tile x pixel tile builds of the direct
 * kernel; 8 = the streaming 1x1 kernel for the HBM-bound stage-1 / layer1 layers - Cin 64 / 128 / 256 with Cin * Cout <= 16384,
 * image planes a multiple of 64 pixels, one residual tensor, same packed weights; 10 = the blocked-GEMM kernel for 1x1 stride 1 / 2
 * and the 2x2 stride-1 sub-pixel phases of the transposed convolution - Cin a multiple of 16, Cout >= 96, planes a multiple of 4
 * pixels, one residual tensor, same packed weights; 11 = the K-split kernel for SMALL problems - 3x3 pad 1 stride 1 / 2 and 1x1 stride 1 (a handful of
 * crops: 16 couts x 16 pixels per workgroup, its eight waves split the k loop - csrc/conv_small_f32.hip; at most 1024 workgroups,
 * up to two residual tensors, same packed weights), 12 = the same kernel with 48 / 64 pixels per workgroup (a few dozen crops; at
 * most 2048 workgroups; bit-identical to 11); 9 is the host tuner's index of the Winograd form, which has its own entry
 * points below; -1 = library heuristic).  Returns MP_ERR_UNSUPPORTED when that variant cannot run the shape.  Used by the host-side autotuner, which times the candidates once per distinct layer shape. */
int mp_conv2d_fwd_variant(const mp_conv_desc* desc, int variant, const float* x_dev, const float* packed_w_dev,
                          const float* scale_dev, const float* shift_dev, const float* res1_dev, const float* res2_dev,
                          float* out_dev, mp_stream_t stream);

/* The 3x3 stride-1 padding-1 convolutions of the branches (hrnet.py:51-64 BasicBlock, 202-241 _make_one_branch) in Winograd
 * F(2x2,3x3) form, all fp32: 16 instead of 36 multiplications per 2x2 output tile and (cin, cout) pair; same operands, epilogue
 * (folded BatchNorm scale/shift, res1, res2, ReLU) and result as mp_conv2d_fwd up to fp32 rounding (the sums are associated
 * differently).  Needs even H and W <= 96 (W % 4 != 0: whole images of at most 24 tiles with H*W % 4 == 0), Cin % 8 == 0 and the plain
 * output mapping; mp_conv_winograd_supported
 * returns MP_OK or MP_ERR_UNSUPPORTED for a descriptor.  The weights are transformed once: U = G w G^T,
 * [Cin_pad4][Cout_pad16][16] floats (mp_conv_winograd_packed_weight_bytes). */
size_t mp_conv_winograd_packed_weight_bytes(int cout, int cin);
int mp_conv_winograd_pack_weight(const float* w_dev, float* packed_dev, int cout, int cin, mp_stream_t stream);
int mp_conv_winograd_supported(const mp_conv_desc* desc);
int mp_conv2d_winograd_fwd(const mp_conv_desc* desc, const float* x_dev, const float* packed_u_dev, const float* scale_dev,
                           const float* shift_dev, const float* res1_dev, const float* res2_dev, float* out_dev,
                           mp_stream_t stream);

/* nn.MaxPool2d(kernel_size=3, stride=2, pad_mode="same"), resnet.py:190: pads bottom/right only. */
int mp_maxpool3x3s2_same(const float* x_dev, float* out_dev, int n, int c, int h, int w, mp_stream_t stream);

/* HRModule exchange unit, up-sampling side (mindpose/models/backbones/hrnet.py:327-339, j > i terms):
 *   out = act( ((base + up_s1(t1)) + up_s2(t2)) + up_s3(t3) )      (reference summation order)
 * base/out [N,C,H,W]; t_k [N,C,H/s_k,W/s_k] already holds BN(conv1x1(x_j)); up_s = nearest (src = dst / s).
 * t2/t3 may be NULL (s ignored).  One streaming pass: the up-sampled terms are never materialised and the
 * full-resolution sum is read and written once per fuse row.  out may alias base. */
int mp_fuse_upsample_sum(const float* base_dev, const float* t1_dev, int s1, const float* t2_dev, int s2,
                         const float* t3_dev, int s3, float* out_dev, int n, int c, int h, int w, int relu,
                         mp_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Launch plan: a recorded sequence of the calls above (one HRNet / ResNet forward = ~300 launches)
 * replayed by ONE native call, so the per-layer host cost is paid once at build time.
 * ------------------------------------------------------------------------------------------ */
typedef struct mp_plan mp_plan;
mp_plan* mp_plan_create(void);
void mp_plan_destroy(mp_plan* plan);
int mp_plan_add_conv(mp_plan* plan, const mp_conv_desc* desc, const float* x_dev, const float* packed_w_dev,
                     const float* scale_dev, const float* shift_dev, const float* res1_dev,
                     const float* res2_dev, float* out_dev);
int mp_plan_add_conv_variant(mp_plan* plan, const mp_conv_desc* desc, int variant, const float* x_dev,
                             const float* packed_w_dev, const float* scale_dev, const float* shift_dev,
                             const float* res1_dev, const float* res2_dev, float* out_dev);
/* mp_conv2d_winograd_fwd as a plan entry (same operands; MP_ERR_UNSUPPORTED when the descriptor is outside the Winograd form). */
/* Conv2dTranspose(k=4, s=2, pad_mode="pad", padding=1) + scale / shift (+ReLU) - simple_baseline_head.py:80-90 - with ALL FOUR
 * sub-pixel phases in one launch of the blocked-GEMM kernel (variant 10 above; phase = a grid dimension, so the small-map layers
 * of the head fill the chip with efficient tiles).  `phase00_desc` is the phase (0, 0) launch of the per-phase form: kh = kw = 2,
 * stride 1, pad_top = pad_left = 1, conv = input size, out = 2x input size, out_mul 2, offsets 0; `packed4_dev` = the four phase
 * packings of mp_conv_pack_weight(transposed = 1, phase_y, phase_x) back to back in the order (0,0) (0,1) (1,0) (1,1), each
 * mp_conv_packed_weight_bytes(cout, cin, 2, 2) long.  Same arithmetic per output as four mp_conv2d_fwd_variant(10) launches. */
int mp_deconv4x4s2_gemm_supported(const mp_conv_desc* phase00_desc);
int mp_deconv4x4s2_gemm_fwd(const mp_conv_desc* phase00_desc, const float* x_dev, const float* packed4_dev, const float* scale_dev,
                            const float* shift_dev, float* out_dev, mp_stream_t stream);
int mp_plan_add_deconv4x4s2_gemm(mp_plan* plan, const mp_conv_desc* phase00_desc, const float* x_dev, const float* packed4_dev,
                                 const float* scale_dev, const float* shift_dev, float* out_dev);
int mp_plan_add_conv_winograd(mp_plan* plan, const mp_conv_desc* desc, const float* x_dev, const float* packed_u_dev,
                              const float* scale_dev, const float* shift_dev, const float* res1_dev, const float* res2_dev,
                              float* out_dev);
int mp_plan_add_maxpool(mp_plan* plan, const float* x_dev, float* out_dev, int n, int c, int h, int w);
int mp_plan_add_fuse_sum(mp_plan* plan, const float* base_dev, const float* t1_dev, int s1, const float* t2_dev, int s2,
                         const float* t3_dev, int s3, float* out_dev, int n, int c, int h, int w, int relu);
/* Execution lanes: entries added after mp_plan_set_lane(plan, l) (l in 0..3) replay on lane l - lane 0 is the stream
 * passed to mp_plan_run, lanes 1..3 are side streams the plan owns - so independent sub-graphs (the HRNet branches, the
 * rows of an exchange unit) overlap on the chip.  mp_plan_add_barrier orders every lane after everything recorded so far
 * on every other lane; mp_plan_run forks the side lanes from the caller's stream and joins them before returning control
 * to it (event fork/join: also valid under stream capture).  mp_plan_run_range always replays sequentially on one stream. */
int mp_plan_set_lane(mp_plan* plan, int lane);
int mp_plan_add_barrier(mp_plan* plan);
int mp_plan_size(const mp_plan* plan);
int mp_plan_run(const mp_plan* plan, mp_stream_t stream);
/* run entries [first, first+count) only (profiling / per-layer timing) */
int mp_plan_run_range(const mp_plan* plan, int first, int count, mp_stream_t stream);
/* launch geometry of entry `index` (roofline report): info[0]=kind (0 conv, 1 maxpool, 2 fuse-sum), [1]=kernel size,
 * [2]=stride, [3]=tile variant, [4]=workgroups, [5]=LDS bytes per workgroup, [6]=cout tile, [7]=pixel tile,
 * [8]=cin chunk, [9]=images per tile, [10]=rows per tile, [11]=light variant (3 workgroups/CU) */
int mp_plan_entry_info(const mp_plan* plan, int index, int64_t info[12]);

/* ------------------------------------------------------------------------------------------
 * Training-side kernels (reference: mindspore.Model.train over NetWithLoss, tools/train.py:170-233, amp aside:
 * everything here computes in fp32).  All reductions are deterministic (fixed partition, fixed combine order).
 *
 * BatchNorm2d in training mode (nn.BatchNorm2d cells of hrnet.py / resnet.py; eps 1e-5, momentum 0.9 meaning
 * moving = 0.9*moving + 0.1*batch [MS-knowledge]):
 *   fwd: per-channel batch mean / biased variance over (N,H,W) of z [N,C,HW];
 *        y = act(gamma*(z-mean)*invstd + beta (+ res)); saves mean/invstd; updates the moving statistics when given
 *        (moving variance takes the unbiased batch variance).
 *   bwd: g = dy masked by (y > 0) when relu; dgamma = sum g*xhat; dbeta = sum g;
 *        dz = gamma*invstd*(g - dbeta/M - xhat*dgamma/M); dres (optional) = g.
 * workspace >= mp_bn_workspace_bytes(c).
 * ------------------------------------------------------------------------------------------ */
size_t mp_bn_workspace_bytes(int c);
int mp_bn_train_fwd(const float* z_dev, const float* gamma_dev, const float* beta_dev, const float* res_dev, float* y_dev,
                    float* save_mean_dev, float* save_invstd_dev, float* moving_mean_dev, float* moving_var_dev, int n,
                    int c, int hw, float eps, float momentum, int relu, void* workspace_dev, size_t workspace_bytes,
                    mp_stream_t stream);
int mp_bn_train_bwd(const float* dy_dev, const float* z_dev, const float* y_dev, const float* gamma_dev,
                    const float* save_mean_dev, const float* save_invstd_dev, float* dz_dev, float* dres_dev,
                    float* dgamma_dev, float* dbeta_dev, int n, int c, int hw, int relu, void* workspace_dev,
                    size_t workspace_bytes, mp_stream_t stream);

/* backward of mp_fuse_upsample_sum: g = dy*(out>0 when relu); dbase = g; dt_k = s_k x s_k block sums of g.
 * Any of dbase / dt_k may be NULL (not needed). */
int mp_fuse_upsample_sum_bwd(const float* dy_dev, const float* out_dev, float* dbase_dev, float* dt1_dev, int s1,
                             float* dt2_dev, int s2, float* dt3_dev, int s3, int n, int c, int h, int w, int relu,
                             mp_stream_t stream);

/* mp_bn_train_bwd that ALSO adds dgamma / dbeta into dgamma_acc / dbeta_acc (both or neither; the caller's gradient arena) */
int mp_bn_train_bwd_acc(const float* dy_dev, const float* z_dev, const float* y_dev, const float* gamma_dev,
                        const float* save_mean_dev, const float* save_invstd_dev, float* dz_dev, float* dres_dev,
                        float* dgamma_dev, float* dbeta_dev, float* dgamma_acc_dev, float* dbeta_acc_dev, int n, int c, int hw,
                        int relu, void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);

/* mindspore.nn.AdamWeightDecay (selected by mindpose/optim/optim_factory.py:69-72 for "adamw"): Adam WITHOUT bias
 * correction, eps added to sqrt(v), decoupled weight decay:  m=b1*m+(1-b1)*g; v=b2*v+(1-b2)*g*g;
 * p -= lr*(m/(sqrt(v)+eps) + wd*p).  Operates on one flat fp32 arena (params, grads, moments). */
int mp_adamw_step(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, size_t count,
                  float lr, float beta1, float beta2, float eps, float weight_decay, mp_stream_t stream);

/* mp_adamw_step with the gradient read as g * grad_scale (fold 1 / (loss_scale * world_size) here instead of a separate pass over
 * the arena) and an optional device flag: when *skip_flag_dev != 0 the launch leaves parameters and moments untouched (the
 * overflow step of DynamicLossScaleManager, tools/train.py:170-173). */
int mp_adamw_step_scaled(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, size_t count,
                         float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                         const int* skip_flag_dev, mp_stream_t stream);
/* Overflow check of the dynamic loss scale: *flag_dev |= 1 when any of grad_dev[0..count) is inf / nan (one read of the
 * arena; the caller zeroes the flag).  grad_dev must be 16-byte aligned. */
int mp_grad_finite_check(const float* grad_dev, size_t count, int* flag_dev, mp_stream_t stream);

/* ---- data-parallel gradient mean over RCCL/xGMI (tools/train.py:43-49: parallel_mode=data_parallel, gradients_mean=True) ----
 * A thin layer over the process's RCCL (bound at run time; mp_comm_available() == 0 when no RCCL can be found).
 *   mp_comm_get_unique_id  rank 0 fills 128 bytes (ncclUniqueId) that the host code broadcasts to the other ranks
 *   mp_comm_init_rank      every rank, after hipSetDevice: creates the communicator (collective call)
 *   mp_allreduce_grads     in-place all-reduce of count fp32 values on `stream` (average != 0: mean over ranks, ncclAvg);
 *                          asynchronous, capturable into a hipGraph like any RCCL call
 *   mp_reduce_scatter_allgather_grads   the same result as reduce-scatter + all-gather of count / nranks shards (count must be a
 *                          multiple of nranks): every xGMI link carries 1/nranks of the arena in each phase
 * Errors: MP_ERR_UNSUPPORTED (no RCCL), MP_ERR_HIP with the ncclResult_t in mp_comm_last_error(). */
int mp_comm_available(void);
int mp_comm_last_error(void);
int mp_comm_get_unique_id(void* id128_host);
int mp_comm_init_rank(void** comm_out, int nranks, const void* id128_host, int rank);
int mp_comm_destroy(void* comm);
/* ncclCommCount: the number of ranks the communicator itself reports (-1 on error) */
int mp_comm_count(void* comm);
int mp_allreduce_grads(void* comm, float* arena_dev, size_t count, int average, mp_stream_t stream);
int mp_reduce_scatter_allgather_grads(void* comm, float* arena_dev, size_t count, int nranks, int rank, int average,
                                      mp_stream_t stream);

/* The other optimizers registered by mindpose/optim/optim_factory.py:9-14, on the same flat fp32 arenas.
 * kind 1 = mindspore.nn.Adam (bias-corrected; hyper = {beta1, beta2, eps, beta1^t, beta2^t}; state1 = m, state2 = v),
 * 2 = nn.SGD (hyper = {momentum, dampening, nesterov, first_step}; state1 = momentum buffer, may be NULL when momentum == 0),
 * 3 = nn.Momentum (hyper = {momentum, use_nesterov}; state1 = accumulator), 4 = nn.Adagrad (state1 = accumulator, initialised
 * by the caller).  The gradient enters as g * grad_scale + weight_decay * p (static loss scale and L2 decay of those cells).
 * Update rules from the MindSpore documentation [MS-knowledge; no reference test pins them]. */
int mp_optimizer_step(int kind, float* param_dev, const float* grad_dev, float* state1_dev, float* state2_dev, size_t count,
                      float lr, float grad_scale, float weight_decay, const float hyper[5], mp_stream_t stream);

/* ---- device-resident step tail (step_end.hip): the host queues training steps without reading one back ---------------------
 * The loss-scale state machine of mindspore.amp.DynamicLossScaleManager (tools/train.py:170-181), the skip decision and the
 * learning-rate lookup run on the device; the update launches read their step-dependent arguments from device memory. */
typedef struct mp_train_tail_state {   /* device memory, owned by the caller */
    double loss_scale;
    int64_t cur_iter, last_overflow_iter, skipped_steps, applied_steps;
} mp_train_tail_state;
typedef struct mp_step_args {          /* device memory, written by mp_train_tail_advance, read by the *_resident launches */
    int32_t skip;                      /* 1: this step overflowed, the update launches leave everything untouched */
    float grad_scale;                  /* (float)(mean_scale / loss_scale before the update / static_loss_scale) */
    float lr;                          /* lr_table[min(applied_steps, lr_len - 1)] */
    float aux0, aux1;                  /* aux_table[min(applied_steps, aux_len - 1)][0..1] (Adam: beta1^t, beta2^t), 0 without a table */
    float first_step;                  /* applied_steps == 0 */
} mp_step_args;
/* One launch of one workgroup.  overflow_flag_dev: the flag mp_grad_finite_check filled; NULL = no loss scaling, never overflow
 * (loss_scale is then neither read into a decision nor changed).  Fills *step_args_dev from the state BEFORE the update, then
 * advances the state as DynamicLossScaleManager.update_loss_scale does, in double: on overflow loss_scale = max(loss_scale /
 * scale_factor, 1), last_overflow_iter = cur_iter, ++skipped_steps; otherwise loss_scale *= scale_factor when (cur_iter -
 * last_overflow_iter) % scale_window == 0, ++applied_steps; always ++cur_iter.  Finally *loss_scale_out_dev (may be NULL) =
 * (float)loss_scale: the scalar a captured step multiplies its loss by.  lr_table_dev: lr_len >= 1 fp32 values; aux_table_dev
 * (may be NULL): aux_len pairs. */
int mp_train_tail_advance(const int* overflow_flag_dev, mp_train_tail_state* state_dev, double scale_factor, int64_t scale_window,
                          double mean_scale, double static_loss_scale, const float* lr_table_dev, int64_t lr_len,
                          const float* aux_table_dev, int64_t aux_len, mp_step_args* step_args_dev, float* loss_scale_out_dev,
                          mp_stream_t stream);
/* mp_adamw_step_scaled / mp_optimizer_step with lr, grad_scale and skip - and, kind 1, hyper[3..4] = aux0, aux1; kind 2, hyper[3]
 * = first_step - read from *step_args_dev instead of the launch's arguments: the same per-element arithmetic, operation for
 * operation.  A set skip leaves parameters and states untouched. */
int mp_adamw_step_resident(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev, size_t count,
                           float beta1, float beta2, float eps, float weight_decay, const mp_step_args* step_args_dev,
                           mp_stream_t stream);
int mp_optimizer_step_resident(int kind, float* param_dev, const float* grad_dev, float* state1_dev, float* state2_dev, size_t count,
                               float weight_decay, const float hyper[5], const mp_step_args* step_args_dev, mp_stream_t stream);

/* ---- gradient clipping by global norm, decided on the device (step_end.hip) ----------------------------------------------------
 * mindspore.ops.clip_by_global_norm restated on the gradient arena; the reference trains without it.  The arena A holds the
 * gradient sums over ranks, still multiplied by the loss scale.  With base = mean_scale / loss_scale / static_loss_scale (double,
 * the expression of mp_step_args.grad_scale) and S = sum over the arena of (double)A[i] * (double)A[i]:
 *   norm = sqrt(S) * base;   coef = clip_norm / norm when norm is finite and norm > clip_norm, else exactly 1.0;
 *   grad_scale = (float)(base * coef)          - the coefficient multiplies last, one rounding to fp32.
 * No epsilon: an unclipped step is bit-equal to the step without clipping.  clip_norm = +inf measures only.  No pass scales the
 * gradients: the update launches already multiply every gradient by grad_scale while reading it. */
typedef struct mp_grad_clip_state {    /* device memory, owned by the caller, zeroed by the caller to start a period */
    double last_norm;                  /* norm of the last step that was not skipped */
    double norm_sum;                   /* running sum of those norms: the mean is norm_sum / measured_steps */
    double norm_max;                   /* their maximum (a NaN norm never becomes it) */
    int64_t measured_steps;            /* steps that were not skipped */
    int64_t clipped_steps;             /* of those, steps with norm > clip_norm */
} mp_grad_clip_state;
typedef struct mp_grad_clip_resolved { /* device memory, written by mp_grad_clip_resolve, downloaded by a host-driven step */
    int32_t flag, pad;                 /* the overflow flag as the launch saw it (0 when it was given none) */
    double norm, coef;                 /* as defined above; garbage-in norm and coef = 1.0 on an overflow step */
} mp_grad_clip_resolved;
/* Number of fp64 partial sums mp_grad_finite_norm writes for `count` values: the number of its workgroups, a function of count
 * alone - ceil(count / 4 / 1024), one per 1024 quads, at least 1, at most 2048; 0 for count == 0. */
int mp_grad_norm_partials(size_t count);
/* mp_grad_finite_check and the sum of squares in ONE read of the arena.  The flag semantics are those of mp_grad_finite_check
 * (*flag_dev |= 1 on any inf / nan, the caller zeroes it; grad_dev 16-byte aligned); partials_dev[b] = the sum of (double)x * x over
 * the values workgroup b read, for b < mp_grad_norm_partials of count (plain stores, every entry written by every launch;
 * 8-byte aligned).  Bit-reproducible and independent of occupancy: the grid depends on count alone; a trip of a workgroup is one
 * contiguous run of 1024 quads, thread t reading quads t, t + 256, t + 512, t + 768 of it, trips a grid stride apart, then a last
 * partial run and (workgroup 0) the scalar tail; a thread adds its values in index order into one fp64 accumulator (products of two
 * fp32 values are exact in fp64: only the additions round, and no finite fp32 value overflows the sum - so the flag is "the sum is
 * not finite"), a wave adds its lanes by shuffles down by 32, 16, 8, 4, 2, 1, thread 0 adds the four wave sums in wave order.  No
 * floating-point atomics. */
int mp_grad_finite_norm(const float* grad_dev, size_t count, int* flag_dev, double* partials_dev, mp_stream_t stream);
/* mp_train_tail_advance with clipping: one launch of one workgroup, the same arguments, and partials_dev[0..n_partials) of
 * mp_grad_finite_norm (n_partials <= 2048), clip_norm (positive or +inf) and *clip_state_dev.  Lane l of the 64 adds partials l,
 * l + 64, ... in index order, the lanes are added by shuffles down by 32 ... 1: that is S.  grad_scale of the step-arguments block
 * is (float)(base * coef); everything else of the block and of mp_train_tail_state is what mp_train_tail_advance makes it.  On a
 * step that is not skipped the clip state advances: last_norm = norm, norm_sum += norm, norm_max = max, ++measured_steps,
 * ++clipped_steps when norm > clip_norm; an overflow step leaves it untouched (its norm is garbage).  Without a flag
 * (overflow_flag_dev NULL) a non-finite norm gives coef = 1 and is recorded as it is. */
int mp_train_tail_advance_clip(const int* overflow_flag_dev, mp_train_tail_state* state_dev, double scale_factor, int64_t scale_window,
                               double mean_scale, double static_loss_scale, const float* lr_table_dev, int64_t lr_len,
                               const float* aux_table_dev, int64_t aux_len, mp_step_args* step_args_dev, float* loss_scale_out_dev,
                               const double* partials_dev, int n_partials, double clip_norm, mp_grad_clip_state* clip_state_dev,
                               mp_stream_t stream);
/* The host-driven step's form of the same decision: one launch of one workgroup runs the same device code for S, norm and coef
 * with loss_scale given by the host (1.0 without a manager), writes *resolved_dev and advances *clip_state_dev as above.  The host
 * downloads the block where it would download the flag - one read-back per step - and multiplies coef in last. */
int mp_grad_clip_resolve(const int* overflow_flag_dev, const double* partials_dev, int n_partials, double mean_scale, double loss_scale,
                         double static_loss_scale, double clip_norm, mp_grad_clip_state* clip_state_dev,
                         mp_grad_clip_resolved* resolved_dev, mp_stream_t stream);

/* ---- training-time pose accuracy (pose_metric.hip): PCK of the output heat maps against the target heat maps ------------------
 * The accuracy() of the HRNet training code (lib/core/evaluate.py), restated; the reference has no counterpart.  output_dev and
 * target_dev: contiguous fp32 [N][K][H][W].  Per map the first (row-major) index of the maximum gives (x, y) = (idx % W, idx / W),
 * or (0, 0) when the maximum is not > 0 or the map holds a NaN; +inf is an ordinary maximum.  A pair (n, k) is valid iff the
 * target's x > 1 and y > 1; with dx, dy the integer differences output - target, a valid pair is a hit iff
 * 100.0 * ((dx W)^2 + (dy H)^2) < thr * thr * (H W)^2, both sides in double in this order, strictly.  Per call acc_k =
 * hits_k / valid_k over the joints with valid_k > 0, cnt = their number, avg_acc = their sum in joint order / cnt (0 without any).
 * Two launches: one workgroup per map pair (at most 4096 workgroups, further pairs by a grid-stride loop) writes flags_dev[n * K + k]
 * = valid | hit << 1; a single workgroup sums them per joint and advances *state_dev.  No atomics, no allocation, no
 * synchronisation; capturable.  The state block is 48 + 16 K bytes of device memory owned by the caller, 8-byte aligned, zeroed by
 * the caller to start an epoch: this header, then int64 hits[K], then int64 valid[K] (summed over the calls).
 * Before any HIP call: NULL -> MP_ERR_NULL; a non-positive extent, N * K of 2^31 or more, thr not positive and finite ->
 * MP_ERR_SHAPE; H or W above 4096 (the hit test's squares would no longer be exact in double), a map pointer off 4-byte
 * or a state pointer off 8-byte alignment -> MP_ERR_UNSUPPORTED. */
typedef struct mp_pose_pck_state {
    int64_t steps;        /* calls accumulated */
    int64_t sum_cnt;      /* running sum of cnt */
    double sum_acc_cnt;   /* running sum of avg_acc * cnt: the epoch's accuracy is sum_acc_cnt / sum_cnt */
    double last_avg_acc;  /* the last call's avg_acc */
    int64_t last_cnt;     /* the last call's cnt */
    int64_t pad;
} mp_pose_pck_state;
int mp_pose_pck_accuracy(const float* output_dev, const float* target_dev, int N, int K, int H, int W, double thr,
                         unsigned char* flags_dev, void* state_dev, mp_stream_t stream);

/* Conv2d weight gradient (training backward of every conv of hrnet.py): dW[co,ci,ky,kx] = sum_{n,y,x}
 * dz[n,co,y,x] * x[n,ci,y*s+ky-p,x*s+kx-p] for k in {1,3}, s in {1,2}, p = k/2 (desc as for the forward conv; its
 * output-mapping fields are ignored).  fp32 MFMA, pixel axis split over workgroups into slabs that are summed in a
 * fixed order (deterministic).  accumulate != 0 adds into dw.  workspace >= mp_conv_wgrad_workspace_bytes(desc). */
size_t mp_conv_wgrad_workspace_bytes(const mp_conv_desc* desc);
int mp_conv_wgrad(const mp_conv_desc* desc, const float* x_dev, const float* dz_dev, float* dw_dev, int accumulate,
                  void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);

/* ---- fp16 matrix-core inference path (amp level O2 / O3; BASELINE.json configs[4] "fp16 MFMA") -----------------------
 * Replaces what mindspore.amp.auto_mixed_precision(network, "O2") does to the cells of mindpose/models/backbones/hrnet.py
 * when they run on the Ascend cube unit: fp16 conv operands, fp32 accumulation, BatchNorm in fp32, fp16 activations.
 * Activations are CHANNEL-BLOCKED fp16, [N][ceil(C/8)][H][W][8] ("c8"; padding channels zero), weights are packed
 * [ceil(Cin/32)][kh*kw][4][Cout_pad16][8] fp16; scale / shift are fp32 arrays of Cout_pad16 entries (zero beyond Cout).
 * Kernel 1x1, 2x2 (stride 1) or 3x3; output mapping plain or strided scatter (out_mul, out_off_*: the sub-pixel phases of
 * the transposed convolution), out_rep must be 1: the exchange-unit up-sampling runs in mp_f16_fuse_upsample_sum.  variant -1 = heuristic, 0..9 = forced tile shape
 * (5..9 = the light builds of 0..4: small chunks, three workgroups per CU), 10..19 = the persistent multi-tile kernel in
 * those shapes (two / one workgroup per CU), 20..23 = the 16-cout x 192-pixel shape (regular, light, multi-tile x2),
 * 24 = 32 couts x 384 pixels for layers whose K fits one chunk (Cin <= 32 at 3x3). */
size_t mp_f16_packed_weight_bytes(int cout, int cin, int kh, int kw);
size_t mp_f16_activation_bytes(int n, int c, int h, int w);
/* transposed = 0: Conv2d weight [Cout,Cin,kh,kw]; 1: the (phase_y, phase_x) 2x2 sub-pixel phase of a
 * Conv2dTranspose(k=4, s=2, pad=1) weight [Cin,Cout,4,4] (kh = kw = 2); 2 / 3: the data-gradient packings of
 * mp_conv_pack_weight (stride-1 conv: roles swapped + taps mirrored; 3x3 stride-2 conv: 2x2 parity phases); 4: the data
 * gradient of transposed-conv phase (phase_y, phase_x) (w = the [Cin_t,Cout_t,4,4] weight, cout := Cin_t, cin := Cout_t) */
int mp_f16_pack_weight(const float* w_dev, void* packed_dev, int cout, int cin, int kh, int kw, int transposed, int phase_y,
                       int phase_x, mp_stream_t stream);
/* All weight packings of one training step in ONE launch (the fp32 master weights change every step, and an HRNet-W32 step
 * needs 700 packings: forward + data-gradient forms).  jobs_dev: device array of n_jobs descriptors with the arguments of
 * mp_f16_pack_weight (same validity rules, checked by the caller); first_block_dev: device array of n_jobs + 1 prefix sums of
 * ceil(units_j / 256), units_j = ceil(cin/32) * 4 * Cout_pad16 (one thread per (8 input channels, cout) pair: it walks the kh * kw
 * taps; a table with MORE blocks per job - e.g. the units of round 4, x kh * kw - is accepted: the surplus blocks leave at once);
 * total_blocks = its last entry.  Both tables are caller-owned and must stay alive until the launch has run. */
typedef struct mp_f16_pack_job {
    const float* w;
    void* packed;
    int cout, cin, kh, kw, transposed, phase_y, phase_x, reserved;
} mp_f16_pack_job;
int mp_f16_pack_weight_batch(const mp_f16_pack_job* jobs_dev, const unsigned* first_block_dev, int n_jobs, unsigned total_blocks,
                             mp_stream_t stream);
/* the fp32 form (mp_conv_pack_weight per job; packed = fp32 [Cin_pad4/4][kh*kw][4][Cout_pad16]): same job descriptor,
 * units_j = Cin_pad4 * kh * kw * Cout_pad16 / 4 (a thread writes four output channels) */
int mp_conv_pack_weight_batch(const mp_f16_pack_job* jobs_dev, const unsigned* first_block_dev, int n_jobs, unsigned total_blocks,
                              mp_stream_t stream);
int mp_f16_to_c8(const float* x_nchw_dev, void* out_c8_dev, int n, int c, int h, int w, mp_stream_t stream);
int mp_f16_from_c8(const void* x_c8_dev, float* out_nchw_dev, int n, int c, int h, int w, mp_stream_t stream);
int mp_f16_conv2d_fwd(const mp_conv_desc* desc, int variant, const void* x_c8_dev, const void* packed_w_dev,
                      const float* scale_dev, const float* shift_dev, const void* res1_c8_dev, const void* res2_c8_dev,
                      void* out_c8_dev, mp_stream_t stream);
/* Fused BasicBlock of the 32-channel and (round 4) the 64-channel HRNet branch (hrnet.py:30-83, 202-241, eval mode; SURVEY 8(b)
 * "mp_basicblock_fused"):
 *   out = relu(bn2(conv3x3(relu(bn1(conv3x3(x))))) + x),  x / out channel-blocked fp16 [n][c/8][h][w][8] (24 < c <= 32, or c == 64),
 * distinct buffers; packed_w1 / packed_w2 = mp_f16_pack_weight(mode 0) of the two [c,c,3,3] weights, scale / shift = folded
 * BatchNorm (c rounded up to 16 fp32 entries each, zero beyond c).  The intermediate tensor stays in LDS; the result is bit-identical
 * to two mp_f16_conv2d_fwd calls.  rows = output rows per workgroup (0 = the largest that fits).  MP_ERR_UNSUPPORTED for other
 * widths / maps too wide for a band; mp_f16_basicblock_supported answers that question without launching (1 / 0). */
int mp_f16_basicblock_supported(int n, int c, int h, int w);
int mp_f16_basicblock_fwd(const void* x_c8_dev, const void* packed_w1_dev, const float* scale1_dev, const float* shift1_dev,
                          const void* packed_w2_dev, const float* scale2_dev, const float* shift2_dev, void* out_c8_dev, int n,
                          int c, int h, int w, int rows, mp_stream_t stream);
/* First convolution of the network in fp32 (hrnet.py:377-385: 3x3, stride 2, padding 1, 3 -> 64 channels, folded BatchNorm, ReLU) as a
 * streaming kernel: out[n][64][h/2][w/2] = act(conv(x; weight) * scale + shift), x fp32 NCHW [n][3][h][w], weight = the [64][3][3][3]
 * tensor itself (no packing).  Same arithmetic as mp_conv2d_fwd on this layer with the 27 products summed in (tap, channel) order.
 * h even, w a multiple of 32: MP_ERR_UNSUPPORTED otherwise. */
int mp_stem_conv_fwd(const float* x_dev, const float* weight_dev, const float* scale_dev, const float* shift_dev, int relu, float* out_dev,
                     int n, int h, int w, mp_stream_t stream);
int mp_plan_add_stem_conv(mp_plan* plan, const float* x_dev, const float* weight_dev, const float* scale_dev, const float* shift_dev,
                          int relu, float* out_dev, int n, int h, int w);
/* First convolution of the network under amp O2, straight from the fp32 NCHW image (hrnet.py:377-385: 3x3, stride 2, padding 1,
 * 3 -> 64 channels, folded BatchNorm, ReLU): out = act(conv(fp16(x); fp16(weight)) * scale + shift), channel-blocked fp16
 * [n][8][h/2][w/2][8].  weight = the fp32 tensor [64][3][3][3] itself (no packing).  Replaces mp_f16_to_c8 + mp_f16_conv2d_fwd: same
 * fp16 operands and fp32 accumulation, the 27 products per output summed in ONE k-step (tap-major) instead of nine - equal within one
 * fp16 rounding of the output.  h even, w a multiple of 32: MP_ERR_UNSUPPORTED otherwise. */
int mp_f16_stem_conv_fwd(const float* x_dev, const float* weight_dev, const float* scale_dev, const float* shift_dev, int relu,
                         void* out_c8_dev, int n, int h, int w, mp_stream_t stream);
int mp_plan_add_stem_conv_f16(mp_plan* plan, const float* x_dev, const float* weight_dev, const float* scale_dev, const float* shift_dev,
                              int relu, void* out_c8_dev, int n, int h, int w);
/* Two chained fp16 1x1 convolutions in ONE launch (hrnet.py:107-123, 126-146, stage 1): the expand conv of Bottleneck i,
 *   y = act3(conv1x1(mid; w3) * scale3 + shift3 + res)      cm -> ce channels, res = the block's identity,
 * and the reduce conv of Bottleneck i + 1 on it,
 *   z = act1(conv1x1(y; w1) * scale1 + shift1)               ce -> cr channels,
 * y written once and never read back from HBM.  Channel-blocked fp16 tensors, weights packed by mp_f16_pack_weight (1x1).  y and z
 * are bit-identical to two mp_f16_conv2d_fwd launches.  Built for cm = 64, ce = 256, cr = 64 and h * w a multiple of 64:
 * MP_ERR_UNSUPPORTED otherwise (the caller launches the two convs). */
int mp_f16_expand_reduce_fwd(const void* mid_c8_dev, const void* res_c8_dev, const void* packed_w3_dev, const float* scale3_dev,
                             const float* shift3_dev, int relu3, const void* packed_w1_dev, const float* scale1_dev,
                             const float* shift1_dev, int relu1, void* y_c8_dev, void* z_c8_dev, int n, int cm, int ce, int cr, int h,
                             int w, mp_stream_t stream);
/* The same kernel with BOTH convs on one 64-channel input (the first Bottleneck of stage 1, hrnet.py:74-81, 107-123: its down-sample
 * conv ya = act_a(conv1x1(x; wa) * scale_a + shift_a), 64 -> 256, and its reduce conv zb = act_b(conv1x1(x; wb) * scale_b + shift_b),
 * 64 -> 64): x read once, one launch; bit-identical to the two launches. */
int mp_f16_dual_pw_fwd(const void* x_c8_dev, const void* packed_wa_dev, const float* scale_a_dev, const float* shift_a_dev, int relu_a,
                       const void* packed_wb_dev, const float* scale_b_dev, const float* shift_b_dev, int relu_b, void* ya_c8_dev,
                       void* zb_c8_dev, int n, int cm, int ce, int cr, int h, int w, mp_stream_t stream);
/* The chain with the FIRST Bottleneck's identity computed inside (hrnet.py:74-81, 107-146): y = act3(conv1x1(mid; w3) * scale3 + shift3 + d),
 * d = conv1x1(x0; wd) * scale_d + shift_d rounded to fp16 (the block's down-sample conv of its 64-channel input, no ReLU), then z as
 * in mp_f16_expand_reduce_fwd.  d is neither written nor read back; y and z are bit-identical to the three mp_f16_conv2d_fwd launches. */
int mp_f16_ds_expand_reduce_fwd(const void* mid_c8_dev, const void* x0_c8_dev, const void* packed_wd_dev, const float* scale_d_dev,
                                const float* shift_d_dev, const void* packed_w3_dev, const float* scale3_dev, const float* shift3_dev,
                                int relu3, const void* packed_w1_dev, const float* scale1_dev, const float* shift1_dev, int relu1,
                                void* y_c8_dev, void* z_c8_dev, int n, int cm, int ce, int cr, int h, int w, mp_stream_t stream);
int mp_plan_add_ds_expand_reduce_f16(mp_plan* plan, const void* mid_c8_dev, const void* x0_c8_dev, const void* packed_wd_dev,
                                     const float* scale_d_dev, const float* shift_d_dev, const void* packed_w3_dev,
                                     const float* scale3_dev, const float* shift3_dev, int relu3, const void* packed_w1_dev,
                                     const float* scale1_dev, const float* shift1_dev, int relu1, void* y_c8_dev, void* z_c8_dev, int n,
                                     int cm, int ce, int cr, int h, int w);
int mp_plan_add_dual_pw_f16(mp_plan* plan, const void* x_c8_dev, const void* packed_wa_dev, const float* scale_a_dev,
                            const float* shift_a_dev, int relu_a, const void* packed_wb_dev, const float* scale_b_dev,
                            const float* shift_b_dev, int relu_b, void* ya_c8_dev, void* zb_c8_dev, int n, int cm, int ce, int cr, int h, int w);
int mp_plan_add_expand_reduce_f16(mp_plan* plan, const void* mid_c8_dev, const void* res_c8_dev, const void* packed_w3_dev,
                                  const float* scale3_dev, const float* shift3_dev, int relu3, const void* packed_w1_dev,
                                  const float* scale1_dev, const float* shift1_dev, int relu1, void* y_c8_dev, void* z_c8_dev, int n,
                                  int cm, int ce, int cr, int h, int w);
/* The fp32 form of the chain (csrc/pwchain_f32.hip; hrnet.py:86-146 Bottleneck, 440-470 layer1): expand conv of Bottleneck i
 *   y = relu(conv1x1(mid; w3) * scale3 + shift3 + r)        64 -> 256 channels
 * and reduce conv of Bottleneck i + 1
 *   z = relu(conv1x1(y; w1) * scale1 + shift1)               256 -> 64 channels
 * in one persistent launch with all weight matrices held in registers; NCHW fp32 tensors, weights packed by mp_conv_pack_weight
 * (1x1), y written once and never read back.  The residual r is EITHER the tensor res_dev (x0_dev / packed_wd_dev / scale_d_dev /
 * shift_d_dev null) OR the block's down-sample conv conv1x1(x0; wd) * scale_d + shift_d of its 64-channel input (hrnet.py:74-81),
 * computed inside the launch (res_dev null).  packed_w1_dev / scale1_dev / shift1_dev / z_dev null = the expand conv alone (the last
 * Bottleneck of the stage; not with the down-sample form).  Same values as the stand-alone mp_conv2d_fwd launches up to fp32
 * rounding (the k sums are associated differently).  Built for cm = 64, ce = 256, cr = 64 and h * w a multiple of 64:
 * MP_ERR_UNSUPPORTED otherwise (the caller launches the convs one by one). */
int mp_expand_reduce_fwd(const float* mid_dev, const float* res_dev, const float* x0_dev, const float* packed_wd_dev,
                         const float* scale_d_dev, const float* shift_d_dev, const float* packed_w3_dev, const float* scale3_dev,
                         const float* shift3_dev, const float* packed_w1_dev, const float* scale1_dev, const float* shift1_dev,
                         float* y_dev, float* z_dev, int n, int cm, int ce, int cr, int h, int w, mp_stream_t stream);
int mp_plan_add_expand_reduce(mp_plan* plan, const float* mid_dev, const float* res_dev, const float* x0_dev, const float* packed_wd_dev,
                              const float* scale_d_dev, const float* shift_d_dev, const float* packed_w3_dev, const float* scale3_dev,
                              const float* shift3_dev, const float* packed_w1_dev, const float* scale1_dev, const float* shift1_dev,
                              float* y_dev, float* z_dev, int n, int cm, int ce, int cr, int h, int w);
int mp_plan_add_basicblock_f16(mp_plan* plan, const void* x_c8_dev, const void* packed_w1_dev, const float* scale1_dev,
                               const float* shift1_dev, const void* packed_w2_dev, const float* scale2_dev, const float* shift2_dev,
                               void* out_c8_dev, int n, int c, int h, int w, int rows);
int mp_f16_fuse_upsample_sum(const void* base_dev, const void* t1_dev, int s1, const void* t2_dev, int s2, const void* t3_dev,
                             int s3, void* out_dev, int n, int c, int h, int w, int relu, mp_stream_t stream);
int mp_plan_add_conv_f16(mp_plan* plan, const mp_conv_desc* desc, int variant, const void* x_c8_dev, const void* packed_w_dev,
                         const float* scale_dev, const float* shift_dev, const void* res1_c8_dev, const void* res2_c8_dev,
                         void* out_c8_dev);
int mp_plan_add_fuse_sum_f16(mp_plan* plan, const void* base_dev, const void* t1_dev, int s1, const void* t2_dev, int s2,
                             const void* t3_dev, int s3, void* out_dev, int n, int c, int h, int w, int relu);
/* to_c8 != 0: NCHW fp32 -> c8 fp16, else c8 fp16 -> NCHW fp32 */
int mp_plan_add_layout_f16(mp_plan* plan, int to_c8, const void* x_dev, void* out_dev, int n, int c, int h, int w);
/* Channel concatenation ops.concat((a, b), 1) of the HigherHRNet head (mindpose/models/heads/higher_hrnet_head.py:217-229):
 * out[n] = [a[n] (ca channels), b[n] (cb channels)].  c8 = 0: fp32 NCHW; c8 != 0: channel-blocked fp16, ca a multiple of 8 (a block
 * copy per image; the pad channels of b's last block - zero - become out's).  mp_plan_add_concat records it as a plan entry. */
int mp_concat_channels(const void* a_dev, int ca, const void* b_dev, int cb, void* out_dev, int n, int h, int w, int c8,
                       mp_stream_t stream);
int mp_plan_add_concat(mp_plan* plan, const void* a_dev, int ca, const void* b_dev, int cb, void* out_dev, int n, int h, int w,
                       int c8);
/* Column band of an activation: out[r][0, w_out) = in[r][start, start + w_out) for rows = n*c*h (fp32 NCHW) or n*ceil(c/8)*h
 * (c8 != 0: channel-blocked fp16, one 16-byte block per pixel).  The plan splits a convolution that no kernel serves at its full
 * width (the 512 / 832-pixel images of the bottom-up recipe, hrnet.py:377-385) into output-column bands: each band's input columns
 * are copied out with this entry and the band's conv writes its columns through mp_conv_desc.out_off_x. */
int mp_col_slice(const void* in_dev, void* out_dev, int rows, int w_in, int start, int w_out, int c8, mp_stream_t stream);
int mp_plan_add_col_slice(mp_plan* plan, const void* in_dev, void* out_dev, int rows, int w_in, int start, int w_out, int c8);
/* 1 when mp_conv2d_fwd_variant(desc, variant, ...) would accept this (shape, variant) - -1 = the library heuristic; host-only. */
int mp_conv_supported(const mp_conv_desc* desc, int variant);

/* ---- loader side: the crop that feeds the network -----------------------------------------------------
 * cv2.warpAffine(image, trans, (out_w, out_h), flags=cv2.INTER_LINEAR) of TopDownAffine._affine / _udp_affine
 * (mindpose/data/transform/topdown_transform.py:198-262), optionally fused with vision.Normalize(mean, std) +
 * vision.HWC2CHW (mindpose/data/data_factory.py:129-133).
 *   src          device buffer holding the source images, HWC uint8, 3 channels
 *   src_offsets  [n] int64 (device): byte offset of crop i's source image inside src
 *   src_hw       [n][2] int32 (device): height, width of crop i's source image
 *   flip         NULL or [n] int32 (device): non-zero = crop i is taken from the horizontally flipped source image
 *                (cv2.flip(image, 1) of TopDownHorizontalRandomFlip :481, applied while sampling: no flipped copy is made)
 *   trans        [n][6] fp64 (device): the 2x3 FORWARD matrices (source -> crop) exactly as get_affine_transform /
 *                get_warp_matrix return them; the kernel inverts them as cv2.warpAffine does
 *   normalize=1: out = fp32 [n][3][out_h][out_w], (pixel - mean[c]) / stddev[c]   (mean/std already times 255, host arrays)
 *   normalize=0: out = uint8 [n][out_h][out_w][3], the warped image only
 * Border mode BORDER_CONSTANT(0); OpenCV's fixed-point bilinear arithmetic restated (parity unpinned: no cv2 here). */
int mp_warp_affine(const uint8_t* src_dev, const long long* src_offsets_dev, const int* src_hw_dev, const int* flip_dev,
                   const double* trans_dev, void* out_dev, int n, int out_h, int out_w, int normalize, const float mean[3], const float stddev[3],
                   mp_stream_t stream);

/* Horizontal flip of an NCHW fp32 batch, out[n,c,y,x] = in[n,c,y,W-1-x]: the input of the flip test's second run
 * (mindpose/engine/inferencer/topdown_inferencer.py:168-170), one pass; in and out must not overlap. */
int mp_flip_width(const float* in_dev, float* out_dev, int n, int c, int h, int w, mp_stream_t stream);

/* Bottom-up evaluation input in one pass (mindpose/data/transform/bottomup_transform.py:143-208 BottomUpRescale, :601-645
 * BottomUpPad, data_factory.py:129-133): cv2.resize(image, (tw, th), INTER_LINEAR) of uint8 HWC sources (packed as for
 * mp_warp_affine: src + src_offsets[i], src_hw[i] = (h, w), both device arrays), zero pad on the right and bottom to
 * (pad_h, pad_w) - applied to the uint8 image, so a padded pixel normalises to (0 - mean) / std -, Normalize and HWC2CHW.
 * dst_wh_host [n, 2]: (tw, th) per image, a HOST array (it is checked here and travels in the kernel arguments; up to 32 images are
 * one launch).  out [n, 3, pad_h, pad_w] fp32; mask [n, pad_h, pad_w] uint8, 1 where y < th && x < tw.  mean / stddev already
 * multiplied by 255.  The interpolation restates OpenCV's 8-bit fixed-point linear resize [cv2-knowledge; parity with cv2 itself
 * is unpinned].  MP_ERR_NULL / MP_ERR_SHAPE as mp_warp_affine; tw > pad_w or th > pad_h -> MP_ERR_SHAPE. */
int mp_resize_pad_normalize(const uint8_t* src_dev, const long long* src_offsets_dev, const int* src_hw_dev, const int* dst_wh_host,
                            float* out_dev, uint8_t* mask_dev, int n, int pad_h, int pad_w, const float mean[3],
                            const float stddev[3], mp_stream_t stream);

/* Bottom-up train-time augmentation of a batch in ONE launch (mindpose/data/transform/bottomup_transform.py:304-460
 * BottomUpRandomAffine, :88-140 BottomUpHorizontalRandomFlip, data_factory.py:129-133 Normalize + HWC2CHW): the bilinear warp of
 * the image and the nearest-neighbour warp of the mask into every heat-map stage, each mirrored afterwards where flip says so.
 *   src / src_offsets / src_hw        the uint8 HWC source images, packed as for mp_warp_affine
 *   mask_src / mask_offsets           one uint8 [H, W] mask per image at the SOURCE resolution (src_hw serves both), byte offsets
 *                                     inside mask_src (device, [n] int64); the reference tiles this plane over the stages
 *   trans        [n][s + 1][6] fp64 (device): the 2x3 FORWARD matrices, the s stages first, the image last
 *   flip         NULL or [n] int32 (device): non-zero mirrors the OUTPUTS after the warp - the value computed for column x lands
 *                in column out_w - 1 - x of the image and W_i - 1 - x of stage i's corner (affine, then flip: the reference's
 *                order; NOT mp_warp_affine's flip of the source)
 *   stage_wh_host [s][2] (W_i, H_i), a HOST array
 *   image        [n, 3, out_h, out_w] fp32: mp_warp_affine's normalised planes to the bit (mean / stddev already times 255)
 *   mask         [n, s, hmax, wmax] uint8: cv2.warpAffine(..., INTER_NEAREST), border 0, in the [:H_i, :W_i] corner of stage i,
 *                0 in the padding [cv2-knowledge; parity with cv2 itself is unpinned]
 * Every byte of both outputs is written; integer / fixed-point arithmetic up to the final normalise, no atomics.  Validation
 * before any HIP call: NULL -> MP_ERR_NULL; s outside 1..8 -> MP_ERR_UNSUPPORTED; non-positive extents, a stage larger than
 * (hmax, wmax), a zero stddev or n > 65535 -> MP_ERR_SHAPE. */
int mp_bottomup_train_augment(const uint8_t* src_dev, const long long* src_offsets_dev, const int* src_hw_dev,
                              const uint8_t* mask_src_dev, const long long* mask_offsets_dev, const double* trans_dev,
                              const int* flip_dev, const int* stage_wh_host, float* image_dev, uint8_t* mask_dev, int n, int s,
                              int out_h, int out_w, int hmax, int wmax, const float mean[3], const float stddev[3],
                              mp_stream_t stream);

/* mp_bottomup_train_augment with one source mask plane PER STAGE (the training mask under `expand_mask: True`, whose planes differ
 * by the erosion radius): stage i of image j reads the [H, W] plane at mask_src + mask_offsets[j] + i * mask_stage_stride[j].
 *   mask_stage_stride  [n] int64 (device), bytes; 0 for an image whose single plane serves every stage.  NULL = all zero, which
 *                      IS mp_bottomup_train_augment (that entry calls this one with NULL: same kernel, same bits).
 * Everything else, the validation included, as mp_bottomup_train_augment. */
int mp_bottomup_train_augment_stages(const uint8_t* src_dev, const long long* src_offsets_dev, const int* src_hw_dev,
                                     const uint8_t* mask_src_dev, const long long* mask_offsets_dev,
                                     const long long* mask_stage_stride_dev, const double* trans_dev, const int* flip_dev,
                                     const int* stage_wh_host, float* image_dev, uint8_t* mask_dev, int n, int s, int out_h, int out_w,
                                     int hmax, int wmax, const float mean[3], const float stddev[3], mp_stream_t stream);

/* Bottom-up training masks of a batch, rasterised and eroded on the device (mindpose/data/dataset/coco_bottomup.py:146-189
 * _get_encoded_mask, there a start-up pass over the whole training set through pycocotools and cv2.erode).  TWO launches per batch.
 * A region is one COCO run-length encoding: counts alternate zeros / ones starting with zeros over the column-major pixel index
 * x * H + y and sum to H * W.  A pixel is invalid when any region of its image covers it; stage i of the uint8 [s, H, W] result is 1
 * where no invalid pixel lies under the disc of radius radii[i] centred on the pixel (pixels outside the image count as valid:
 * cv2.erode's default border).  The disc arrives as per-row half widths, so its raster is the caller's definition.
 *   prefix        uint32 [T]: the INCLUSIVE prefix sums of every region's counts, regions back to back (the last of a region = H * W)
 *   region_ptr    int32 [R + 1]: region r owns prefix[region_ptr[r] .. region_ptr[r + 1])
 *   image_tab     int32 [n][4]: (H, W, first region, number of regions) - 0 regions: the image's planes are all ones
 *   offsets       int64 [n][2]: byte offset of the image's [s, H, W] block in out, of its [H, W] row-clearance plane in workspace
 *                 (an image without regions has no clearance plane: its second offset is not looked at)
 *   the four tables are given twice, a HOST copy (validated here, before any HIP call) and the DEVICE copy the kernels read
 *   radii_host    int32 [s], half_widths_host uint8 [s][128]: half_widths[i][d] is the half width of disc i's row at distance d from
 *                 its centre row, 0 <= d <= radii[i] (the table is symmetric in the sign of d); both travel in the kernel arguments
 *   out / workspace  uint8 device buffers of out_bytes / workspace_bytes; workspace holds clear(y, x) = min(255, distance to the
 *                 nearest invalid pixel of row y), stage i is valid iff clear(y + d, x) > half_widths[i][|d|] for every in-image row
 * Launch 1 finds, per pixel and region, the parity of the run that holds x * H + y by binary search (a gather: no scatter, no
 * memset, no atomics) and writes the clearance of the row; launch 2 writes every byte of every stage once.  Integer throughout.
 * Validation: NULL -> MP_ERR_NULL; s outside 1..8 or a radius outside 0..127 -> MP_ERR_UNSUPPORTED; n outside 1..65535, an extent
 * outside 1..16384, a region table that is not ascending, a region whose counts do not sum to H * W, or a block that leaves out /
 * workspace -> MP_ERR_SHAPE. */
int mp_bottomup_train_masks(const uint32_t* prefix_host, const int* region_ptr_host, const int* image_tab_host,
                            const long long* offsets_host, const uint32_t* prefix_dev, const int* region_ptr_dev,
                            const int* image_tab_dev, const long long* offsets_dev, const int* radii_host,
                            const uint8_t* half_widths_host, uint8_t* out_dev, size_t out_bytes, uint8_t* workspace_dev,
                            size_t workspace_bytes, int n, int s, mp_stream_t stream);

/* ---- bottom-up (associative-embedding) decoder, BottomUpHeatMapAEDecoder -------------------------------------------------
 * Replaces mindpose/models/decoders/bottom_up_decoder.py:81-203 (the ~10 MindSpore ops of decode()) with two launches.
 * stages[0 .. num_stages-1]: the model outputs in the reference's order, stages[num_stages-1] the full-resolution one (its h, w
 * are the map size H, W); every stage's first k channels are heat maps, channels k.. of a stage with has_tags are its tags
 * (k of them with tag_per_joint, else 1).  L = the number of stages with tags (1..4).  fp32 NCHW, contiguous.
 *
 * mp_bottomup_parse_nms_topk (bottom_up_decoder.py:102-138 _parse_heatmaps / _aggregate_heatmap, :173-178 _nms, the per-tile
 *   half of :140-171 top_k): heatmap_raw [n,k,H,W] = mean of the stages resized to H x W (ResizeBilinear without half-pixel
 *   centres), 0 where the nearest-resized mask [n,mask_h,mask_w] (uint8) is 0; tagging [n,k_tag,H,W,L] = the resized tags;
 *   nms_kernel 3 / 5 / 7 = the max-pool NMS, 1 = none; the top max_num (value, flat index) of every 16 x 64 tile into the
 *   workspace (mp_bottomup_workspace_bytes).  max_num 1..64, else MP_ERR_UNSUPPORTED.
 * mp_bottomup_gather (bottom_up_decoder.py:140-171 _get_max_preds, :180-203 _shift_coordinate): merges the workspace into the
 *   global top max_num per (image, joint), values descending and equal values in ascending flat index (ops.top_k), and writes
 *   val_k [n,k,M], ind_k [n,k,M,2] (x, y) fp32 and tag_k [n,k,M,L] gathered from tagging; shift_coordinate adds 0.25 * sign of
 *   the heatmap_raw central difference, entry m taking the offset of the m-th smallest selected flat index (the reference's
 *   masked_select order).  Same stream as the first launch, same workspace. */
typedef struct mp_bottomup_stage {
    const float* data_dev; /* [n, c, h, w] */
    int32_t c, h, w;
    int32_t has_tags;
} mp_bottomup_stage;
size_t mp_bottomup_workspace_bytes(int n, int k, int h, int w, int max_num);
int mp_bottomup_parse_nms_topk(const mp_bottomup_stage* stages_host, int num_stages, const uint8_t* mask_dev, int mask_h, int mask_w,
                               int n, int k, int tag_per_joint, int nms_kernel, int max_num, float* heatmap_raw_dev,
                               float* tagging_dev, void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);
int mp_bottomup_gather(const float* heatmap_raw_dev, const float* tagging_dev, const void* workspace_dev, size_t workspace_bytes,
                       int n, int k, int h, int w, int tag_per_joint, int num_tags, int max_num, int shift_coordinate,
                       float* val_k_dev, float* ind_k_dev, float* tag_k_dev, mp_stream_t stream);

/* mp_bottomup_parse_nms_topk_flip: mp_bottomup_parse_nms_topk for the flip test (mindpose/engine/inferencer/bottomup_inferencer.py:
 * 252-297, _MultiRunNet), folding the outputs of the horizontally mirrored image into the same launch.  flipped_stages[i] is the
 * output of the mirrored run beside stages[i] (same c, h, w, has_tags, else MP_ERR_SHAPE); flip_index_host [k] is a HOST array, joint
 * j of the plain run meeting channel flip_index[j] of the mirrored one.  At stage resolution, before any resize (the resize has no
 * half-pixel centres, so it does not commute with the mirror; each of its four taps is the averaged value):
 *     heat_i[n,j,y,x] = (stages_i[n,j,y,x] + flipped_i[n,flip_index[j],y,w_i-1-x]) * 0.5f     (one fp32 add, one fp32 multiply)
 * and on the last axis of tagging [n,k,H,W,2L] the L plain tags stages_i[n,k+j,y,x] in stage order, then the L mirrored-back tags
 * flipped_i[n,k+flip_index[j],y,w_i-1-x] in the same order; everything after that (stage mean, the un-mirrored mask, NMS, per-tile
 * top-k, the workspace) is mp_bottomup_parse_nms_topk's, and mp_bottomup_gather follows with num_tags = 2L.  The mirrored maps are
 * never flipped, averaged or concatenated in memory.
 * Refusals, all before the launch: a NULL array or data pointer MP_ERR_NULL; a flip_index entry outside [0, k) MP_ERR_SHAPE (the
 * entry copies the index into the kernel parameters, so no caller can make the kernel read outside a stage); tag_per_joint == 0
 * (the reference indexes the single tag channel with the k-long flip_index: out of range), k > 64 or 2L > 4 MP_ERR_UNSUPPORTED. */
int mp_bottomup_parse_nms_topk_flip(const mp_bottomup_stage* stages_host, const mp_bottomup_stage* flipped_stages_host,
                                    const int32_t* flip_index_host, int num_stages, const uint8_t* mask_dev, int mask_h, int mask_w,
                                    int n, int k, int tag_per_joint, int nms_kernel, int max_num, float* heatmap_raw_dev,
                                    float* tagging_dev, void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);

/* mp_bottomup_parse_nms_topk_multi: the first decoder launch of the multi-scale test (this project's protocol; the
 * reference ships none), over num_runs (1..4) runs of the network on the batch resized by one scale factor each.  runs_host is a
 * HOST array; runs_host[r].stages [num_stages] (HOST) are run r's outputs and runs_host[r].flipped [num_stages] those of its
 * horizontally mirrored input, NULL in every run = no flip test (then flip_index_host is NULL too).  Run base_run is the scale-1
 * run: its last stage is the map (H, W), and the tags come from it alone, exactly as the plain / flip entry writes them (L slots,
 * or 2L with the flip test); tag channels of the other runs are never read.  Every run has num_stages stages with the base run's
 * c and has_tags per stage; its h, w are free (smaller or larger than the map: in / out > 1 is allowed).  With
 *     t_{r,i}   = stages_i of run r, or with the flip test (stages_i[n,j,y,x] + flipped_i[n,flip_index[j],y,w_i-1-x]) * 0.5f,
 *     R(.)      = ResizeBilinear to (H, W) without half-pixel centres, src = dst * (in / out); for the base run's last stage
 *                 the direct read,
 *     v_r       = R(t_{r,last}); v_r = v_r + R(t_{r,i}) for i = 0 .. num_stages - 2; v_r = v_r / (float)num_stages if > 1 stage,
 *     total     = v_0 + v_1 + ... in array order; total = total / (float)num_runs if num_runs > 1 (a true division),
 * heatmap_raw [n,k,H,W] = total, 0 where the nearest-resized mask is 0.  num_runs == 1 is mp_bottomup_parse_nms_topk (or _flip)
 * operation for operation.  NMS, per-tile top-k, the workspace (mp_bottomup_workspace_bytes of the base map) and the
 * mp_bottomup_gather that follows are unchanged.  Deterministic, no atomics.  The launch parameters (at most 16 stage records and
 * the 64-entry joint permutation, under 1.5 KiB) travel BY VALUE in the kernel arguments: the entry writes no device table.
 * Refusals, all before the launch: a NULL array or data pointer, or mirrored arrays without flip_index_host (or the reverse),
 * MP_ERR_NULL; num_runs outside 1..4, base_run outside [0, num_runs), mirrored arrays in some runs only, a stage whose c or
 * has_tags differs from the base run's, non-positive extents, a mirrored stage shaped unlike its plain one, a flip_index entry
 * outside [0, k) MP_ERR_SHAPE; with the flip test tag_per_joint == 0, k > 64 or 2L > 4 MP_ERR_UNSUPPORTED; everything
 * mp_bottomup_parse_nms_topk refuses, on the base run. */
typedef struct mp_bottomup_run {
    const mp_bottomup_stage* stages;  /* HOST [num_stages] */
    const mp_bottomup_stage* flipped; /* HOST [num_stages], or NULL */
} mp_bottomup_run;
int mp_bottomup_parse_nms_topk_multi(const mp_bottomup_run* runs_host, int num_runs, int base_run, const int32_t* flip_index_host,
                                     int num_stages, const uint8_t* mask_dev, int mask_h, int mask_w, int n, int k,
                                     int tag_per_joint, int nms_kernel, int max_num, float* heatmap_raw_dev, float* tagging_dev,
                                     void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);

/* mp_resize_bilinear_nchw: ops.ResizeBilinear((oh, ow)), align_corners=False, half_pixel_centers=False, of `planes` contiguous fp32
 * planes [planes, ih, iw] -> [planes, oh, ow]: src = dst * ((float)in / (float)out), x0 = min(floor(src), in - 1),
 * x1 = min(x0 + 1, in - 1), top = a + (b - a) * dx, bot = c + (d - c) * dx, out = top + (bot - top) * dy in fp32 without
 * contraction - the decoder's own device function, so pixel q of the source lands on s * q of a map scaled by s and the decoder's
 * resize reads exactly there.  16-byte stores when ow % 4 == 0 and out is 16-byte aligned, else 4-byte stores.  in and out must not
 * overlap.  NULL -> MP_ERR_NULL; non-positive extents or a plane of 2^31 or more pixels -> MP_ERR_SHAPE. */
int mp_resize_bilinear_nchw(const float* in_dev, float* out_dev, int planes, int ih, int iw, int oh, int ow, mp_stream_t stream);

/* mp_bottomup_refine_missing (mindpose/engine/inferencer/bottomup_inferencer.py:189-250, refine_missing_joint): for every person p
 * of a batch's person list (image person_image[p], mean tag mean_tag [P, L] formed by the caller) and every joint, the first
 * arg-max in flat index over the joint's H x W map of  heatmap_raw - rint(sqrt(sum_l (tagging_l - mean_tag_l)^2))  in fp32 (tag
 * channel 0 without tag_per_joint); found [P, k, 3] = (x + 0.5 +- 0.25, y + 0.5 +- 0.25, heat-map value) of that pixel, the shifts by
 * the reference's two clamped neighbour comparisons.  One workgroup per (joint, person); num_persons 0 = no launch, MP_OK.  Inputs
 * are assumed finite; a person_image outside [0, n) leaves its rows of found unwritten. */
int mp_bottomup_refine_missing(const float* heatmap_raw_dev, const float* tagging_dev, const float* mean_tag_dev,
                               const int* person_image_dev, int num_persons, int n, int k, int h, int w, int tag_per_joint,
                               int num_tags, float* found_dev, mp_stream_t stream);

/* mp_bottomup_match_by_tag (bottomup_match.hip; mindpose/utils/match.py:15-116, match_by_tag, for a batch): groups the decoder's
 * detections of n images in ONE launch, one wave64 per image, bit-equal to the host function: scipy's rectangular
 * linear_sum_assignment (tie order included), numpy's float32 mean / norm and the reference's dict semantics are restated in the
 * kernel file's header.  val_k [n, k, m], tag_k [n, k, m, L], ind_k [n, k, m, 2]; joint_order_host [k] is a HOST array, a permutation
 * of 0 .. k - 1, checked and copied by the entry.  people [n, k * m, k, 3 + L] receives person p of image i at people[i, p], in
 * the order the groups were opened; a person's [k, 3 + L] block is zeroed when its group is opened and, for status[i] == 0, nothing
 * beyond counts[i] persons is ever written (k * m is an exact bound: every detection opens at most one group).  status[i] == 1: a
 * visible detection of image i carries a NaN or infinite tag (scipy raises on such a matrix), found before anything is written;
 * status[i] == 2: finite tags so far apart that a float32 distance overflows, found while the costs are scanned - the persons of the
 * earlier steps may have been written.  Either way counts[i] is 0 and the caller runs the host function for that image.  workspace >= mp_bottomup_match_workspace_bytes.
 * Before any HIP call: n == 0 -> MP_OK without a launch; NULL -> MP_ERR_NULL; non-positive extents or a joint_order that is no
 * permutation -> MP_ERR_SHAPE; k > 64, m > 64, L > 4 or k * m > 1024 -> MP_ERR_UNSUPPORTED (mp_bottomup_match_supported answers
 * 1 / 0 for the same limits, host-only); a missing or short workspace -> MP_ERR_WORKSPACE. */
int mp_bottomup_match_supported(int k, int m, int num_tags);
size_t mp_bottomup_match_workspace_bytes(int n, int k, int m, int num_tags);
int mp_bottomup_match_by_tag(const float* val_k_dev, const float* tag_k_dev, const float* ind_k_dev, int n, int k, int m, int num_tags,
                             const int* joint_order_host, float vis_thr, float tag_thr, int ignore_too_much, int use_rounded_norm,
                             float* people_dev, int* counts_dev, int* status_dev, void* workspace_dev, size_t workspace_bytes,
                             mp_stream_t stream);

/* mp_bottomup_finish_people (bottomup_ops.hip; the tail of mindpose/engine/inferencer/bottomup_inferencer.py:120-150 and :189-250 for a
 * batch): per-person score, mean tag and the missing-joint refinement of the persons mp_bottomup_match_by_tag left in device
 * memory, with no host value that depends on how many there are.  people [n, k * m, k, 3 + L], counts [n] and status [n] are that
 * entry's outputs, untouched; heatmap_raw [n, k, h, w] and tagging [n, ktag, h, w, L] the decoder's (ktag = k with tag_per_joint,
 * else 1).  Both grids are sized from the capacity k * m; every workgroup reads counts[i], clamped to [0, k * m], and status[i]
 * itself and exits for p >= counts[i] or status[i] != 0: rows of people beyond counts[i] are never read, and nothing of an image
 * that was handed over (status != 0) is read or written.
 *   Launch A, one wave64 per (person, image): scores [n, k * m] = np.mean of the person's value column (person[:, 2], k values)
 *     and, in the workspace, the mean tag [n, k * m, L] over the joints with value > 0 in joint order, followed by the number of
 *     those joints [n, k * m] (int32).  The tag of joint j is read at column (int)x, row (int)y of the person's row j - truncated
 *     toward zero, then clamped to the map, a NaN coordinate reading column / row 0 - from tag channel j (channel 0 without
 *     tag_per_joint).  Both means are numpy's float32 ones (rule (b) of bottomup_match.hip): a 1-D view - the score and the mean
 *     tag with L == 1 - sums sequentially from 0 below eight values and with eight accumulators over whole blocks of eight, combined
 *     ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)), the tail added in order, from eight on; L >= 2 sums sequentially in joint order from
 *     the first tag; then one float32 division by the number of values.
 *   Launch B, with refine != 0 only, behind A in stream order, one workgroup per (joint, person, image): for the joints with
 *     person[j, 2] == 0 of a person with at least one located joint, the arg-max of mp_bottomup_refine_missing (the same device
 *     function) against the person's mean tag; when the winner's heat-map value is > 0, person[j, 0:3] = (x, y, value) in place.
 *     Every other workgroup exits after reading counts, status and one value.  Each (joint, person) scans its own map: (1 + L) * h * w
 *     * 4 bytes per MISSING joint, none for a located one.
 * Deterministic, no atomics.  workspace >= mp_bottomup_finish_workspace_bytes (0 outside the limits).
 * Before any HIP call: n == 0 -> MP_OK without a launch; NULL -> MP_ERR_NULL; n < 0 or n > 65535, non-positive k, m, h, w or
 * num_tags, or a map of 2^31 or more pixels -> MP_ERR_SHAPE; k > 64, m > 64, L > 4 or k * m > 1024 (the grouping entry's limits) ->
 * MP_ERR_UNSUPPORTED; a missing or short workspace -> MP_ERR_WORKSPACE. */
size_t mp_bottomup_finish_workspace_bytes(int n, int k, int m, int num_tags);
int mp_bottomup_finish_people(float* people_dev, const int* counts_dev, const int* status_dev, const float* heatmap_raw_dev,
                              const float* tagging_dev, int n, int k, int m, int h, int w, int tag_per_joint, int num_tags, int refine,
                              float* scores_dev, void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);

/* ---- bottom-up training ends: masked heat-map MSE, associative-embedding loss, target generation (bottomup_train_ops.hip) -------
 * Every entry validates before any HIP call (NULL -> MP_ERR_NULL, bad extents / strides -> MP_ERR_SHAPE), fully writes its
 * outputs and is deterministic: no atomics, fixed-order reductions.
 *
 * mp_joints_mse_mask_fwd / _bwd (mindpose/models/loss/mse.py:47-72, JointsMSELossWithMask):
 *   loss = sum((pred - target)^2 * mask[n,h,w]) / (n k h w)  - masked pixels count in the divisor;
 *   grad_pred = 2 (pred - target) mask grad_out[0] / (n k h w)  (grad_out NULL = 1).
 *   pred, target and grad_pred are [n,k,h,w] VIEWS given by element strides of batch / channel / row (*_sn, *_sc, *_sr; the column
 *   stride is 1), mask is an [n,h,w] view (fp32, or one byte per pixel with mask_is_u8) with batch / row strides: a corner of a
 *   padded target and the heat-map channels of a stage tensor are read and written in place.  16-byte accesses when w, the
 *   strides and the base addresses allow.  workspace >= mp_joints_mse_mask_workspace_bytes(n, k), else MP_ERR_WORKSPACE.
 *
 * mp_ae_loss_fwd / _bwd (mindpose/models/loss/ae.py:40-89, AELoss with reduction "mean"; eps = 0.01):
 *   tags [n,k,hw] fp32 with a batch stride (the tag channels of a stage tensor; k = 1 without tag_per_joint), tag_ind [n,m,k,2]
 *   int32 = (flat pixel index, flag) contiguous; loss2 = (push, pull), each the mean over n.  The backward takes grad_out2 = the
 *   two upstream gradients and writes grad_tags [n,k,hw] (batch stride): zero but for the indexed pixels, persons that share a
 *   pixel summed in ascending m.  An index outside [0, hw) counts as flag 0.  m <= 256, else MP_ERR_UNSUPPORTED.
 *   workspace >= mp_ae_loss_workspace_bytes(n).
 *
 * mp_bottomup_target (mindpose/data/transform/bottomup_transform.py:527-598, BottomUpGenerateTarget for a batch):
 *   keypoints [n,s,m,k,3] fp32 already scaled per stage, counts [n] int32 persons per image (rows beyond are ignored),
 *   stage_wh_host [s][2] = (W, H) on the host; target [n,s,k,hmax,wmax] fp32 = max over persons of the Gaussian, 0 in the padding
 *   of smaller stages; tag_ind [n,s,max_num,k,2] int32 (tag_per_joint) or [n,s,max_num,2].  s <= 8, m and max_num <= 256 and a
 *   whole 3 sigma, else MP_ERR_UNSUPPORTED. */
size_t mp_joints_mse_mask_workspace_bytes(int n, int k);
int mp_joints_mse_mask_fwd(const float* pred_dev, long long pred_sn, long long pred_sc, long long pred_sr, const float* target_dev,
                           long long target_sn, long long target_sc, long long target_sr, const void* mask_dev, int mask_is_u8,
                           long long mask_sn, long long mask_sr, float* loss_dev, void* workspace_dev, size_t workspace_bytes, int n,
                           int k, int h, int w, mp_stream_t stream);
int mp_joints_mse_mask_bwd(const float* pred_dev, long long pred_sn, long long pred_sc, long long pred_sr, const float* target_dev,
                           long long target_sn, long long target_sc, long long target_sr, const void* mask_dev, int mask_is_u8,
                           long long mask_sn, long long mask_sr, const float* grad_out_dev, float* grad_pred_dev, long long grad_sn,
                           long long grad_sc, long long grad_sr, int n, int k, int h, int w, mp_stream_t stream);
size_t mp_ae_loss_workspace_bytes(int n);
int mp_ae_loss_fwd(const float* tags_dev, long long tag_batch_stride, const int32_t* tag_ind_dev, float* loss2_dev,
                   void* workspace_dev, size_t workspace_bytes, int n, int m, int k, int hw, mp_stream_t stream);
int mp_ae_loss_bwd(const float* tags_dev, long long tag_batch_stride, const int32_t* tag_ind_dev, const float* grad_out2_dev,
                   float* grad_tags_dev, long long grad_batch_stride, int n, int m, int k, int hw, mp_stream_t stream);
int mp_bottomup_target(const float* keypoints_dev, const int* counts_dev, const int* stage_wh_host, float* target_dev,
                       int32_t* tag_ind_dev, int n, int s, int m, int k, int hmax, int wmax, int max_num, int tag_per_joint,
                       double sigma, mp_stream_t stream);

/* fp16 (amp O2) training passes over channel-blocked fp16 activations; same contracts as mp_bn_train_fwd / _bwd and
 * mp_fuse_upsample_sum_bwd (statistics, gamma / beta gradients and the workspace stay fp32 / fp64; mp_bn_workspace_bytes) */
int mp_f16_bn_train_fwd(const void* z_dev, const float* gamma_dev, const float* beta_dev, const void* res_dev, void* y_dev,
                        float* save_mean_dev, float* save_invstd_dev, float* moving_mean_dev, float* moving_var_dev, int n, int c,
                        int hw, float eps, float momentum, int relu, void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);
/* dgamma_acc / dbeta_acc (both or neither, may be NULL): the gamma / beta gradients are ALSO added into these buffers (the
 * caller's gradient arena), which saves the framework's separate accumulate launch.
 * ReLU mask (relu != 0): taken from the stored forward output y_dev - or, for a layer WITHOUT residual input (dres_dev NULL),
 * re-derived from z with the forward arithmetic when y_dev is NULL and beta_dev is given (y is then not read: two tensor
 * reads less).  beta_dev may be NULL when y_dev is passed. */
int mp_f16_bn_train_bwd(const void* dy_dev, const void* z_dev, const void* y_dev, const float* gamma_dev, const float* beta_dev,
                        const float* save_mean_dev, const float* save_invstd_dev, void* dz_dev, void* dres_dev, float* dgamma_dev,
                        float* dbeta_dev, float* dgamma_acc_dev, float* dbeta_acc_dev, int n, int c, int hw, int relu,
                        void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);
int mp_f16_fuse_upsample_sum_bwd(const void* dy_dev, const void* out_dev, void* dbase_dev, void* dt1_dev, int s1, void* dt2_dev,
                                 int s2, void* dt3_dev, int s3, int n, int c, int h, int w, int relu, mp_stream_t stream);

/* ---- BatchNorm fused out of the amp-O2 training step (round 3) ------------------------------------------------------------------
 * Reference: every conv of mindpose/models/backbones/hrnet.py:51-64 is followed by nn.BatchNorm2d, trained under amp O2
 * (tools/train.py:170-181).  MindSpore runs conv, the batch-statistics reduction and the normalisation as separate cells; here the
 * conv launch that PRODUCES a tensor also produces the per-channel partial sums its BatchNorm needs, so the reduction passes
 * over the tensor disappear in both directions:
 *   mode 1 (forward):  the launch computes z = conv(x); partials of  sum z, sum z*z  over the fp16-rounded output.
 *   mode 2 (backward): the launch computes the gradient dy reaching a BatchNorm's OUTPUT (a stride-1 data-gradient conv; res1 = the
 *                      residual gradient, as in mp_f16_conv2d_fwd).  z_dev = that BatchNorm's input, y_dev its output (relu != 0:
 *                      mask = y > 0), both in the output geometry.  The tensor STORED is g = dy * mask, and the partials are
 *                      sum g, sum g * z (raw z: the consumer forms sum g * xhat = invstd * (sum g z - mean * sum g) in fp64).
 *                      Kernel 1x1 or 3x3, plain output mapping.  mean / invstd / gamma / beta of the struct are unused by the conv.
 * partials: fp32 [ceil(cout/8)][n_parts][8][2], n_parts = mp_f16_conv_stats_parts(desc, variant) (one slot per pixel-tile workgroup;
 * variant -1 = the library's deterministic choice, the same in both calls; 0 = this variant / shape has no statistics build: use
 * the plain entry + the reduction passes).  Fixed summation order, no
 * atomics: bit-reproducible.  The conv output is bit-identical to mp_f16_conv2d_fwd's (mode 2: times the mask). */
typedef struct mp_f16_conv_stats {
    int mode, relu;
    float* partials_dev;
    size_t partials_bytes;
    const void* z_dev;
    const void* y_dev;
    const float* mean_dev;
    const float* invstd_dev;
    const float* gamma_dev;
    const float* beta_dev;
    /* mode 1 only - BatchNorm apply of the layer BELOW on this conv's input operand (hrnet.py:67-72: conv1 -> bn1 -> relu -> conv2
     * without a pass over y1): x_c8_dev holds the RAW output z of the conv below, pre_scale / pre_shift its folded batch statistics
     * (mp_f16_bn_train_finalize: [round_up(cin, 32)] floats, zeros behind cin); the kernel convolves
     * act(z * scale + shift) - the same fp32 fma, ReLU and single fp16 rounding as mp_f16_bn_train_fwd_stats - and, when
     * pre_out_dev is given, also stores that activation tensor (geometry of x; the backward pass reads it).  Bit-identical to the
     * apply pass followed by the plain launch.  3x3 stride-1 weights-in-registers variants only: MP_ERR_UNSUPPORTED otherwise. */
    const float* pre_scale_dev;
    const float* pre_shift_dev;
    void* pre_out_dev;
    int pre_relu;
} mp_f16_conv_stats;
int mp_f16_conv_stats_parts(const mp_conv_desc* desc, int variant);
/* 1 when mp_f16_conv2d_fwd_stats(desc, variant, ...) accepts stats->pre_scale_dev (BatchNorm apply of the layer below on the input
 * operand): an explicit variant of the weights-in-registers family on a 3x3 stride-1 layer staged one image per tile. */
int mp_f16_conv_pre_supported(const mp_conv_desc* desc, int variant);
/* 1 when mp_f16_conv2d_fwd (stats_mode 0; n_res = 0 / 1 / 2 residual tensors) or mp_f16_conv2d_fwd_stats (stats_mode 1 / 2; n_res
 * 0 / 1) would ACCEPT this (shape, tile variant) - the entry's own checks and the kernel family's own dispatch run without the
 * launch; host-only, no device work.  0 = the entry would answer MP_ERR_UNSUPPORTED (or a shape error).  The test matrix is
 * generated from this query, so a pair that stops being served shows up as a failing floor test instead of a skip. */
int mp_f16_conv_supported(const mp_conv_desc* desc, int variant, int n_res, int stats_mode);
/* The launch record that query builds, as numbers (host-only; tests pin the tile geometry with it): out[0] = the build's return
 * code, out[1] = the dry dispatch's; after an accepted build: kernel size, stride, variant, LDS bytes, every scalar field of the
 * kernel parameter block in declaration order (magic numbers unsigned), every pointer field as 0 / 1 (null / set), and the byte
 * offset of the partial-sum pointer from partials_dev.  Returns the number of words written, MP_ERR_WORKSPACE when cap is too
 * small (80 is enough). */
int mp_f16_conv_launch_words(const mp_conv_desc* desc, int variant, int n_res, int stats_mode, int64_t* out, int cap);
int mp_f16_conv2d_fwd_stats(const mp_conv_desc* desc, int variant, const void* x_c8_dev, const void* packed_w_dev,
                            const float* scale_dev, const float* shift_dev, const void* res1_c8_dev, void* out_c8_dev,
                            const mp_f16_conv_stats* stats, mp_stream_t stream);
/* The consumers.  mp_f16_bn_train_fwd_stats: mp_f16_bn_train_fwd without its reduction pass (statistics from the mode-1 partials;
 * one launch: every workgroup folds the partials of its 8 channels itself, in a fixed order; above 512 slots a small fold
 * launch runs first).  mp_f16_bn_train_bwd_stats: dy_dev is the PRE-MASKED gradient g a mode-2 launch stored;
 *   dz = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat));  the residual branch's gradient is g itself (no dres tensor).
 * workspace: mp_bn_workspace_bytes(c). */
int mp_f16_bn_train_fwd_stats(const void* z_dev, const float* gamma_dev, const float* beta_dev, const void* res_dev, void* y_dev,
                              float* save_mean_dev, float* save_invstd_dev, float* moving_mean_dev, float* moving_var_dev, int n,
                              int c, int hw, float eps, float momentum, int relu, const float* partials_dev, int n_parts,
                              void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);
/* The statistics half of mp_f16_bn_train_fwd_stats alone (reference: nn.BatchNorm2d in training mode, hrnet.py:51-64): saved mean /
 * invstd, moving averages and the folded scale_dev / shift_dev ([ceil(c/8)*8] floats, zeros on padding channels) for a consumer
 * that applies the BatchNorm on its own operand (mp_f16_conv_stats.pre_scale_dev).  Same fold order and arithmetic as the apply
 * pass: the two routes give bit-identical activations. */
int mp_f16_bn_train_finalize(const float* gamma_dev, const float* beta_dev, float* save_mean_dev, float* save_invstd_dev,
                             float* moving_mean_dev, float* moving_var_dev, int n, int c, int hw, float eps, float momentum,
                             const float* partials_dev, int n_parts, float* scale_dev, float* shift_dev, void* workspace_dev,
                             size_t workspace_bytes, mp_stream_t stream);
/* The two element-wise producers of a BatchNorm's output gradient with the same statistics (partials [ceil(c/8)][n_parts][8][2],
 * n_parts = mp_f16_ew_stats_parts(n, c, hw of the OUTPUT tensor)):
 *   mp_f16_sum_tensors_stats: out = fp16(((a + b) + c) + d) * [y > 0] - mp_sum_tensors (the gradients of the consumers of a branch
 *     output, hrnet.py:327-339) followed by the mask; sums of g, g * z.
 *   mp_f16_fuse_sum_bwd_term_stats: ONE term of mp_f16_fuse_upsample_sum_bwd (scale s; s = 1: the base term), masked with y_t > 0 when
 *     relu_t; z_t / y_t: input / output of the BatchNorm that produced the term. */
int mp_f16_ew_stats_parts(int n, int c, int hw);
int mp_f16_fuse_term_stats_parts(int n, int c, int h, int w, int s); /* n_parts of mp_f16_fuse_sum_bwd_term_stats (h, w: full resolution) */
int mp_f16_sum_tensors_stats(const void* a_dev, const void* b_dev, const void* c_dev, const void* d_dev, void* out_dev, const void* z_dev,
                             const void* y_dev, int relu, int n, int c, int hw, float* partials_dev, size_t partials_bytes,
                             mp_stream_t stream);
int mp_f16_fuse_sum_bwd_term_stats(const void* dy_dev, const void* out_dev, void* dt_dev, int s, int n, int c, int h, int w, int relu,
                                   const void* z_t_dev, const void* y_t_dev, int relu_t, float* partials_dev, size_t partials_bytes,
                                   mp_stream_t stream);
int mp_f16_bn_train_bwd_stats(const void* g_dev, const void* z_dev, const float* gamma_dev, const float* save_mean_dev,
                              const float* save_invstd_dev, void* dz_dev, float* dgamma_dev, float* dbeta_dev, float* dgamma_acc_dev,
                              float* dbeta_acc_dev, int n, int c, int hw, const float* partials_dev, int n_parts,
                              void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);

/* Up to FOUR apply-only BatchNorm passes as ONE launch: the k-th BatchNorm of every branch of an HRModule (hrnet.py:202-241) -
 * independent tensors of different shapes, each ~10 us of launch, fold and tail around a few us of streaming when launched alone.
 * A job carries exactly the arguments of mp_f16_bn_train_fwd_stats / mp_f16_bn_train_bwd_stats (same results, bit for bit). */
typedef struct mp_f16_bn_fwd_job {
    const void* z_dev; const float* gamma_dev; const float* beta_dev; const void* res_dev; void* y_dev;
    float* save_mean_dev; float* save_invstd_dev; float* moving_mean_dev; float* moving_var_dev;
    const float* partials_dev; void* workspace_dev; size_t workspace_bytes;
    int n, c, hw, relu, n_parts, reserved;
} mp_f16_bn_fwd_job;
typedef struct mp_f16_bn_bwd_job {
    const void* g_dev; const void* z_dev; const float* gamma_dev; const float* save_mean_dev; const float* save_invstd_dev; void* dz_dev;
    float* dgamma_dev; float* dbeta_dev; float* dgamma_acc_dev; float* dbeta_acc_dev;
    const float* partials_dev; void* workspace_dev; size_t workspace_bytes;
    int n, c, hw, n_parts;
} mp_f16_bn_bwd_job;
int mp_f16_bn_train_fwd_stats_grouped(const mp_f16_bn_fwd_job* jobs, int n_jobs, float eps, float momentum, mp_stream_t stream);
int mp_f16_bn_train_bwd_stats_grouped(const mp_f16_bn_bwd_job* jobs, int n_jobs, mp_stream_t stream);

/* out = a + b (+ c) (+ d) over `bytes` bytes (a multiple of 16) of fp32 (half = 0) or fp16 (half = 1, fp32 sums, one rounding):
 * the fan-in of gradients at a tensor with several consumers - every branch output of an HRModule feeds every exchange-unit row
 * (hrnet.py:318-344) - in one pass instead of the framework's k - 1 pairwise adds.  out may alias an input. */
int mp_sum_tensors(const void* a_dev, const void* b_dev, const void* c_dev, const void* d_dev, void* out_dev, size_t bytes, int half,
                   mp_stream_t stream);
/* weight gradient of a conv (kernel 1x1 or 3x3, stride 1 or 2, padding k/2) from channel-blocked fp16 x and dz on the fp16
 * matrix cores, fp32 accumulation and fp32 result dw [Cout,Cin,kh,kw] (times `scale`: pass 1 / loss_scale); accumulate != 0
 * adds into dw (the caller's gradient arena) instead of overwriting; workspace from mp_f16_conv_wgrad_workspace_bytes */
size_t mp_f16_conv_wgrad_workspace_bytes(const mp_conv_desc* desc);
int mp_f16_conv_wgrad(const mp_conv_desc* desc, const void* x_c8_dev, const void* dz_c8_dev, float* dw_dev, float scale,
                      int accumulate, void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);
/* The same for 1 .. 8 layers of ONE shape in a single launch pair (weight gradients are leaves of the backward pass, tools/train.py:233:
 * nothing waits for them before the update, so the layers of an HRNet branch - hrnet.py:202-241, eight 3x3 convs of one shape - are
 * collected and run together): per layer fewer, longer pixel slabs, 1/n of the launches.  x / dz / dw: HOST arrays of n_jobs device
 * pointers (they travel in the kernel arguments: no upload, hipGraph-capturable).  Same fixed-order reduction per layer as the
 * single-layer entry; a layer's result does not depend on its group (slab partition aside: fp32 summation order). */
size_t mp_f16_conv_wgrad_grouped_workspace_bytes(const mp_conv_desc* desc, int n_jobs);
int mp_f16_conv_wgrad_grouped(const mp_conv_desc* desc, const void* const* x_dev, const void* const* dz_dev, float* const* dw_dev,
                              int n_jobs, float scale, int accumulate, void* workspace_dev, size_t workspace_bytes, mp_stream_t stream);
/* The launch a weight-gradient entry point builds, as numbers (host-only; tests pin the geometry and the dispatch with it).
 * half = 0: mp_conv_wgrad (n_jobs 0 or 1); half = 1: mp_f16_conv_wgrad (n_jobs = 0) or mp_f16_conv_wgrad_grouped (n_jobs 1 .. 8).
 * out[0] = the return code of the geometry; after MP_OK: every non-pointer field of the kernel parameter block in declaration
 * order (magic numbers unsigned), the grid (x, y, z), the block, the LDS bytes, the kernel (half, form, kernel size, stride; form:
 * fp32 0 = scalar-staged, 1 = pipelined; fp16 0 = LDS-DMA 32 x 32, 1 = wide, 2 = narrow, 3 = register-staged) and the slab reduce
 * (threads per element or 0 for the plain kernel, workgroups, jobs).  Returns the number of words written, MP_ERR_WORKSPACE when
 * cap is too small (64 is enough). */
int mp_conv_wgrad_launch_words(const mp_conv_desc* desc, int half, int n_jobs, int64_t* out, int cap);

/* ---- training kernels of the SimpleBaseline-ResNet family ---------------------------------------------------------------
 * mp_maxpool3x3s2_same_bwd: backward of nn.MaxPool2d(3, 2, pad_mode="same") (resnet.py:190), gradient to the first maximum of
 *   each window in scan order; fp32 NCHW.
 * mp_stem_conv_wgrad: weight gradient of the k x k (k = 7 or 3) stride-2 padding-k/2 stem conv with <= 4 input channels
 *   (resnet.py:180-188), fp32 NCHW x [n,cin,h,w], dz [n,cout,ho,wo] -> dw [cout,cin,k,k].
 * mp_f16_gather_phase: out[n,c,m,k] = x[n,c,2m+phase_y,2k+phase_x] on channel-blocked fp16 (x is [n,c,2h,2w]): the sub-pixel
 *   phase of a gradient that the 2x2 phase kernels of the transposed convolution (mp_f16_pack_weight mode 4) consume.
 * The transposed convolution's weight gradient is mp_f16_conv_wgrad on a 4x4 stride-2 padding-1 descriptor with the roles
 *   (x := dy at the up-sampled resolution, dz := the layer input): dW[cin_t][cout_t][ky][kx] = sum x_t[m] * dy[2m+ky-1]. */
int mp_maxpool3x3s2_same_bwd(const float* x_dev, const float* dy_dev, float* dx_dev, int n, int c, int h, int w, mp_stream_t stream);
int mp_stem_conv_wgrad(const float* x_dev, const float* dz_dev, float* dw_dev, int n, int cin, int h, int w, int cout, int k,
                       mp_stream_t stream);
int mp_f16_gather_phase(const void* x_c8_dev, void* out_c8_dev, int n, int c, int h, int w, int phase_y, int phase_x,
                        mp_stream_t stream);
/* the same gather on fp32 NCHW; the fp32 transposed-conv gradients use it with mp_conv_pack_weight mode 4 (data gradient of
 * phase (phase_y, phase_x)) and mp_conv_wgrad on a 4x4 stride-2 padding-1 descriptor with the roles exchanged */
int mp_gather_phase(const float* x_dev, float* out_dev, int n, int c, int h, int w, int phase_y, int phase_x, mp_stream_t stream);

/* Diagnostics: only a library built with -DMP_CONV_STAMPS=1 (never the product build) records per-workgroup
 * phase cycle counters (8 x uint64 per workgroup) of each conv launch into this device buffer; the product
 * build returns MP_ERR_UNSUPPORTED. */
int mp_debug_set_stamp_buffer(void* dev_ptr, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* MINDPOSE_HIP_H */

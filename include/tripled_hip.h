/*
 * tripled_hip.h -- C ABI of libtripled_hip.so: hand-written CDNA4 (gfx950) kernels for
 * the self-supervised depth loss hot path.
 *
 * The reference (ufukpage/TripleD, pure Python/PyTorch) has NO native interface on this
 * path; its hot ops are nn.Module methods built from stock ATen calls.  Each entry point
 * below names the reference code it replaces (paths relative to the reference checkout).
 * The binding a maintainer of the reference would add is a ctypes stub: INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter is marked TD_HOST: an array the library reads on the host before it
 *     launches (its values, or the device pointers it holds, travel in the kernel arguments).  The macro expands to nothing; the
 *     ctypes binding reads it, and the numeric #defines below, from this file (tripled_amd/native.py: parse_header), so a
 *     prototype here IS its Python signature: scalars are int / float / double / long long, a pointer to pointers is always
 *     TD_HOST, a TD_HOST array of values has one of those four element types;
 *   - tensors are dense, NCHW, fp32, row-major (x fastest), exactly as the reference holds them -- except the colour
 *     frames of td_photo_fwd, which are RGBX pixels [B,H,W,4] produced from the reference's [B,3,H,W] tensors by
 *     td_photo_identity (as a by-product) or td_pack_rgbx (one 16-byte load per pixel or bilinear tap: the forward is bound
 *     by the number of memory instructions in flight, not by bytes); td_photo_identity and td_photo_bwd read the NCHW frames;
 *   - the caller owns every buffer; the library allocates nothing and keeps no global state;
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream); no call synchronises, so every call is legal inside hipGraph capture;
 *   - return value: TD_OK (0) or a negative TD_ERR_* code; nothing throws across the ABI;
 *   - n_src = number of non-reference frames (frame_ids[1:]), 1..TD_MAX_SRC;
 *   - candidate order of the min-reprojection is the reference's: identity terms for
 *     src 0..n_src-1 first (when automasking), then the warped terms for src 0..n_src-1.
 */
#ifndef TRIPLED_HIP_H
#define TRIPLED_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TD_ABI_VERSION 3      /* 3: fused bottleneck entry points (td_conv1x1_fwd_bnrelu, td_conv1x1_dgrad*, td_bn_*_partials); 2: td_photo_fwd takes RGBX frames (td_photo_identity emits them), idloss is [B,H,W,n_src], d_up has one plane per frame */
#define TD_MAX_SRC 4
#define TD_HOST               /* marks a parameter the library dereferences on the host (Conventions) */

#define TD_OK 0
#define TD_ERR_BAD_ARG (-1)      /* null pointer / non-positive size / n_src out of range */
#define TD_ERR_UNSUPPORTED (-2)  /* shape the kernels do not cover (e.g. H or W < 3)        */
#define TD_ERR_LAUNCH (-3)       /* hipGetLastError() != hipSuccess after the launch        */
#define TD_ERR_WORKSPACE (-4)    /* caller-provided workspace too small                     */

typedef void* td_stream_t;

int td_abi_version(void);
const char* td_error_string(int code);
/* Last HIP error text recorded by a failed launch on this thread ("" if none). */
const char* td_last_hip_error(void);

/* Number of thread blocks td_photo_fwd uses for a B x H x W problem (sizes `partial`), and
 * the number td_photo_bwd uses (sizes `dP_partial`; its tiles are smaller). */
int td_photo_num_blocks(int B, int H, int W);
int td_photo_bwd_num_blocks(int B, int H, int W);

/* [B,3,H,W] fp32 colour frame -> RGBX [B,H,W,4] (x = 0), the frame format of td_photo_fwd (when td_photo_identity does not run). */
int td_pack_rgbx(const float* img, int B, int H, int W, float* out, td_stream_t stream);

/*
 * Identity (auto-mask) photometric term, scale independent:
 *   idloss[b, i, y, x] = 0.85 * mean_c SSIM(src_i, tgt) + 0.15 * mean_c sqrt((tgt - src_i)^2 + 1e-6)
 * Replaces compute_reprojection_loss(inputs[("color", f, 0)], target) inside the automask loop,
 * mono/model/mono_fm_joint_inpaint/net.py:101-106 (SSIM: mono/model/mono_fm_joint/layers.py:85-107,
 * robust_l1 + weights: mono/model/mono_fm_joint/net.py:59-71).  The reference recomputes it per
 * scale; it does not depend on the scale, so it is computed once per step here.
 *   tgt     [B,3,H,W] (the reference's tensor)
 *   src     host array of n_src device pointers, each [B,3,H,W]
 *   idloss  [B,H,W,n_src] (out): the terms of a pixel are adjacent (td_photo_fwd reads them with one load)
 *   tgt_rgbx, src_rgbx (out, both or neither NULL): [B,H,W,4] RGBX copies of the frames (x = 0), the frame format of
 *           td_photo_fwd -- written from the pixels this kernel reads anyway, which saves the td_pack_rgbx passes
 */
int td_photo_identity(const float* tgt, TD_HOST const float* const* src, int n_src,
                      int B, int H, int W, float* idloss, float* tgt_rgbx, TD_HOST float* const* src_rgbx, td_stream_t stream);

/*
 * Fused per-scale photometric forward.  Replaces, for one scale,
 *   generate_images_pred            mono/model/mono_fm_joint/net.py:181-194
 *     F.interpolate(disp,[H,W],bilinear)            :183
 *     disp_to_depth                                 :157-162
 *     Backproject.forward                           mono/model/mono_fm_joint/layers.py:57-61
 *     Project.forward                               mono/model/mono_fm_joint/layers.py:73-82
 *     F.grid_sample(img, grid, padding_mode="border")  net.py:193  (bilinear, align_corners=False)
 *   compute_reprojection_loss (SSIM + robust L1)    mono/model/mono_fm_joint/net.py:67-71
 *   the automask + torch.cat + torch.min block      mono/model/mono_fm_joint_inpaint/net.py:101-117
 *
 *   tgt, src  RGBX frames [B,H,W,4] (from td_photo_identity's copies or td_pack_rgbx)
 *   disp      [B,1,hs,ws]  sigmoid disparity of this scale (any hs<=H, ws<=W)
 *   P         [n_src,B,3,4]  (K @ T_i)[:, :3, :]  -- formed by the caller (tiny matmul, keeps autograd to T)
 *   invK      [B,4,4]  (only the upper-left 3x3 block is read, as in the reference)
 *   idloss    [B,H,W,n_src] from td_photo_identity, or NULL to disable automasking
 *   noise     [n_src,B,H,W] standard-normal draws (scaled by 1e-5 inside, net.py:105) or NULL
 *   argmin    [B,H,W] uint8 (out): index into the candidate list (reference: int64 "min_index")
 *   warped    [n_src,B,3,H,W] (out, nullable): the warped sources, outputs[("color", f, s)]
 *   min_map   [B,H,W] (out, nullable): per-pixel minimum
 *   partial   [td_photo_num_blocks] (out): per-wave-task sums of the per-pixel minimum; the loss is
 *             sum(partial) / (B*H*W) / n_scales  (td_sum_scaled finishes it deterministically)
 *   coef      [B,9,H,W] (out, nullable; pass it when a backward will follow): per pixel p and channel c
 *             the SSIM-adjoint coefficients (alpha, beta, gamma) of the warped frame the arg-min selected
 *             (zeros where an identity term won), with  d SSIM_p / d x_q = (alpha + beta x_q + gamma y_q)/9
 *             for every member q of p's 3x3 window.
 */
int td_photo_fwd(const float* tgt, TD_HOST const float* const* src, int n_src,
                 const float* disp, const float* P, const float* invK,
                 const float* idloss, const float* noise,
                 int B, int H, int W, int hs, int ws,
                 float min_depth, float max_depth,
                 uint8_t* argmin, float* warped, float* min_map, float* partial, float* coef,
                 td_stream_t stream);

/*
 * Backward of td_photo_fwd w.r.t. disp and P (what autograd derives in the reference from the
 * same lines).  The warp is recomputed in-kernel; argmin and coef come from the forward.
 *   gscale    device scalar: d(total)/d(loss_s) as handed over by autograd
 *   inv_count 1 / (B*H*W*n_scales)  (the mean and the /len(scales) of net.py:117)
 *   d_up      [n_src,B,H,W] (out, workspace): gradient w.r.t. the UPSAMPLED disparity, one plane per source frame
 *             (the frames of a column strip are separate wave tasks; their sum is the gradient)
 *   dP_partial[td_photo_bwd_num_blocks, n_src*12] (out): per-block partial sums of dL/dP
 *   tgt, src  the NCHW frames [B,3,H,W]; tgt_rgbx, src_rgbx (both or neither NULL): their RGBX copies -- read instead of the
 *             NCHW frames at the finest scale (2*hs >= H), where the disparity's detail breaks the coalescing of dword gathers
 * Follow with td_upsample_adjoint_planes (d_up planes -> d_disp) and td_reduce_dP.
 */
int td_photo_bwd(const float* tgt, TD_HOST const float* const* src, const float* tgt_rgbx, TD_HOST const float* const* src_rgbx, int n_src,
                 const float* disp, const float* P, const float* invK,
                 const uint8_t* argmin, const float* coef, int automask,
                 const float* gscale, float inv_count,
                 int B, int H, int W, int hs, int ws,
                 float min_depth, float max_depth,
                 float* d_up, float* dP_partial, td_stream_t stream);

/* Adjoint of F.interpolate(..., [H,W], mode="bilinear", align_corners=False)
 * (mono/model/mono_fm_joint/net.py:183): d_up [B,H,W] -> d_disp [B,1,hs,ws].
 * accumulate != 0 adds into d_disp instead of overwriting it. Gather form, deterministic. */
int td_upsample_adjoint(const float* d_up, int B, int H, int W, int hs, int ws,
                        float* d_disp, int accumulate, td_stream_t stream);
/* The same adjoint of the SUM of n_planes gradient planes d_up [n_planes,B,H,W] (td_photo_bwd's per-frame planes), summed in
 * plane order while gathering. */
int td_upsample_adjoint_planes(const float* d_up, int n_planes, int B, int H, int W, int hs, int ws,
                               float* d_disp, int accumulate, td_stream_t stream);

/* dP[i,b,:,:] = sum over the blocks of sample b of dP_partial (deterministic tree). */
int td_reduce_dP(const float* dP_partial, int n_src, int B, int H, int W,
                 float* dP /* [n_src,B,3,4] */, td_stream_t stream);

/* out[0] = scale * sum(partial[0..n)) ; deterministic single-block tree. */
int td_sum_scaled(const float* partial, int n, float scale, float* out, td_stream_t stream);

/*
 * Area (box) down-sampling of the target frame: F.interpolate(img, (h, w), mode='area')
 * at mono/model/mono_fm_joint/net.py:283 and :311, for integer factors fy = H/h, fx = W/w.
 *   img [B,C,H,W] -> out [B,C,h,w]
 */
int td_area_downsample(const float* img, int B, int C, int H, int W, int h, int w,
                       float* out, td_stream_t stream);

/* Number of blocks td_smooth_fwd/bwd use for a B x h x w disparity. */
int td_smooth_num_blocks(int B, int h, int w);

/*
 * Edge-aware first + second order smoothness, forward.  Replaces
 *   disp mean-normalisation   mono/model/mono_fm_joint_inpaint/net.py:122-124
 *   get_smooth_loss + gradient  mono/model/mono_fm_joint/net.py:279-307
 * (the image is the area-resized target, see td_area_downsample).
 *   disp    [B,1,h,w]   img [B,3,h,w]
 *   normalize != 0 applies disp / (mean_hw(disp) + 1e-7) per sample first
 *   mean    [B] (out): per-sample mean of disp (saved for the backward)
 *   partial [td_smooth_num_blocks, 6] (out): per-block sums of the six terms
 *           (dx, dy, dxx, dxy, dyx, dyy); each term's mean uses its own element count.
 * Finish with td_smooth_finish.
 */
int td_smooth_fwd(const float* disp, const float* img, int B, int h, int w, int normalize,
                  float* mean, float* partial, td_stream_t stream);

/* loss[0] = weight * sum_k (sum_blocks partial[:,k]) / count_k   (count_k = elements of term k). */
int td_smooth_finish(const float* partial, int B, int h, int w, float weight, float* loss,
                     td_stream_t stream);

/*
 * Smoothness backward: d(loss)/d(disp) including the mean-normalisation.
 *   gscale device scalar upstream gradient; weight as in td_smooth_finish
 *   g_hat  [B,h,w] (workspace): gradient w.r.t. the normalised disparity
 *   dot_partial [td_smooth_num_blocks] (workspace): per-block sums of g_hat * disp
 *   d_disp [B,1,h,w] (out); accumulate != 0 adds into it.
 */
int td_smooth_bwd(const float* disp, const float* img, const float* mean,
                  int B, int h, int w, int normalize,
                  const float* gscale, float weight,
                  float* g_hat, float* dot_partial, float* d_disp, int accumulate,
                  td_stream_t stream);

/* Element types of the activation kernels below. */
#define TD_DTYPE_F32 0
#define TD_DTYPE_BF16 1

/*
 * nn.MaxPool2d(kernel_size=5, stride=1, padding=2) of the CRP blocks
 * (mono/model/mono_fm_joint/layers.py:208,213) on channels-last activations.
 *   in / out / grad_* : [N,H,W,C] (NHWC memory, i.e. a torch channels_last tensor), C % 8 == 0
 *   idx               : [N,H,W,C] uint8, window offset dy*5+dx of the selected element
 *                       (ATen's tie-break: first maximum in row-major order; NaN propagates)
 */
int td_maxpool5_fwd(const void* in, int dtype, int N, int H, int W, int C, void* out, uint8_t* idx,
                    td_stream_t stream);
int td_maxpool5_bwd(const void* grad_out, const uint8_t* idx, int dtype, int N, int H, int W, int C,
                    void* grad_in, td_stream_t stream);
/* The same with a tensor add [N,H,W,C] (nullable) summed into the result: grad_in = maxpool5_backward(grad_out) + add -- the gradient an
 * input of the CRP block's chain receives both through its pool and directly from the running sum (layers.py:200-215). */
int td_maxpool5_bwd_add(const void* grad_out, const uint8_t* idx, const void* add, int dtype, int N, int H, int W, int C,
                        void* grad_in, td_stream_t stream);

/*
 * The ResNet stem pool, nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (mono/model/mono_fm_joint/resnet.py:101),
 * same conventions as td_maxpool5_*: in [N,H,W,C] -> out / idx [N,Ho,Wo,C] with Ho = (H - 1) / 2 + 1,
 * idx = dy*3+dx of the selected element; H, W in td_maxpool3s2_bwd are the INPUT sizes.
 */
int td_maxpool3s2_fwd(const void* in, int dtype, int N, int H, int W, int C, void* out, uint8_t* idx,
                      td_stream_t stream);
int td_maxpool3s2_bwd(const void* grad_out, const uint8_t* idx, int dtype, int N, int H, int W, int C,
                      void* grad_in, td_stream_t stream);

/*
 * Channel concatenation of the DepthDecoder stages on channels-last activations
 * (mono/model/mono_fm_joint/depth_decoder.py:89-103, torch.cat((reduce(l), x, disp), 1)):
 *   out[pix, :] = [a[pix, :C0], b[pix, :C1], tail[pix, :C2], 0 ... 0]   with C0 + C1 + 8 output channels,
 *   C0 % 8 == C1 % 8 == 0, 1 <= C2 <= 8; all tensors [npix, C] row-major (NHWC), dtype f32 or bf16.
 * td_join_bwd writes the three slices of grad_out (the padding's gradient is dropped).
 */
int td_join_fwd(const void* a, const void* b, const void* tail, int dtype, long long npix, int C0, int C1, int C2,
                void* out, td_stream_t stream);
int td_join_bwd(const void* grad_out, int dtype, long long npix, int C0, int C1, int C2, void* grad_a, void* grad_b,
                void* grad_tail, td_stream_t stream);
/* The same with the middle operand `b_half` [N,H/2,W/2,C1] up-sampled x2 (nearest) on the fly: the DepthDecoder's
 * torch.cat((reduce(l), upsample(x), disp), 1) without materialising upsample(x) (depth_decoder.py:89-103; 189 MB at the
 * last stage of C2).  H, W even.  The backward sums the four output pixels of every low-resolution pixel. */
int td_join_up2_fwd(const void* a, const void* b_half, const void* tail, int dtype, int N, int H, int W, int C0, int C1,
                    int C2, void* out, td_stream_t stream);
int td_join_up2_bwd(const void* grad_out, int dtype, int N, int H, int W, int C0, int C1, int C2, void* grad_a,
                    void* grad_b_half, void* grad_tail, td_stream_t stream);

/*
 * Training-mode BatchNorm2d on channels-last activations with the residual add and ReLU of the ResNet
 * blocks fused in (mono/model/mono_fm_joint/resnet.py:30-49 BasicBlock.forward, :66-86
 * Bottleneck.forward; F.batch_norm(training=True) semantics: biased batch variance for the output,
 * unbiased for running_var, running = (1 - momentum) * running + momentum * batch).
 *
 *   x, residual, y, dy, dx, dresidual : [M, C] row-major (= NHWC with M = N*H*W), dtype f32 or bf16, C % 64 == 0
 *   gamma, beta, running_*, save_*, dgamma, dbeta : [C] f32 ; residual / running_* / dresidual may be NULL
 *   y = relu?( (x - mean) * invstd * gamma + beta [+ residual] )
 *   backward: g = dy * [y > 0] (relu; with y == NULL and no residual the mask is recomputed from x, gamma, beta,
 *             save_mean, save_invstd exactly as the forward formed it) ; dbeta = sum g ; dgamma = sum g * xhat ;
 *             dx = gamma * invstd * (g - dbeta / M - xhat * dgamma / M) ; dresidual = g
 *   groups: the M rows are `groups` consecutive equal ranges with separate batch statistics (save_mean /
 *           save_invstd are [groups, C]); the running statistics receive one momentum update per group, in
 *           order, and dgamma / dbeta are summed over the groups -- i.e. exactly `groups` separate calls on the
 *           stacked passes of one network over different frames (pose pairs, source-frame features).
 *   workspace: td_bn_workspace_floats(M, groups, C) floats (partial sums + coefficients; contents undefined on return).
 */
long long td_bn_workspace_floats(long long M, int groups, int C);
int td_bn_fwd(const void* x, const void* residual, int dtype, const float* gamma, const float* beta,
              float* running_mean, float* running_var, float momentum, float eps, int relu, long long M, int groups,
              int C, void* y, float* save_mean, float* save_invstd, float* workspace, td_stream_t stream);
int td_bn_bwd(const void* dy, const void* x, const void* y, int dtype, const float* gamma, const float* beta, const float* save_mean,
              const float* save_invstd, int relu, long long M, int groups, int C, void* dx, void* dresidual,
              float* dgamma, float* dbeta, float* workspace, td_stream_t stream);

/*
 * 1x1 convolution of the ResNet bottlenecks on channels-last bf16 activations as an MFMA GEMM
 * (v_mfma_f32_32x32x16_bf16, fp32 accumulation) whose epilogue forms the partial batch statistics of the
 * BatchNorm that follows it.  Replaces nn.Conv2d(kernel_size=1) + the statistics pass of nn.BatchNorm2d in
 * Bottleneck.forward (mono/model/mono_fm_joint/resnet.py:66-86: conv1 -> bn1, conv3 -> bn3) and in the strided
 * 1x1 down-sample branch (resnet.py:119-127).
 *   x [rows_in, K] bf16 (rows_in = M for stride 1; N_img*Hi*Wi for the strided form), w [N, K] bf16 (the [N,K,1,1] weight),
 *   y [M, N] bf16, M = output pixels; K % 64 == 0, N % 64 == 0; groups: M is `groups` consecutive equal row ranges with
 *   separate statistics (stacked passes, as td_bn_fwd).
 *   stat_partials (may be NULL): [groups, S, N, 2] f32 with S = td_conv1x1_stat_rows(M, groups, N): (sum y, sum y^2) over the
 *   rows of each row tile, of the bf16-rounded outputs -- the layout td_bn_fwd_from_partials consumes.
 * td_bn_fwd_from_partials: td_bn_fwd without its statistics pass: mean / invstd / running statistics from `partials`
 *   [groups, stat_rows, C, 2] (finished in the prologue of the apply kernel; the buffer is SCRATCH: more than 96 rows are first
 *   reduced in place), then y = relu?( (x - mean) * invstd * gamma + beta [+ residual] ).
 * td_conv1x1_wgrad: the weight gradient of the same convolution, dW[n, k] = sum_m dY[m, n] * X[src(m), k] (autograd of the
 *   Conv2d above), on the MFMA through transposed LDS reads (ds_read_b64_tr_b16); M is cut into row ranges whose fp32 partial
 *   tiles a second kernel adds in order (deterministic; dW in bf16 or f32: dw_dtype).
 *   workspace: td_conv1x1_wgrad_workspace_floats(M, K, N) floats.
 */
int td_conv1x1_stat_rows(long long M, int groups, int N);
int td_conv1x1_fwd(const void* x, const void* w, long long M, int groups, int K, int N, int Hi, int Wi, int stride, void* y,
                   float* stat_partials, td_stream_t stream);
/* 3x3 convolution (stride 1 or 2, padding 0 or 1) of the ResNet blocks and the decoders as an implicit MFMA GEMM: K = 9 * Cin
 * walked tap by tap over the channels-last input (the im2col matrix is never formed), same epilogue as td_conv1x1_fwd
 * (stat_partials: td_conv1x1_stat_rows(B*Ho*Wo, groups, N) row tiles; may be NULL).  Replaces conv2 (+ bn2's statistics pass)
 * of Bottleneck.forward and the convolutions of BasicBlock.forward (mono/model/mono_fm_joint/resnet.py:30-49, 66-86).
 *   x [B, Hi, Wi, Cin] bf16 channels-last, w [N, 3, 3, Cin] bf16 (the memory of a channels-last [N, Cin, 3, 3] weight),
 *   y [B, Ho, Wo, N] bf16; Cin % 8 == 0, N % 64 == 0. */
int td_conv3x3_fwd(const void* x, const void* w, int B, int groups, int Hi, int Wi, int Cin, int N, int stride, int pad, void* y,
                   float* stat_partials, td_stream_t stream);
/* Weight gradient of a 3x3 stride-1 convolution (zero padding `pad` = 1: conv2 of the ResNet blocks, mono/model/mono_fm_joint/resnet.py:
 * 30-49, 57-58; `pad` = 0 on a pre-padded input: Conv3x3 = ReflectionPad2d(1) + conv, mono/model/mono_fm_joint/layers.py:171-184):
 *   dW[n, ky, kx, c] = sum_(b,ho,wo) dY[b, ho, wo, n] * X[b, ho + ky - pad, wo + kx - pad, c]
 *   dy [B, Ho, Wo, N], x [B, Ho + 2 - 2 pad, Wo + 2 - 2 pad, C] bf16 channels-last; dw [N, 3, 3, C] (the memory of a channels-last
 *   [N, C, 3, 3] weight) in bf16 or f32 (dw_dtype); C % 64 == N % 64 == 0, Wo >= 20, Ho >= 4.
 * MFMA over the pixel index like td_conv1x1_wgrad, nine taps per staged tile, fp32 slabs per row range added in a fixed order
 * (deterministic; MIOpen's split-K kernels accumulate with atomics into a zero-filled fp32 workspace and cast afterwards).
 *   workspace: td_conv3x3_wgrad_workspace_floats(B, Ho, Wo, C, N) floats. */
long long td_conv3x3_wgrad_workspace_floats(int B, int Ho, int Wo, int C, int N);
int td_conv3x3_wgrad(const void* dy, const void* x, int B, int Ho, int Wo, int C, int N, int pad, int dw_dtype, void* dw,
                     float* workspace, td_stream_t stream);
long long td_conv1x1_wgrad_workspace_floats(long long M, int K, int N);
int td_conv1x1_wgrad(const void* dy, const void* x, long long M, int K, int N, int Hi, int Wi, int stride, int dw_dtype, void* dw,
                     float* workspace, td_stream_t stream);
/* n weight gradients in few launches: problem i == td_conv1x1_wgrad(dy[i], x[i], M[i], K[i], N[i], Hi[i], Wi[i], stride[i], dw_dtype[i],
 * dw[i], workspace[i]), bit for bit (same tiling / row ranges / summation order); all array arguments are HOST arrays of length n
 * (<= 4096).  A training step has ~90 independent 1x1 weight gradients that nothing needs before the optimiser step: enqueued by
 * the autograd nodes and launched together they stop being ~180 latency-bound launches (tripled_amd.ops.deferred_wgrads). */
int td_conv1x1_wgrad_group(int n, TD_HOST const void* const* dy, TD_HOST const void* const* x, TD_HOST const long long* M,
                           TD_HOST const int* K, TD_HOST const int* N, TD_HOST const int* Hi, TD_HOST const int* Wi,
                           TD_HOST const int* stride, TD_HOST const int* dw_dtype, TD_HOST void* const* dw,
                           TD_HOST float* const* workspace, td_stream_t stream);
int td_bn_fwd_from_partials(const void* x, const void* residual, int dtype, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, float momentum, float eps, int relu, long long M,
                            int groups, int C, float* partials, int stat_rows, void* y, float* save_mean,
                            float* save_invstd, td_stream_t stream);

/*
 * Bias + activation behind a convolution and its adjoint with the bias gradient, on channels-last activations [M, C] (f32 or bf16,
 * C % 8 == 0, C <= 256, 256 % (C / 8) == 0).  Replaces, around the decoders' convolutions (ConvBlock = Conv3x3 -> ELU,
 * mono/model/mono_fm_joint/layers.py:143-155; F.leaky_relu(iconv / merge), mono/model/mono_fm_joint/depth_decoder.py:89-103): the bias
 * add of the convolution, the activation, the activation's backward and the bias-gradient reduction of the convolution's backward.
 *   act: 0 none, 1 ELU(alpha = 1), 2 leaky ReLU(0.01);  bias [C] f32 or bf16 (bias_dtype; NULL = no bias)
 *   td_bias_act_fwd: a = act(y + bias)            (a may alias y)
 *   td_bias_act_bwd: gy = g * act'(a) (from the RESULT a; gy may alias g; act 0: gy is not written, dbias = column sums of g),
 *                    dbias [C] (nullable) = sum over rows of gy, deterministic; workspace: td_bias_act_workspace_floats(M, C) floats.
 */
long long td_bias_act_workspace_floats(long long M, int C);
int td_bias_act_fwd(const void* y, const void* bias, int bias_dtype, int dtype, long long M, int C, int act, void* a, td_stream_t stream);
int td_bias_act_bwd(const void* g, const void* a, int dtype, long long M, int C, int act, void* gy, void* dbias, int dbias_dtype,
                    float* workspace, td_stream_t stream);

/*
 * Optimiser step of a flat fp32 parameter buffer in one pass: the gradient scale of torch.nn.utils.clip_grad_norm_ (total_norm: device
 * scalar, the 2-norm of grad, or NULL for no clipping), torch.optim.Adam's update (weight_decay 0, no amsgrad; `step` = device scalar
 * holding the 1-based step count, lr from the device scalar lr_dev or, when NULL, lr_host) and the bf16 working copy of the first
 * n_lowp parameters.  Replaces optimizer_config.grad_clip + optimizer.step() of the training hook (mono/core/utils/dist_utils.py:54-60)
 * on the flat store of tripled_amd/flat_amp.py.  n % 4 == 0, n_lowp % 4 == 0.
 */
int td_adam_flat(float* w, const float* grad, float* exp_avg, float* exp_avg_sq, void* lowp, long long n, long long n_lowp,
                 const float* step, const float* lr_dev, float lr_host, double beta1, double beta2, float eps, const float* total_norm,
                 float max_norm, td_stream_t stream);

/*
 * flat[dst_offsets[i] + e] = (float) srcs[i][e] for e < numels[i], i < n; srcs[i] == NULL zero-fills the slot.  srcs / dst_offsets /
 * numels are HOST arrays (the pointers travel in the kernel arguments, 64 tensors per launch: legal under graph capture); all
 * sources have the dtype src_dtype (bf16 or f32).  The gradient gather of the flat parameter store (tripled_amd/flat_amp.py):
 * replaces torch.cat over the per-parameter gradients + the bf16 -> f32 pass.
 */
int td_gather_flat(TD_HOST const void* const* srcs, TD_HOST const long long* dst_offsets, TD_HOST const long long* numels, int n,
                   int src_dtype, float* flat, td_stream_t stream);

/*
 * Fused forms of the bottleneck's 1x1 convolutions (round 4): the BatchNorm passes of the NEIGHBOURING layers ride on the GEMM's
 * operand staging and epilogue instead of being separate passes over the activations.  Reference: Bottleneck.forward,
 * mono/model/mono_fm_joint/resnet.py:66-86 (conv1 -> bn1 -> relu -> conv2 -> bn2 -> relu -> conv3 -> bn3 -> += identity -> relu)
 * and what autograd derives from it.  All activations [M, C] bf16 row-major (channels-last), stride 1, channel counts % 64 == 0,
 * `groups` stacked passes with separate statistics as td_bn_fwd.
 *
 * td_bn_partial_rows / td_bn_fwd_partials / td_bn_bwd_partials: the statistics passes of td_bn_fwd / td_bn_bwd on their own:
 *   partials [groups, td_bn_partial_rows(M, groups, C), C, 2] f32 = per row range (sum x, sum x^2), resp. (sum g, sum g (x - mean))
 *   with g = dy masked by the ReLU exactly as td_bn_bwd does.  The buffer is SCRATCH for the consumer (reduced in place).
 * td_bn_bwd_from_partials: td_bn_bwd without its statistics pass (the sums come from td_conv1x1_dgrad_bnsums' epilogue).
 *
 * td_conv1x1_fwd_bnrelu: y = conv1x1(relu(bn(z)), w) where bn's batch statistics come from `in_partials` (in_rows rows per group, e.g.
 *   from td_bn_fwd_partials; finished in the GEMM's prologue, which also writes save_mean / save_invstd [groups, K] and updates the
 *   running statistics): conv3(relu(bn2(conv2 output))) of the bottleneck without the bn2 pass.  a_side (nullable) [M, K] receives
 *   relu(bn(z)) (the weight gradient of this convolution needs it); stat_partials as td_conv1x1_fwd.  K <= 512.
 * td_conv1x1_dgrad: dx[M, Cin] = dy[M, Cout] . w[Cout, Cin] (+ residual [M, Cin], added to the bf16-rounded product and rounded
 *   again: the tensor add autograd runs behind the data gradient for the block's identity branch).  The weight is read as the
 *   forward stores it (transposed LDS reads).
 * td_conv1x1_dgrad_bnsums: the same GEMM whose epilogue forms the backward sums of the BatchNorm that PRODUCED this convolution's
 *   input: out_partials [groups, td_conv1x1_stat_rows(M, groups, Cin), Cin, 2] = (sum g, sum g (z - mean)), g = dx * [bn(z) > 0],
 *   z [M, Cin] that BatchNorm's input (conv3's data gradient + bn2's backward statistics, no pass over dx for them).
 * td_conv1x1_dgrad_bnbwd: dx = BNbackward(g, z) . w (+ residual): the dy operand is formed while it is staged from the gradient g
 *   [M, Cout] of relu(bn(z)) and z [M, Cout] (dz = gamma invstd (g' - mean(g') - xhat mean(g' xhat)), g' = g [bn(z) > 0]); the sums
 *   come from in_partials (td_bn_bwd_partials), dgamma / dbeta [Cout] are written, dz_side (nullable) [M, Cout] receives dz for the
 *   weight gradient: conv1's data gradient straight from conv2's, without the bn1 dx pass and without the residual add.  Cout <= 512.
 */
int td_bn_partial_rows(long long M, int groups, int C);
int td_bn_fwd_partials(const void* x, int dtype, long long M, int groups, int C, float* partials, td_stream_t stream);
int td_bn_bwd_partials(const void* dy, const void* x, const void* y, int dtype, const float* gamma, const float* beta,
                       const float* save_mean, const float* save_invstd, int relu, long long M, int groups, int C, float* partials,
                       td_stream_t stream);
int td_bn_bwd_from_partials(const void* dy, const void* x, const void* y, int dtype, const float* gamma, const float* beta,
                            const float* save_mean, const float* save_invstd, int relu, long long M, int groups, int C,
                            float* partials, int stat_rows, void* dx, void* dresidual, float* dgamma, float* dbeta,
                            td_stream_t stream);
int td_conv1x1_fwd_bnrelu(const void* z, const void* w, long long M, int groups, int K, int N, float* in_partials, int in_rows,
                          const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                          float* save_mean, float* save_invstd, void* a_side, void* y, float* stat_partials, td_stream_t stream);
int td_conv1x1_dgrad(const void* dy, const void* w, long long M, int groups, int Cout, int Cin, const void* residual, void* dx,
                     td_stream_t stream);
/* y = conv1x1(x, w) [M, N] and run_out = run_in + y (both bf16 [M, N]; run_out rounded from the bf16 y + run_in, as the tensor add
 * would be): the pointwise convolution of a CRP stage with the block's running sum in its epilogue (layers.py:200-215). */
int td_conv1x1_fwd_sum(const void* x, const void* w, long long M, int K, int N, const void* run_in, void* y, void* run_out,
                       td_stream_t stream);
int td_conv1x1_dgrad_bnsums(const void* dy, const void* w, long long M, int groups, int Cout, int Cin, const void* z,
                            const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, void* dx,
                            float* out_partials, td_stream_t stream);
int td_conv1x1_dgrad_bnbwd(const void* g, const void* z, const void* w, long long M, int groups, int Cout, int Cin, float* in_partials,
                           int in_rows, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                           float* dgamma, float* dbeta, void* dz_side, const void* residual, void* dx, td_stream_t stream);

/*
 * The same normalisation with statistics synchronised over the data-parallel ranks (the reference trains with
 * syncbn=True: torch.nn.SyncBatchNorm.convert_sync_batchnorm, mono/apis/trainer.py:156-157).  The caller
 * all-reduces (SUM) the [groups, C, 2] per-channel sums and the row count between the two stages; everything
 * heavy stays in the kernels of td_bn_fwd / td_bn_bwd:
 *   td_bn_sync_fwd_sums   sums[g,c,:] = (sum x, sum x^2) over this rank's rows
 *   td_bn_sync_fwd_apply  mean / invstd / running statistics from the GLOBAL sums and `count` (device scalar:
 *                         global rows per group), then y as in td_bn_fwd
 *   td_bn_sync_bwd_sums   sums[g,c,:] = (sum g, sum g * (x - mean)),  g = dy masked by the ReLU
 *   td_bn_sync_bwd_dx     dgamma / dbeta from the LOCAL sums (the gradient all-reduce averages them like every
 *                         parameter gradient), dx from the GLOBAL sums; coef: [groups, C, 3] scratch
 *   workspace: td_bn_workspace_floats(M, groups, C) floats.
 */
int td_bn_sync_fwd_sums(const void* x, int dtype, long long M, int groups, int C, float* sums, float* workspace,
                        td_stream_t stream);
int td_bn_sync_fwd_apply(const void* x, const void* residual, int dtype, const float* sums, const float* count,
                         const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                         float eps, int relu, long long M, int groups, int C, void* y, float* save_mean,
                         float* save_invstd, td_stream_t stream);
int td_bn_sync_bwd_sums(const void* dy, const void* x, const void* y, int dtype, const float* gamma, const float* beta,
                        const float* save_mean, const float* save_invstd, int relu, long long M, int groups, int C,
                        float* sums, float* workspace, td_stream_t stream);
int td_bn_sync_bwd_dx(const void* dy, const void* x, const void* y, int dtype, const float* local_sums,
                      const float* global_sums, const float* count, const float* gamma, const float* beta,
                      const float* save_mean, const float* save_invstd, int relu, long long M, int groups, int C,
                      void* dx, void* dresidual, float* dgamma, float* dbeta, float* coef, td_stream_t stream);

/*
 * Edge-aware regulariser on C-channel feature maps: get_feature_regularization_loss,
 * mono/model/mono_fm_joint/net.py:309-330 (six stencil terms |d_k F| * exp(-a * mean_c |d_k I|)).
 *
 * td_edge_weights: Wt[b,k,y,x] = scale6[k] * exp(-a * mean_c |d_k img|), 0 where term k has no anchor
 *   at (y,x); k = dx, dy, dxx, dxy, dyx, dyy.  img [B,3,h,w] is the area-resized target; scale6 (HOST
 *   array) carries coefficient / element-count of each term, so that
 *       loss = sum over anchors, channels, k of |d_k F| * Wt
 * td_featreg_fwd: partial[td_featreg_num_blocks] per-block sums of that (finish with td_sum_scaled).
 * td_featreg_bwd: grad = gscale[0] * d loss / d feat, same dtype/layout as feat.
 *   feat: [B,h,w,C] channels-last memory, C % 8 == 0, dtype TD_DTYPE_F32 or TD_DTYPE_BF16.
 */
int td_edge_weights(const float* img, int B, int h, int w, float a, TD_HOST const float* scale6, float* Wt,
                    td_stream_t stream);
int td_featreg_num_blocks(int B, int h, int w, int C);
int td_featreg_fwd(const void* feat, int dtype, const float* Wt, int B, int h, int w, int C,
                   float* partial, td_stream_t stream);
int td_featreg_bwd(const void* feat, int dtype, const float* Wt, const float* gscale, int B, int h, int w,
                   int C, void* grad, td_stream_t stream);

/*
 * Masked photometric reconstruction term of the in-painting auto-encoder
 * (mono/model/mono_fm_joint_inpaint/net.py:80-91):
 *     S = sum_p hole[p] * (0.85 * mean_c SSIM_c(x, y)(p) + 0.15 * mean_c sqrt((y - x)^2 + 1e-6))
 *   x (prediction), y (target): [B,3,h,w] f32 planar; hole: [B,h,w] f32 per-pixel weight
 * td_recon_fwd: partial[td_recon_num_tasks] per-wave sums of S (finish with td_sum_scaled);
 * td_recon_bwd: dx = gscale[0] * dS/dx, [B,3,h,w].
 */
int td_recon_num_tasks(int B, int h, int w);
int td_recon_fwd(const float* x, const float* y, const float* hole, int B, int h, int w,
                 float* partial, td_stream_t stream);
int td_recon_bwd(const float* x, const float* y, const float* hole, const float* gscale, int B, int h,
                 int w, float* dx, td_stream_t stream);

/*
 * nn.ReflectionPad2d(1) in front of every decoder Conv3x3 (mono/model/mono_fm_joint/layers.py:171-184) on
 * channels-last activations: in [N,H,W,C] -> out [N,H+2,W+2,C]; the backward is the gather-form adjoint
 * (grad_out [N,H+2,W+2,C] -> grad_in [N,H,W,C]).  C % 8 == 0, H, W >= 2.
 */
int td_reflpad1_fwd(const void* in, int dtype, int N, int H, int W, int C, void* out, td_stream_t stream);
int td_reflpad1_bwd(const void* grad_out, int dtype, int N, int H, int W, int C, void* grad_in,
                    td_stream_t stream);

/*
 * out = ReflectionPad2d(1)(F.interpolate(in, scale_factor=2, mode="nearest")) without materialising the
 * up-sampled tensor: the `iconv(upsample(upconv(x)))` step of the image decoders
 * (mono/model/mono_fm_joint/decoder.py:40-57).  in [N,H,W,C], out [N,2H+2,2W+2,C], channels-last, C % 8 == 0.
 * td_up2_reflpad1_bwd is the exact adjoint (gather form, <= 16 taps at a corner, 4 in the interior).
 */
int td_up2_reflpad1_fwd(const void* in, int dtype, int N, int H, int W, int C, void* out, td_stream_t stream);
int td_up2_reflpad1_bwd(const void* grad_out, int dtype, int N, int H, int W, int C, void* grad_in,
                        td_stream_t stream);

/*
 * Feature-metric term: generate_features_pred (mono/model/mono_fm_joint/net.py:196-223) +
 * compute_perceptional_loss (:63-65) + min over source frames (mono_fm_joint_inpaint/net.py:58-70), fused.
 *   tgt, src[i]  [B,h,w,C] channels-last feature maps (C % 64 == 0; dtype f32 or bf16); n_src <= 2
 *   disp         [B,1,hs,ws]; P [n_src,B,3,4] and invK [B,4,4] at FEATURE resolution (K rows 0,1 halved)
 *   argmin       [B,h,w] uint8 (out: which source frame gives the minimum)
 *   partial      [td_featwarp_num_blocks] per-block sums of min_f mean_c sqrt((tgt - warp_f)^2 + 1e-6)
 * Backward (gradient of gscale[0] * inv_count * sum(partial)):
 *   d_tgt [B,h,w,C] (feature dtype), d_src[i] [B,h,w,C] int32 fixed-point accumulators -- MUST be zero-filled by the caller; the
 *   scatter adds contributions rounded to multiples of |gscale| * inv_count / C / 2^14 with integer atomics (order-independent,
 *   bit-reproducible); td_featwarp_dsrc_finish turns them into the gradient in the feature dtype --,
 *   d_up [B,h,w] (w.r.t. the up-sampled disparity; td_upsample_adjoint),
 *   dP_partial [td_featwarp_num_blocks, n_src*12] (td_reduce_partials with blocks_per_sample =
 *   td_featwarp_num_blocks / B).
 */
int td_featwarp_num_blocks(int B, int h, int w);
int td_featwarp_fwd(const void* tgt, TD_HOST const void* const* src, int n_src, int dtype, const float* disp,
                    const float* P, const float* invK, int B, int h, int w, int C, int hs, int ws,
                    float min_depth, float max_depth, uint8_t* argmin, float* partial, td_stream_t stream);
int td_featwarp_bwd(const void* tgt, TD_HOST const void* const* src, int n_src, int dtype, const float* disp,
                    const float* P, const float* invK, const uint8_t* argmin, const float* gscale,
                    float inv_count, int B, int h, int w, int C, int hs, int ws, float min_depth,
                    float max_depth, void* d_tgt, TD_HOST int* const* d_src, float* d_up, float* dP_partial,
                    td_stream_t stream);
/* out[i] = acc[i] * |gscale[0]| * inv_count / C / 2^14 (n elements, n % 8 == 0; dtype f32 or bf16): the scatter's accumulators
 * -> d/d(source features). */
int td_featwarp_dsrc_finish(const int* acc, const float* gscale, float inv_count, int C, long long n, int dtype, void* out,
                            td_stream_t stream);
/* dP[i,b,:] = sum over the blocks_per_sample consecutive rows of partial[., n_src*12] that belong to sample b. */
int td_reduce_partials(const float* partial, int n_src, int B, int blocks_per_sample, float* dP,
                       td_stream_t stream);

/*
 * Robust-L1 channel-mean map between a network output and an image, and its adjoint:
 *   out[b,y,x] = weight * mean_c sqrt((pred[b,c,y,x] - target[b,c,y,x])^2 + 1e-6)
 * Replaces compute_perceptional_loss on images -- compute_auto_res_loss,
 * mono/model/mono_fm_joint_inpaint/net.py:520-527 (a per-pixel MAP that batch_processor's mean reduces), and
 * compute_colorization_loss, :310-323 -- with robust_l1 of mono/model/mono_fm_joint/net.py:59-65.
 *   pred          C-channel tensor of dtype TD_DTYPE_F32 / TD_DTYPE_BF16 with arbitrary element strides
 *   pred_strides  HOST array of 4 element strides (n, c, h, w): channels-last decoder outputs and channel
 *                 slices are read in place, no .float()/.contiguous() copy
 *   target        [B,C,H,W] fp32 NCHW;  out [B,1,H,W] fp32
 * td_l1map_bwd: dpred (same dtype and strides as pred) = gmap[b,y,x] * weight / C * (pred - target) / sqrt(...).
 */
int td_l1map_fwd(const void* pred, int dtype, TD_HOST const long long* pred_strides, const float* target, int B, int C,
                 int H, int W, float weight, float* out, td_stream_t stream);
int td_l1map_bwd(const void* pred, int dtype, TD_HOST const long long* pred_strides, const float* target,
                 const float* gmap, int B, int C, int H, int W, float weight, void* dpred, td_stream_t stream);

/*
 * sRGB -> normalised CIE Lab: rgb2lab, mono/model/mono_fm_joint_inpaint/color_conversions.py:106-114 (rgb2xyz
 * :6-27, xyz2lab :52-75), called on the target frame by the colourisation models (net.py:236,292).
 *   rgb [B,3,H,W] fp32 in [0,1];  lab [B,3,H,W] = ((L - l_cent) / l_norm, a / ab_norm, b / ab_norm).
 * No gradient (the input is data).
 */
int td_rgb2lab(const float* rgb, int B, int H, int W, float l_cent, float l_norm, float ab_norm, float* lab,
               td_stream_t stream);

/*
 * Pose vectors -> camera transforms -> projection matrices for all frame pairs of a step in one launch.
 * Replaces transformation_from_parameters / rot_from_axisangle / get_translation_matrix,
 * mono/model/mono_fm_joint/net.py:225-277, and torch.matmul(K, T)[:, :3, :] of Project.forward,
 * mono/model/mono_fm_joint/layers.py:73-75.
 *   axisangle, translation  [n_pairs*B, 3] (PoseDecoder outputs, pair-major)
 *   invert                  HOST array of n_pairs flags (frame id < 0: M = R^T Trans(-t), else Trans(t) R)
 *   K                       [B,4,4] intrinsics (may be NULL when P is NULL)
 *   T   [n_pairs,B,4,4] (out)     P  [n_pairs,B,3,4] = (K @ T)[:, :3, :] (out, may be NULL)
 * td_pose_bwd: g_axisangle / g_translation [n_pairs*B,3] from gT and/or gP (either may be NULL, not both).
 */
int td_pose_fwd(const float* axisangle, const float* translation, TD_HOST const int* invert, const float* K,
                int n_pairs, int B, float* T, float* P, td_stream_t stream);
int td_pose_bwd(const float* axisangle, const float* translation, TD_HOST const int* invert, const float* K,
                int n_pairs, int B, const float* gT, const float* gP, float* g_axisangle,
                float* g_translation, td_stream_t stream);

/*
 * Input expansion on the device: uint8 frames -> float images + their colour-jittered copies.  Replaces ToTensor and
 * ColorJitter per frame on the host (MonoDataset.preprocess, mono/datasets/mono_dataset.py:83-101; parameters drawn at
 * :146-152) and the float32 upload of both copies (change_input_variable, mono/apis/trainer.py:19-29).
 *   frames_u8  [N,3,H,W] uint8 (N = frames x samples)
 *   aug        [N,9] float: (enabled, op0..op3, brightness, contrast, saturation, hue); ops 0..3 = brightness, contrast,
 *              saturation, hue, applied in the listed order (torchvision ColorJitter's float formulas)
 *   means_scratch [N] floats;  color, color_aug [N,3,H,W] float32 in [0,1] (out)
 */
int td_color_jitter(const uint8_t* frames_u8, const float* aug, int N, int H, int W, float* means_scratch, float* color,
                    float* color_aug, td_stream_t stream);

/*
 * Per-tensor fp8 quantisation (OCP e4m3fn, saturating) for the fp8 1x1-convolution path (BASELINE config 5).  The
 * reference has no reduced-precision path (it trains in fp32: mono/apis/trainer.py:147-189); the 1x1 convolutions this
 * serves are resnet.py:52-86 (Bottleneck conv1/conv3, downsample) and layers.py:110-118 (Conv1x1).
 *   td_fp8_amax_partials  partials[td_fp8_num_blocks(n)] = per-block max |x|
 *   td_fp8_quantize       q[i] = e4m3(x[i] * 448 / amax), inv_scale[0] = amax / 448  (amax = max of the partials; the
 *                         product  q_a . q_b * inv_scale_a * inv_scale_b  is the de-quantised GEMM result)
 *   x: n elements of dtype TD_DTYPE_F32 / TD_DTYPE_BF16, n % 8 == 0.
 */
int td_fp8_num_blocks(long long n);
int td_fp8_amax_partials(const void* x, int dtype, long long n, float* partials, td_stream_t stream);
int td_fp8_quantize(const void* x, int dtype, long long n, const float* partials, uint8_t* q, float* inv_scale,
                    td_stream_t stream);

/*
 * Depth inference around the network forward (csrc/td_infer.hip).  Both resizes are ATen's upsample_bilinear2d with
 * align_corners=False in float32: scale = (float)n_in / n_out, src = max(scale * (dst + 0.5f) - 0.5f, 0), i0 = (int)src,
 * i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1, value = l0y (l0x p00 + l1x p01) + l1y (l0x p10 + l1x p11).
 *
 * td_infer_preprocess: image -> network input.  Replaces transform(), scripts/infer.py:25-30 (astype(float32), permute,
 * F.interpolate(bilinear), /= 255), and -- with mirror = 1 -- the flipped second pass of the flip post-processing.
 *   img_u8 [B,H0,W0,3] uint8, interleaved RGB;  out [B*(1+mirror),3,h,w] float32 (out)
 *   mirror = 1: out[B+n,:,y,x] = out[n,:,y,w-1-x]
 *
 * td_disp_postprocess: network disparity -> full-size disparity and depth in one launch.  Replaces predict(),
 * scripts/infer.py:41-46 (F.interpolate to the image size, depth = SCALE / (disp * max_disp + min_disp)) and
 * batch_post_process_disparity, scripts/eval_depth_pp.py:22-28.
 *   disp [B*(1+paired),1,h,w], dtype TD_DTYPE_F32 / TD_DTYPE_BF16
 *   paired = 1: every bilinear tap is  r_mask l + l_mask r + (1 - l_mask - r_mask) 0.5 (l + r)  with l = disp[n,0,y,x],
 *               r = disp[B+n,0,y,w-1-x], l_mask(x) = 1 - clip(20 (x / (w-1) - 0.05), 0, 1), r_mask(x) = l_mask(w-1-x)  (w >= 2)
 *   disp_out [B,H0,W0] (out);  depth_out [B,H0,W0] = depth_scale / (a * disp_out + b) (out, may be NULL)
 *   scripts/infer.py: a = 1/1e-3, b = 1/80, depth_scale = 36;  disp_to_depth(., 0.1, 100): a = 1/0.1 - 1/100, b = 1/100, 1.
 *
 * td_colorize: value -> colour through a 256-entry table.  Replaces plt.imsave(path, disp, cmap='magma',
 * vmax=np.percentile(disp, 95)), scripts/infer.py:65-66 (the caller computes vmin / vmax).
 *   x [B,n] float32;  vmin, vmax [B] (device);  lut [256,3] uint8 (device);  out [B,n,3] uint8 (out)
 *   index = clamp((int)floorf(((x - vmin) / (vmax - vmin)) * 256.f), 0, 255), every step a rounded float32 operation.
 */
int td_infer_preprocess(const uint8_t* img_u8, int B, int H0, int W0, int h, int w, int mirror, float* out,
                        td_stream_t stream);
int td_disp_postprocess(const void* disp, int dtype, int B, int h, int w, int paired, int H0, int W0, float a, float b,
                        float depth_scale, float* disp_out, float* depth_out, td_stream_t stream);
int td_colorize(const float* x, int B, long long n, const float* vmin, const float* vmax, const uint8_t* lut, uint8_t* out,
                td_stream_t stream);

/*
 * KITTI depth evaluation of a batch on the device (csrc/td_eval.hip).  Replaces, per image, the protocol of
 * scripts/eval_depth.py:73-101 = mono/core/evaluation/eval_hooks.py:225-262 (cv2.resize of the scaled disparity to the
 * ground-truth size, 1 / ., mask min < gt < max inside the Garg crop, np.median ratio (x 36 for stereo), clip, compute_errors).
 *
 * td_eval_depth: 10 launches whatever B is, no synchronisation, no copy to the host, no allocation.
 *   disp [B,h,w], dtype TD_DTYPE_F32 / TD_DTYPE_BF16: the sigmoid disparity;  scaled = b + a * disp (float32; disp_to_depth(.,
 *        0.1, 100): a = 9.99, b = 0.01; (1, 0) for an already scaled disparity)
 *   gt [B,Hmax,Wmax] float32: image i occupies the top-left sizes[i] = (gt_h, gt_w); the padding never enters
 *   sizes [B,2] int32 (device);  crops [B,4] int32 (device): (y0, y1, x0, x1), half-open, computed by the caller in float64 as
 *        the host path does (np.array([0.40810811 gt_h, 0.99189189 gt_h, 0.03594771 gt_w, 0.96405229 gt_w]).astype(int32))
 *   resize: source coordinate (q + 0.5) * (n_in / n_out) - 0.5 in double, floor, both taps clipped to the border; the affine is
 *        applied to the four taps, the interpolation (rows, then columns) is float32
 *   pred = 1 / resized;  N = pixels in the mask;  scale = median(gt) / median(pred), np.median's of the float32 values (even N:
 *        0.5f * (lower + upper));  pred *= stereo ? TD_STEREO_SCALE_FACTOR : scale;  clip to [min_depth, max_depth]
 *   metrics [B,8] (out): abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, scale;  counts [B] int32 (out): N.  N = 0: a NaN row.
 *   workspace: td_eval_depth_workspace_bytes(B, Hmax, Wmax) bytes, 8-byte aligned (TD_ERR_WORKSPACE if workspace_bytes is less)
 *   Sums are accumulated in double per block and added in a fixed order; the select uses integer atomics only: two calls on the
 *   same inputs return the same bits.
 *
 * td_masked_median: the exact select on its own.  values [B,n] float32, an entry <= 0 (or NaN) is absent;
 *   median [B] (out) = np.median of the row's present entries (NaN if none), count [B] int32 (out);
 *   workspace: td_masked_median_workspace_bytes(B) bytes, 4-byte aligned.
 */
#define TD_STEREO_SCALE_FACTOR 36
long long td_eval_depth_workspace_bytes(int B, int Hmax, int Wmax);
int td_eval_depth(const void* disp, int dtype, int B, int h, int w, float a, float b, const float* gt, int Hmax, int Wmax,
                  const int* sizes, const int* crops, float min_depth, float max_depth, int stereo, void* workspace,
                  long long workspace_bytes, float* metrics, int* counts, td_stream_t stream);
long long td_masked_median_workspace_bytes(int B);
int td_masked_median(const float* values, int B, long long n, void* workspace, long long workspace_bytes, float* median,
                     int* count, td_stream_t stream);

/*
 * KITTI odometry evaluation on the device (csrc/td_odom.hip).  All pose arithmetic is float64 (float32 inputs are widened
 * exactly), sums have a fixed order and there are no floating-point atomics: two calls on the same inputs return the same bits.
 *
 * td_pose_pairs_u8: the pose network's input.  Replaces torch.cat([inputs[("color_aug", i, 0)] for i in [0, 1]], 1) on ToTensor
 * frames, scripts/eval_pose.py:59 (= scripts/draw_odometry.py:69), without decoding or uploading any frame twice.
 *   frames [n+1,3,H,W] uint8 (device);  pair i = cat(frame i, frame i+1) along the channels, each byte float(b) / 255 (a float32
 *   division), stored as dtype TD_DTYPE_F32 / TD_DTYPE_BF16 (round to nearest even).  Pairs [first, first+count) are written to
 *   rows out_first .. out_first+count-1 of out [.,6,H,W]: out_first = first fills a window of the full [n,6,H,W] array,
 *   out_first = 0 a batch buffer.  8 bytes per thread where 3 H W is a multiple of 8 (and the bases are aligned), else scalar.
 *
 * td_odom_trajectory: relative transforms -> global poses.  Replaces the loop global_pose = global_pose @ np.linalg.inv(g),
 * scripts/draw_odometry.py:62-74.
 *   rel [n,4,4] float32 (rel_f64 = 0) or float64 (1): frame k+1 -> frame k;  poses [n+1,3,4] float64 (out): G_0 = I,
 *   G_{k+1} = G_k inv(M_k), inv = the affine inverse (3x3 by cofactors, -A^-1 t), not the transpose.  One workgroup: every thread
 *   composes a contiguous chunk in order, an LDS scan of the chunk totals keeps left-to-right order.  Any n >= 1.
 *
 * td_odom_snippet_ate: replaces scripts/eval_pose.py:66-80 with dump_xyz and compute_ate, mono/datasets/utils.py:105-122.
 *   rel as above (the PREDICTED relative transforms);  gt_poses [n+1,3,4] float64;  track_length 2..16 (the reference: 5)
 *   ates [n] float64 (out): snippet i covers transforms i .. min(i + track_length - 1, n) - 1; gt local transforms are
 *   inv(inv(G_{k}) G_{k+1}); positions are cumulative products of the transforms themselves; the least-squares scale
 *   sum(gt * pred) / sum(pred^2) (0 / 0 = NaN); sqrt(sum err^2) / (the snippet's own point count).  One thread per snippet.
 *
 * td_odom_sequence_errors: replaces kittiOdomEval.eval's core, mono/tools/kitti_evaluation_toolkit.py:109-182 (trajectoryDistances,
 * lastFrameFromSegmentLength, calcSequenceErrors) and align_trajectory(correct_only_scale=True), mono/tools/trajectory.py:367-402
 * with geometry.umeyama_alignment, mono/tools/geometry.py:20-67.
 *   gt_poses, pred_poses [m,3,4] float64;  lengths: HOST array of n_lengths <= 16 positive segment lengths;  step: first frames
 *   are 0, step, 2 step, ... (F = ceil(m / step) of them)
 *   align_scale = 1: c = trace(diag(d) S) / sigma_x of the predicted against the ground-truth positions (singular values of the
 *        3x3 covariance by one-sided Jacobi, fixed sweep count; S's last entry = sign(det(cov))) scales the predicted translations
 *   dist [m] float64 (out / workspace): cumulative ground-truth distance, accumulated sequentially in index order
 *   rows [F,n_lengths,5] float64 (out): first_frame, r_err / len, t_err / len, len, speed;  valid [F,n_lengths] uint8 (out): 0 where
 *        no frame lies more than len beyond first_frame (the row's errors and speed are then NaN)
 *   summary [2] float64 (out): c (1 without align_scale), total ground-truth distance
 */
#define TD_ODOM_THREADS 256          /* the workgroup of td_odom_trajectory: a thread composes ceil(n / 256) transforms */
#define TD_ODOM_MAX_LENGTHS 16       /* td_odom_sequence_errors: the most segment lengths of one call */
int td_pose_pairs_u8(const uint8_t* frames, int n, int H, int W, int first, int count, int dtype, void* out, long long out_first,
                     td_stream_t stream);
int td_odom_trajectory(const void* rel, int rel_f64, int n, double* poses, td_stream_t stream);
int td_odom_snippet_ate(const void* rel, int rel_f64, const double* gt_poses, int n, int track_length, double* ates,
                        td_stream_t stream);
int td_odom_sequence_errors(const double* gt_poses, const double* pred_poses, int m, TD_HOST const double* lengths, int n_lengths, int step,
                            int align_scale, double* dist, double* rows, uint8_t* valid, double* summary, td_stream_t stream);

/*
 * Resize and flip of uint8 frames on the device, bit-equal to Pillow's Image.resize((W, H), LANCZOS) after
 * Image.transpose(FLIP_LEFT_RIGHT) (csrc/td_resize.hip).  Replaces MonoDataset's per-frame resize and flip in the loader workers,
 * mono/datasets/mono_dataset.py:60-63,129-143, for the "raw_u8" wire format.  One launch, no synchronisation, no allocation.
 *   src [N,3,Hc,Wc] uint8 (4-byte aligned): image n occupies the top-left (h, w) of its canvas, the size its size index names;
 *        no byte outside that region enters a result
 *   meta [N,2] int32 (device): (size index, flip).  An index outside [0, n_sizes) zero-fills that image and sets status[0] = 1.
 *   meta_host: the same array on the host, or NULL; when given, an index out of range is TD_ERR_BAD_ARG before any launch
 *   tables: int32 device buffer of table_ints ints;  desc: HOST int32 [n_sizes,8] = (h, w, ksx, ksy, off_kx, off_bx, off_ky, off_by),
 *        offsets in ints into tables: horizontal coefficients TRANSPOSED [ksx,W], horizontal bounds [W,2] = (first, count),
 *        vertical coefficients [H,ksy], vertical bounds [H,2]; 22-bit fixed point, |k| < 2^23 (tripled_amd/resize.py: LanczosBank)
 *   a pass:  out = clamp((2^21 + sum_t k[t] * pixel[first + t]) >> 22, 0, 255), int32; horizontal (reading column w - 1 - (first + t)
 *        with flip), a uint8 intermediate, then vertical
 *   dst [N,3,H,W] uint8 (out);  status [1] int32 (device): written only on a bad index (1) or tables that do not fit the sizes (2)
 *        (3: td_lanczos_resize_u8_indexed, below)
 *   TD_ERR_BAD_ARG: n_sizes outside 1..16, a size larger than the canvas, offsets outside the buffer, a bad index in meta_host.
 *   TD_ERR_UNSUPPORTED: rows too wide for the LDS tile, N > 65535, a misaligned src.
 */
#define TD_RESIZE_MAX_SIZES 16       /* the most sizes of one bank (n_sizes, the rows of desc) */
int td_lanczos_resize_u8(const uint8_t* src, const int* meta, TD_HOST const int* meta_host, const int* tables, long long table_ints,
                         TD_HOST const int* desc, int n_sizes, int N, int Hc, int Wc, int H, int W, uint8_t* dst, int* status,
                         td_stream_t stream);

/*
 * The same resize and flip with the sources fetched from a byte store resident in device memory (the "resident" wire format,
 * tripled_amd/resident.py): image n is planar uint8 [3,h,w] at byte offsets[n] of the store, rows tight (stride w), (h, w) the size
 * its size index names.  Arithmetic, tables, dst and the meaning of meta, meta_host, tables, desc are those of the call above.
 *   store: store_bytes bytes (4-byte aligned base); the offsets themselves may have any alignment
 *   offsets [N] int64 (device).  An offset that is negative or with offset + 3 h w > store_bytes zero-fills that image and sets
 *        status[0] = 3; no byte outside [store, store + store_bytes) is ever read
 *   offsets_host: the same array on the host, or NULL; when given, such an offset is TD_ERR_BAD_ARG before any launch (checked against
 *        the frame's own size when meta_host is given too, against the smallest size of the bank otherwise)
 *   TD_ERR_UNSUPPORTED: rows of the widest size too wide for the LDS tile, N > 65535, a misaligned store.
 */
int td_lanczos_resize_u8_indexed(const uint8_t* store, long long store_bytes, const long long* offsets,
                                 TD_HOST const long long* offsets_host, const int* meta, TD_HOST const int* meta_host, const int* tables,
                                 long long table_ints, TD_HOST const int* desc, int n_sizes, int N, int H, int W, uint8_t* dst,
                                 int* status, td_stream_t stream);

/*
 * Fusion of depth maps and camera poses into a voxel-averaged coloured point cloud (csrc/td_cloud.hip, tripled_amd/cloud.py).
 * Store, sort, then sum per destination: td_cloud_keys stores a (key, payload) pair per pixel, the caller sorts the keys
 * (torch.sort), td_cloud_heads marks where a voxel's run starts (the caller's torch.cumsum of the marks numbers the runs),
 * td_cloud_reduce_* sums every run into its voxel's row and td_cloud_finish turns rows into points.  Everything accumulated is an
 * integer: results are bit-identical from run to run and do not depend on how a sequence is cut into batches.  No kernel waits
 * on another workgroup.  An empty input (B, N or V = 0) is a successful no-op without a launch.  Offsets are 64-bit.
 *
 * td_cloud_keys.  depth [B,H,W] float32;  color [B,3,H,W] uint8 (planar);  poses [B,3,4] float64, camera-to-world (device);
 *   inv_K: HOST array, the nine float64 entries of the 3x3 block;  inv_voxel = 1 / voxel, computed once by the caller.
 *   float64 throughout, every product and sum rounded on its own (pixel (u, v) at integer coordinates, no half-pixel offset):
 *     ray_k = (m_k0 u + m_k1 v) + m_k2;  p = (depth depth_scale) ray;  world_k = ((r_k0 p_x + r_k1 p_y) + r_k2 p_z) + pose_scale t_k;
 *     g = world inv_voxel;  i = floor(g);  q = min(1023, (int)floor((g - i) 1024.0))
 *   a pixel is invalid, by the first cause that holds: (1) x or y is no multiple of stride; (2) it lies within border pixels of
 *   an image edge; (3) its depth is not finite or depth depth_scale is outside [min_depth, max_range]; (4) edge > 0 and for a
 *   4-neighbour inside the image the neighbour is not finite or |d - d_nb| > edge min(d, d_nb) (float32, unscaled); (5) a voxel
 *   coordinate is outside [-2^20, 2^20), or the key would equal the sentinel (the one voxel with all three coordinates 2^20 - 1)
 *   key [B H W] int64 (out): ((ix + 2^20) << 42) | ((iy + 2^20) << 21) | (iz + 2^20); INT64_MAX for an invalid pixel
 *   payload [B H W] uint64 (out): qx | qy << 10 | qz << 20 | r << 30 | g << 38 | b << 46; 0 for an invalid pixel
 *   stats [6] int64 (device) or NULL: incremented by the numbers of valid pixels and of pixels invalid by causes 1 ... 5
 *   A thread owns 4, 2 or 1 consecutive columns of a row: the widest that divides W and that the base pointers are aligned for.
 *
 * td_cloud_heads.  keys [N] int64, sorted ascending;  flags [N] int32 (out): 1 where the key is valid and differs from its
 *   predecessor.  seg = the inclusive cumulative sum of flags (int64): element i belongs to row seg[i] - 1, and seg[N-1] = V.
 *
 * td_cloud_reduce_packed / td_cloud_reduce_rows.  keys, seg [N] as above;  perm [N] int64 or NULL (identity): the source index of
 *   sorted element i (the sort's permutation; the gather is part of the kernel);  payload [n_src] uint64 as td_cloud_keys wrote it
 *   (one point per element: count 1), or rows [n_src,7] int64 already-summed rows;  out_keys [V] int64 (out): the key of every
 *   row;  sums [V,7] int64, ZERO-INITIALISED by the caller (out): count, sum qx, sum qy, sum qz, sum r, sum g, sum b.
 *   A wave reduces the runs inside its own stretch of 512 elements in registers; a run wholly inside the stretch is written with
 *   plain stores, the first and last run of a stretch, which may continue in a neighbour's, with 64-bit integer atomics.
 *   Elements whose seg is outside 1 ... V or whose source index is outside [0, n_src) write and read nothing.
 *
 * td_cloud_finish.  keys [V], sums [V,7] -> xyz [V,3] float32 = (float)(((double)i + ((double)sum_q / (double)count + 0.5) / 1024.0)
 *   voxel);  rgb [V,3] uint8 = (2 sum_c + count) / (2 count), integer;  count [V] int32, saturating;  keep [V] uint8 = count >= min_count.
 */
int td_cloud_keys(const float* depth, const uint8_t* color, const double* poses, TD_HOST const double* inv_K, int B, int H, int W,
                  double depth_scale, double pose_scale, double inv_voxel, int stride, int border, double min_depth, double max_range,
                  float edge, long long* key, unsigned long long* payload, long long* stats, td_stream_t stream);
int td_cloud_heads(const long long* keys, long long N, int* flags, td_stream_t stream);
int td_cloud_reduce_packed(const long long* keys, const long long* seg, const long long* perm, const unsigned long long* payload,
                           long long n_src, long long N, long long V, long long* out_keys, long long* sums, td_stream_t stream);
int td_cloud_reduce_rows(const long long* keys, const long long* seg, const long long* perm, const long long* rows, long long n_src,
                         long long N, long long V, long long* out_keys, long long* sums, td_stream_t stream);
int td_cloud_finish(const long long* keys, const long long* sums, long long V, double voxel, long long min_count, float* xyz,
                    uint8_t* rgb, int* count, uint8_t* keep, td_stream_t stream);

/*
 * Multi-view consistency of a sequence's depth maps (csrc/td_views.hip).  The reference has no such program: the statement is
 * tripled_amd/cloud.py:views_numpy, which the kernel equals bit for bit.  For every pixel of the centre frames c0 ... c1-1, the
 * number of neighbouring frames that, reprojected, see the same depth there.  One launch, plain stores, no synchronisation.
 *
 * td_cloud_views.  depth [N,H,W] float32, the whole window;  poses [N,3,4] float64, camera-to-world (device);  K, inv_K: HOST arrays,
 *   the nine float64 entries of the 3x3 blocks.  The neighbours of centre i are the 2 radius other frames of a .. a + 2 radius,
 *   a = min(max(i - radius, lo), hi - 1 - 2 radius): the window is shifted, not shortened, at the ends of [lo, hi).
 *   float64 throughout, every product, sum and quotient rounded on its own (R, t: a pose's rotation and translation):
 *     ok_f = isfinite(d_f) and min_depth <= ds_f <= max_range,  ds_f = (double)d_f depth_scale
 *     ray_k = (m_k0 u + m_k1 v) + m_k2;  p = ds_i ray;  w_k = ((Ri_k0 p_x + Ri_k1 p_y) + Ri_k2 p_z) + pose_scale ti_k    (td_cloud_keys)
 *     e_k = w_k - pose_scale tj_k;  q_k = (Rj_0k e_0 + Rj_1k e_1) + Rj_2k e_2;  z = q_2
 *     X = (K00 q_0 + K01 q_1) + K02 q_2;  Y = (K10 q_0 + K11 q_1) + K12 q_2;  uj = X / z;  vj = Y / z
 *     inside = ok_i and z > 0 and 0 <= uj <= W-1 and 0 <= vj <= H-1     (a NaN fails)
 *     x0 = min(floor(uj), W-2);  y0 = min(floor(vj), H-2);  fx = uj - x0;  fy = vj - y0
 *     t00, t01, t10, t11 = ds_j at (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1), all four ok_j
 *     top = t00 + fx (t01 - t00);  bot = t10 + fx (t11 - t10);  s = top + fy (bot - top)
 *     neighbour j votes when inside, the taps are ok and |z - s| <= tol min(z, s)
 *   key, payload [(c1-c0) H W] (in/out, td_cloud_keys' pairs of the centre frames) or both NULL.  With key: a pixel whose key is
 *     INT64_MAX is skipped (0 votes, not tested); a tested pixel with fewer than min_views votes gets key INT64_MAX and payload 0.
 *     Without key every pixel is tested and nothing but votes is written.
 *   votes [(c1-c0) H W] uint8 (out) or NULL (only with key);  stats [2] int64 (device) or NULL: incremented by the numbers of pixels
 *     tested and of tested pixels with fewer than min_views votes.
 *   TD_ERR_BAD_ARG before any launch: a null depth, poses, K or inv_K, key without payload or payload without key, neither key nor
 *     votes, N < 0, H < 2, W < 2, radius outside 1..8, min_views outside 0 .. 2 radius, tol negative or NaN, not 0 <= lo <= c0 <=
 *     c1 <= hi <= N, hi - lo < 2 radius + 1.  N = 0 or c0 = c1 is a successful no-op without a launch (checked before the window's
 *     length).  TD_ERR_UNSUPPORTED: a frame of more than 2^29 pixels (offsets inside a frame are 32-bit).
 */
#define TD_VIEWS_MAX_RADIUS 8        /* the largest radius: 16 neighbouring frames */
int td_cloud_views(const float* depth, const double* poses, TD_HOST const double* K, TD_HOST const double* inv_K, int N, int H, int W,
                   int c0, int c1, int lo, int hi, int radius, int min_views, double tol, double depth_scale, double pose_scale,
                   double min_depth, double max_range, long long* key, unsigned long long* payload, uint8_t* votes, long long* stats,
                   td_stream_t stream);

/*
 * Truncated signed distance fusion: surface points with oriented normals from depth maps and poses (csrc/td_tsdf.hip,
 * tripled_amd/tsdf.py).  The reference has no such program: the statements are tsdf.samples_numpy and tsdf.surface_numpy, which the
 * kernels equal bit for bit.  td_tsdf_samples writes (key, payload) pairs of td_cloud_keys' format, which the unchanged torch.sort /
 * td_cloud_heads / cumsum / td_cloud_reduce_packed / merge chain sums into voxel rows; td_tsdf_surface reads the key-sorted rows.
 * No TD_HOST parameter: inv_K is a DEVICE array.  An empty input (B = 0, V = 0) is a successful no-op without a launch.
 *
 * td_tsdf_samples: one launch.  depth, color, poses, stride, border, min_depth, max_range, edge, depth_scale, pose_scale, inv_voxel
 *   (= 1 / voxel, computed once by the caller): as td_cloud_keys;  inv_K [9] float64 (device);  mask [B,H,W] uint8 or NULL: 0 drops
 *   the pixel;  T: the band in voxels, 1 ... TD_TSDF_MAX_T.  A pixel is invalid by the first cause that holds: td_cloud_keys' causes
 *   1 ... 4, then (5) its mask is 0.  For a valid pixel, float64, every operation rounded on its own (ray, p: td_cloud_keys'):
 *     half = voxel 0.5;  trunc = (double)T voxel;  scale = 1048576.0 / trunc
 *     for s = -2T ... 2T:   d_s = p_z + (double)s half;  f = d_s / ray_z;  sample = (ray_x f, ray_y f, ray_z f)
 *       world = camera_to_world(sample)  (td_cloud_keys);  g = world inv_voxel;  i = floor(g);  k = the key of voxel i
 *       the slot is skipped, by the first rule that holds: (range) k is invalid as in td_cloud_keys' cause 5; (duplicate) s > -2T and
 *       k equals the key computed for slot s-1 (whether or not that slot was kept); (band) not |sdf| <= trunc, with
 *         e_k = (i_k + 0.5) voxel - pose_scale t_k;  z_c = (r_02 e_0 + r_12 e_1) + r_22 e_2;  sdf = p_z - z_c
 *       q = (long long)rint(sdf scale), clamped to [-2^20, 2^20];  payload = (q + 2^20) | r << 30 | g << 38 | b << 46
 *   key, payload [4T+1][B H W] (out), slot-major: slot s of pixel p is element (s + 2T) B H W + p; INT64_MAX and 0 for a skipped slot
 *   and for every slot of an invalid pixel.  A voxel's row after the reduction: w = count, S = (sum q_x + 1024 sum q_y + 2^20 sum q_z)
 *   - 2^20 w, the summed distance in units of trunc / 2^20.
 *   stats [TD_TSDF_SAMPLE_STATS] int64 (device) or NULL: incremented by the numbers of valid pixels, of pixels invalid by causes
 *   1 ... 5, of slots kept, and of slots skipped as duplicate, by the band and by the range, in this order.
 *   A thread owns 4, 2 or 1 consecutive columns of a row, as in td_cloud_keys (the mask's alignment counts too).
 *   TD_ERR_BAD_ARG before any launch: a null depth, color, poses, inv_K, key or payload, B < 0, H or W < 1, T outside 1 ...
 *   TD_TSDF_MAX_T, stride < 1, border < 0, voxel or inv_voxel not positive, edge negative or NaN.
 *
 * td_tsdf_surface: one launch, one thread per voxel.  keys [V] int64 ascending and unique, sums [V,7] int64 (the rows above).
 *   D = (double)S / (double)w.  A voxel qualifies when w >= min_weight.  For voxel a and axis x, y, z: b = the voxel one step up the
 *   axis (none when a's coordinate is 2^20 - 1; found by a binary search, for z by looking at the next key).  The edge crosses the
 *   surface when a and b exist and qualify and (S_a >= 0) != (S_b >= 0).  Then, float64, every operation rounded on its own:
 *     t = D_a / (D_a - D_b);  point_k = (float)((i_k + 0.5) voxel), on the edge's axis (float)(((i_k + 0.5) + t) voxel)
 *     gradient of D at a voxel, per axis: (D_+ - D_-) / 2.0 where both neighbours qualify, D_+ - D or D - D_- where one does, else 0
 *     g_k = (1.0 - t) ga_k + t gb_k;  n = sqrt((g_0 g_0 + g_1 g_1) + g_2 g_2);  normal_k = (float)(g_k / n), (0, 0, 0) when n = 0
 *     colour: (2 sum_c + w) / (2 w), integer, of a if t < 0.5, else of b;  weight = min(w_a, w_b), saturating at int32
 *   xyz, normal [V,3,3] float32, rgb [V,3,3] uint8, weight [V,3] int32 (out): written for (voxel, axis) where mask [V,3] uint8 (out,
 *   always written) is 1.  stats [TD_TSDF_SURFACE_STATS] int64 (device) or NULL: incremented by the numbers of voxels under
 *   min_weight, of crossings on x, y and z, and of crossings whose normal is (0, 0, 0).
 *   TD_ERR_BAD_ARG before any launch: a null pointer other than stats, V < 0, voxel not positive, min_weight < 1.
 */
#define TD_TSDF_MAX_T 8              /* the widest band: 33 slots per pixel */
#define TD_TSDF_SAMPLE_STATS 10
#define TD_TSDF_SURFACE_STATS 5
int td_tsdf_samples(const float* depth, const uint8_t* color, const double* poses, const double* inv_K, const uint8_t* mask, int B, int H,
                    int W, int T, double depth_scale, double pose_scale, double voxel, double inv_voxel, int stride, int border,
                    double min_depth, double max_range, float edge, long long* key, unsigned long long* payload, long long* stats,
                    td_stream_t stream);
int td_tsdf_surface(const long long* keys, const long long* sums, long long V, double voxel, long long min_weight, float* xyz,
                    float* normal, uint8_t* rgb, int* weight, uint8_t* mask, long long* stats, td_stream_t stream);

/*
 * The TSDF map ray-cast into camera views: depth, camera-space normal, colour and weight per pixel (csrc/td_tsdf_cast.hip,
 * tripled_amd/tsdf.py).  The reference has no such program: the statement is tsdf.raycast_numpy, which the kernel equals bit for bit.
 *
 * td_tsdf_cast: one fill (the stats rows) and one launch whatever C is, one thread per pixel, no synchronisation, no allocation.
 *   keys [V] int64 ascending and unique, sums [V,7] int64: td_tsdf_surface's rows;  poses [C,3,4] float64 camera-to-world (device);
 *   inv_K [9] float64 (device), as td_tsdf_samples': no TD_HOST parameter;  inv_voxel = 1 / voxel, computed once by the caller.
 *   A voxel qualifies when w >= min_weight;  D = (double)S / (double)w  (td_tsdf_surface).  Per camera [R|t] and pixel (x, y), float64,
 *   every operation rounded on its own (ray, camera_to_world: td_tsdf_samples'):
 *     step = step_voxels voxel;  n_steps = floor((z_far - z_near) / step) + 1
 *     for s = 0 ... n_steps-1:  z_s = z_near + (double)s step;  f = z_s / ray_z;  world = camera_to_world(ray f);  g = world inv_voxel
 *       corners(g):  h_k = g_k - 0.5;  i_k = floor(h_k);  f_k = h_k - i_k;  known when every i_k lies in [-2^20, 2^20 - 1) (a NaN fails;
 *         the last coordinate of a key field has no + neighbour, nothing is carried into the next field) and the eight voxels
 *         i + {0,1}^3 are in keys, qualify and are not the sentinel voxel (the +z corner of a column is the next row)
 *       v: along z  c_xy = D_xy0 + f_z (D_xy1 - D_xy0);  along y  c_x = c_x0 + f_y (c_x1 - c_x0);  along x  v = c_0 + f_x (c_1 - c_0)
 *       prev = sample s-1 if it was known.   hit: prev known, v_prev >= 0, v < 0:  t = v_prev / (v_prev - v);  z_hit = z_(s-1) + t step
 *       back face: prev known, v_prev < 0, v >= 0: the ray ends without a hit.   A ray that runs out of samples is a miss.
 *     at a hit:  g_hit from z_hit as g from z_s, its corners fetched again;  with e the differences of D along the gradient's axis
 *       G_0: e_yz along z, then y;  G_1: e_xz along z, then x;  G_2: e_xy along y, then x;  n = G / sqrt((G_0 G_0 + G_1 G_1) + G_2 G_2)
 *       normal_k = (float)((R_0k n_0 + R_1k n_1) + R_2k n_2): it faces where the surface was seen from and is NOT turned to the viewer;
 *       (0, 0, 0), and counted, when the corners of g_hit are not all known or the root is not > 0
 *       colour (2 sum_c + w) / (2 w) and weight w (saturating at int32) of the voxel floor(g_hit): the corner c_k = (floor(g_k) != i_k);
 *       when the corners of g_hit are not all known, of sample s by the same rule on g_s
 *   depth [C,H,W] float32 (out): (float)z_hit, 0 without a hit;  normal [C,3,H,W] float32 (out);  color [C,3,H,W] uint8 (out): the
 *   background without a hit;  weight [C,H,W] int32 (out): 0 without a hit;  every element is written.
 *   stats [C,TD_TSDF_CAST_STATS] int64 (out, zeroed by the call): rays, hits, back faces, misses (rays = hits + back faces + misses), hits
 *   whose normal is (0, 0, 0).  LDS counters per workgroup, then at most five integer atomics: no floating-point atomics, no kernel
 *   waits on another workgroup, two calls on the same inputs return the same bits.
 *   TD_ERR_BAD_ARG before any launch: a null pointer (also with V = 0), V < 0, C < 0, H or W < 1, voxel or inv_voxel not positive and finite, min_weight < 1, z_near not > 0, z_far not finite or below
 *   z_near, step_voxels not positive and finite, pose_scale not finite, a background outside 0 ... 255.  TD_ERR_UNSUPPORTED: n_steps >
 *   TD_TSDF_CAST_MAX_STEPS, C > 65535, H W > 2^31 - 1.  C = 0 is a successful no-op without a launch;  V = 0 is legal: every ray is a miss.
 */
#define TD_TSDF_CAST_MAX_STEPS 65536 /* the most samples per ray: a guard against a runaway launch, not a tuning value */
#define TD_TSDF_CAST_STATS 5
int td_tsdf_cast(const long long* keys, const long long* sums, long long V, const double* poses, const double* inv_K, int C, int H, int W, double voxel, double inv_voxel,
                 long long min_weight, double z_near, double z_far, double step_voxels, double pose_scale, int bg_r, int bg_g, int bg_b,
                 float* depth, float* normal, uint8_t* color, int* weight, long long* stats, td_stream_t stream);

/*
 * KITTI ground-truth depth maps from velodyne scans, a batch of frames of different sizes per call (csrc/td_velo.hip,
 * tripled_amd/velodyne.py).  Replaces generate_depth_map, mono/datasets/kitti_utils.py:50-102 (the projection :71-86, the last-write
 * scatter :89-90, the duplicate rule with sub2ind :43-47,93-99, the clamp :100), which KITTIRAWDataset.get_depth calls per frame,
 * mono/datasets/kitti_dataset.py:201-215; the scipy.misc.imresize of :210 is not part of it (the evaluation reads native size).
 *
 * td_velo_depth: two fills and two launches whatever B is, no synchronisation, no copy to the host, no allocation.
 *   points [Ntot,4] float32 (x forward, y left, z up, reflectance: column 3 is never read), the frames' scans concatenated, 4-byte
 *        aligned (a 16-byte aligned base is read 16 bytes at a time);  offsets [B+1] int64 (device): frame b owns points
 *        offsets[b] .. offsets[b+1]-1;  P [B,3,4] float64 (device) = P_rect_0c . R_rect_00 . [R|T]_velo_to_cam, multiplied on the host
 *   sizes [B,2] int32 (device) = (H, W) per frame.  The host never reads it: a frame with H outside 1..Hmax, W outside 2..Wmax or
 *        offsets that run backwards gets an all-zero map and a stats row of -1
 *   per point, float64, every product and sum rounded on its own:
 *        kept when x >= 0 (float32 compare; -0.0 passes);  r_k = ((P_k0 x + P_k1 y) + P_k2 z) + P_k3;
 *        u = rint(r_0 / r_2) - 1, v = rint(r_1 / r_2) - 1 (half to even);  valid when 0 <= u < W and 0 <= v < H (NaN and inf fail,
 *        r_2 < 0 can pass);  d = r_2, or (double)x with vel_depth
 *   per pixel: d of the LAST valid point on it, in file order.  Points are grouped by g = v (W-1) + u - 1 (pixel (v, W-1) shares a
 *        group with pixel (v+1, 0); g = -1 is pixel (0,0)): for a group of more than one point, the pixel of the group's FIRST point
 *        is overwritten with the minimum d of the whole group.  Values < 0 become 0, pixels nobody hit are 0.
 *   gt [B,Hmax,Wmax] float32 (out), written completely: frame b occupies the top-left sizes[b], the padding is 0 (the layout of
 *        td_eval_depth's gt)
 *   stats [B,6] int64 (out): points, behind (x < 0), outside (kept but not valid, a NaN x included), valid, pixels hit, pixels
 *        clamped from negative to 0
 *   workspace: td_velo_depth_workspace_bytes(B, Hmax, Wmax) bytes (0: unsupported shape), 8-byte aligned: four tables of 64-bit
 *        integers, one entry per pixel and three per group (H (W-1) + 1 groups per frame)
 *   TD_ERR_BAD_ARG before any launch: a null pointer, B <= 0, Hmax < 1, Wmax < 2, a workspace that is too small or misaligned.
 *   Every table entry is a 64-bit integer minimum (a maximum of indices as the minimum of the complements of index + 1, a minimum of doubles
 *   through an order-preserving map of their bits; -0.0 sorts below +0.0): no floating-point atomics, no kernel waits on another
 *   workgroup, two calls on the same inputs return the same bits.
 */
long long td_velo_depth_workspace_bytes(int B, int Hmax, int Wmax);
int td_velo_depth(const float* points, const long long* offsets, int B, const double* P, const int* sizes, int Hmax, int Wmax,
                  int vel_depth, void* workspace, long long workspace_bytes, float* gt, long long* stats, td_stream_t stream);

/*
 * A point cloud drawn into a batch of camera views: a z-buffered point renderer (csrc/td_render.hip, tripled_amd/render.py).  The
 * reference has no such program: the statement is tripled_amd/render.py:render_numpy, which the kernels equal bit for bit.
 *
 * td_cloud_render: two fills and two launches whatever C is (one launch with V = 0), no synchronisation, no copy to the host, no
 *   allocation.
 *   xyz [V,3] float32, rgb [V,3] uint8: the cloud (device);  poses [C,3,4] float64, camera-to-world (device);  K: a HOST array, the nine
 *        float64 entries of the 3x3 block, in pixels (the third row is not read);  bg_r, bg_g, bg_b: the background colour, 0 ... 255
 *   per point i and camera c, float64, every product, sum and quotient rounded on its own ([R|t]: the pose):
 *        e_k = (double)xyz_k - pose_scale t_k;  q_k = (R_0k e_0 + R_1k e_1) + R_2k e_2  (the transpose of R);  z = q_2
 *        perspective:   u = ((K00 q_0 + K01 q_1) + K02 q_2) / z;  v = ((K10 q_0 + K11 q_1) + K12 q_2) / z;  s = (splat K00) / z
 *        orthographic:  u = (K00 q_0 + K01 q_1) + K02;            v = (K10 q_0 + K11 q_1) + K12;            s = splat K00
 *        in_range = z_near <= z <= z_far  (a NaN fails);  ui = rint(u), vi = rint(v)  (half to even; pixel centres at integer
 *        coordinates);  r = min(8, floor(0.5 s))  (TD_RENDER_MAX_SPLAT = 8)
 *        visible = in_range and ui + r >= 0 and ui - r <= W-1 and vi + r >= 0 and vi - r <= H-1  (in float64; a NaN fails)
 *        every pixel of the square [ui-r, ui+r] x [vi-r, vi+r] inside the image takes the minimum of its entry and
 *        (bits of (float)z) << 32 | i:  the nearest point, and among equal (float)z the lowest index
 *   depth [C,H,W] float32 (out): (float)z of the pixel's point, 0 where nothing was drawn;  color [C,3,H,W] uint8 (out): its rgb, the
 *        background where nothing was drawn;  index [C,H,W] int32 (out): i, -1 where nothing was drawn
 *   stats [C,5] int64 (out): points, out of range, outside (in range, the square misses the image), drawn, pixels hit
 *   workspace: td_cloud_render_workspace_bytes(C, H, W) bytes (0: unsupported shape), 8-byte aligned: one 64-bit integer per pixel
 *   TD_ERR_BAD_ARG before any launch: a null pointer (also with V = 0), C <= 0, H < 1, W < 1, V < 0, z_near not > 0, z_far not finite
 *        or below z_near, splat negative or not finite, a background outside 0 ... 255, a workspace that is too small or misaligned.
 *        TD_ERR_UNSUPPORTED: C > 65535, H W > 2^31 - 1, V >= 2^31 - 1 (the index is the low word of a table entry).
 *   V = 0 is legal: only the fills and the resolve run, and every pixel is background.
 *   The table is a 64-bit integer minimum: no floating-point atomics, no kernel waits on another workgroup, two calls on the same
 *   inputs return the same bits.
 */
#define TD_RENDER_MAX_SPLAT 8        /* the largest r: a splat covers at most 17 x 17 pixels */
long long td_cloud_render_workspace_bytes(int C, int H, int W);
int td_cloud_render(const float* xyz, const uint8_t* rgb, long long V, const double* poses, TD_HOST const double* K, int C, int H, int W,
                    double pose_scale, double z_near, double z_far, double splat, int ortho, int bg_r, int bg_g, int bg_b,
                    void* workspace, long long workspace_bytes, float* depth, uint8_t* color, int* index, long long* stats,
                    td_stream_t stream);

/*
 * A fused cloud scored against the lidar scans (csrc/td_scan.hip, csrc/td_nn.hip, tripled_amd/cloud_eval.py).  The reference has
 * no such program: the statements are cloud_eval.scan_keys_numpy and cloud_eval.nearest_numpy (itself pinned by an all-pairs brute
 * force), which the kernels equal bit for bit.
 *
 * td_scan_keys: one launch, S velodyne scans of mixed lengths -> the (key, payload) pairs of td_cloud_keys, which the unchanged
 *   sort / td_cloud_heads / td_cloud_reduce_* / td_cloud_finish chain fuses.
 *   points [n,4] float32 (x, y, z, reflectance), the scans concatenated (a 16-byte aligned base is read 16 bytes at a time);
 *   offsets [S+1] int64 (device): scan s owns points offsets[s] .. offsets[s+1]-1, found per point by a bounded binary search;
 *   Tr: a HOST array, 3x4 float64 velodyne-to-camera (the Tr: line of the odometry calib.txt);  poses [S,3,4] float64 camera-to-world
 *   (device);  K: a HOST array, the nine float64 entries of the 3x3 block in pixels (rows 0 and 1 are read), NULL allowed with H = 0;
 *   H, W: the image the view test keeps points in, H = 0: no view test.
 *   float64, every product, sum and quotient rounded on its own:
 *     cam_k   = ((Tr_k0 x + Tr_k1 y) + Tr_k2 z) + Tr_k3
 *     u = ((K00 cam_x + K01 cam_y) + K02 cam_z) / cam_z;  v likewise from row 1
 *     world_k = ((r_k0 cam_x + r_k1 cam_y) + r_k2 cam_z) + t_k
 *     key, q  = td_cloud_keys' formula from world inv_voxel
 *     r = g = b = clamp(floor((double)reflectance 255.0 + 0.5), 0, 255), 0 for a NaN reflectance
 *   a point is invalid (key INT64_MAX, payload 0) by the first cause that holds: point (x, y or z not finite, or no scan owns the
 *     point), depth (cam_z outside [min_depth, max_range]; a NaN fails), view (H > 0 and not 0 <= u <= W-1 and 0 <= v <= H-1), range (a
 *     voxel coordinate outside [-2^20, 2^20), or the key is the sentinel)
 *   key [n] int64, payload [n] uint64 (out);  stats [5] int64 (device) or NULL: incremented by valid, point, depth, view, range (LDS
 *     counters per workgroup, then at most five integer atomics per workgroup)
 *   TD_ERR_BAD_ARG before any launch: a null points, offsets, Tr, poses, key or payload, K null with H > 0, n < 0, S < 1, H < 0, W < 0,
 *     W < 1 with H > 0, inv_voxel not > 0, not min_depth <= max_range.  n = 0 is a successful no-op without a launch.
 *
 * td_nn_query: one launch, one thread per query: the nearest reference point within tau, exactly.
 *   query [N,3] float64;  the reference as a sorted grid (cloud_eval.grid_hip): points [M,3] float64 in cell order, order [M] int64 (the
 *   original index of every sorted point), cell_key [C] int64 ascending (td_cloud_keys' packing of floor(x inv_cell) per axis),
 *   cell_start [C+1] int64;  inv_cell = (1 - 2^-20) / tau and tau2 = tau tau are computed on the host, in float64, by this function
 *   and by the grid's builder alike.  |x - y| <= tau puts x and y in cells at most one apart on every axis, so the 27 cells around
 *   the query's cell hold every candidate.
 *   per candidate j: e = point_j - query;  d2 = ((e_x e_x) + (e_y e_y)) + (e_z e_z);  candidate iff d2 <= tau2;  the winner is the
 *   smallest d2, among equal d2 the lowest order[j].  A neighbour cell outside [-2^20, 2^20) is skipped.  A query that is not finite
 *   or whose cell is outside [-2^20, 2^20) is invalid.
 *   d2 [N] float64 (out): +inf when nothing lies within tau or the query is invalid;  index [N] int64 (out): the winner's original
 *   index, -1 likewise
 *   thr2: a HOST array of K <= 16 squared thresholds (NULL allowed with K = 0);  counts [K+2] int64 (device), incremented:
 *   counts[k] by the queries with d2 <= thr2[k], counts[K] by the queries that found a neighbour, counts[K+1] by the invalid queries
 *   (LDS counters per workgroup, then at most K+2 64-bit integer atomics per workgroup)
 *   Every index read from cell_start is clamped to [0, M] and every search stays inside [0, C): a malformed grid reads nothing
 *   outside the buffers.  A thread's work is bounded by 27 x the largest cell population.
 *   TD_ERR_BAD_ARG before any launch: a null query, cell_start, d2, index or counts, points or order null with M > 0, cell_key null
 *     with C > 0, thr2 null with K > 0, N < 0, M < 0, C < 0, C > M, K outside 0 .. 16, tau not > 0 or not finite.  N = 0 is a
 *     successful no-op without a launch;  M = 0 fills the "not found" answer.
 */
int td_scan_keys(const float* points, long long n, const long long* offsets, int S, TD_HOST const double* Tr, const double* poses,
                 TD_HOST const double* K, int H, int W, double min_depth, double max_range, double inv_voxel, long long* key,
                 unsigned long long* payload, long long* stats, td_stream_t stream);
#define TD_NN_MAX_THRESHOLDS 16      /* td_nn_query: the most thresholds (K) of one call */
int td_nn_query(const double* query, long long N, const double* points, const long long* order, long long M, const long long* cell_key,
                const long long* cell_start, long long C, double tau, TD_HOST const double* thr2, int K, double* d2, long long* index,
                long long* counts, td_stream_t stream);

/*
 * A fused cloud aligned to the lidar by iterated closest points (csrc/td_align.hip, tripled_amd/cloud_align.py): x' = c R x + t maps
 * the predicted cloud into the reference's frame.  The correspondences are td_nn_query's; the closed-form solve (Umeyama 1991, the
 * reference's mono/tools/geometry.py umeyama_alignment) runs on the host on the 17 sums and the count below.  The statements are
 * cloud_align.transform_numpy and cloud_align.moments_numpy, which the kernels equal bit for bit.  float64, every product and sum
 * rounded on its own; no floating-point atomics, no kernel waits on another workgroup.
 *
 * td_cloud_transform: one launch, one thread per point.
 *   src [N,3] float64;  c, and the HOST arrays R (nine float64, row-major) and t (three float64), are copied into the launch;
 *   out [N,3] float64 (out), src itself allowed:
 *     out_k = c ((R_k0 x + R_k1 y) + R_k2 z) + t_k
 *   A row that is not finite gives a row that is not finite (which td_nn_query counts as invalid).
 *   TD_ERR_BAD_ARG before any launch: a null src, R, t or out, N < 0, c or an entry of R or t not finite.  N = 0 is a successful
 *     no-op without a launch.
 *
 * td_icp_moments: two launches (ceil(N / 256) workgroups, then one).
 *   cur [N,3] float64: the transformed predicted points that were queried;  ref [M,3] float64: the reference in its ORIGINAL order,
 *   the order td_nn_query's index refers to (NULL allowed with M = 0);  index [N] int64 and d2 [N] float64: td_nn_query's outputs;
 *   origin: a HOST array of three float64, subtracted from both clouds before anything is multiplied.
 *   Row i is matched iff 0 <= index_i < M and d2_i <= trim2 (a NaN fails).  With p = cur_i - origin and q = ref[index_i] - origin a
 *   matched row contributes, in this order, the 17 values
 *     p_x p_y p_z,  q_x q_y q_z,  q_r p_c (nine, row-major: r the slow index),  (p_x p_x + p_y p_y) + p_z p_z,  d2_i
 *   and any other row +0.0 in every slot.  An index_i >= M or < -1 reads nothing and is counted as bad_index.
 *   The order of the sums is fixed and depends on N alone.  Stage 1: workgroup b owns rows 256 b ... 256 b + 255 (rows past N are
 *   +0.0) and reduces them by the halving tree: for s = 128, 64, ..., 1: row j += row j + s for every j < s; row 0 is
 *   partials[b][17].  Stage 2: one workgroup; thread j adds partials[j], partials[j + 256], ... one after the other, in that order,
 *   onto +0.0; the same tree over the 256 threads follows.
 *   workspace: td_icp_moments_workspace(N) bytes (17 float64 per workgroup of stage 1; 0 for N = 0), 8-byte aligned
 *     (TD_ERR_WORKSPACE if workspace_bytes is less)
 *   out: 19 x 8 bytes (out): the 17 sums as float64, then matched and bad_index as int64.  All 19 are cleared first, also for
 *     N = 0, which launches nothing else; the counters are added up in LDS per workgroup, then at most two 64-bit integer atomics per
 *     workgroup.
 *   TD_ERR_BAD_ARG before any launch: a null origin or out, N < 0, M < 0, trim2 not >= 0 (+inf is allowed: no trimming), an origin
 *     that is not finite, workspace_bytes < 0, a workspace or out that is not 8-byte aligned; with N > 0: a null cur, index, d2 or
 *     workspace, ref null with M > 0.
 */
int td_cloud_transform(const double* src, long long N, double c, TD_HOST const double* R, TD_HOST const double* t, double* out,
                       td_stream_t stream);
#define TD_ICP_SLOTS 17              /* the sums of td_icp_moments: p (3), q (3), q_r p_c (9, row-major), |p|^2, d2 */
long long td_icp_moments_workspace(long long N);
int td_icp_moments(const double* cur, long long N, const double* ref, long long M, const long long* index, const double* d2, double trim2,
                   TD_HOST const double* origin, void* workspace, long long workspace_bytes, double* out, td_stream_t stream);

/*
 * Point-to-plane alignment: surface normals of a cloud (csrc/td_normals.hip, tripled_amd/cloud_normals.py) and the sums of the
 * linearised point-to-plane step (csrc/td_align.hip, tripled_amd/cloud_align.py, criterion="plane").  The statements are
 * cloud_normals.normals_numpy and cloud_align.plane_moments_numpy, which the kernels equal bit for bit.  float64, every product and
 * sum rounded on its own; no floating-point atomics, no kernel waits on another workgroup.
 *
 * td_cloud_normals: one launch, one thread per query.
 *   query [N,3] float64;  points [M,3] float64, cell_key [C] int64, cell_start [C+1] int64: a cloud sorted into td_nn_query's grid
 *   for `tau` (cloud_eval.grid_hip; `order` is not needed; points and cell_key may be NULL with M = 0, C = 0);  radius in (0, tau];
 *   Q = 2^18 / radius, divided ONCE by the caller;  min_neighbours >= 3;  max_curvature >= 0 (+inf: nothing is rough).
 *   The query walks the 27 cells around it like td_nn_query.  For every grid point p with e = p - query and
 *   ((e_x e_x) + (e_y e_y)) + (e_z e_z) <= radius radius (a NaN fails): n += 1, i_k = (int64) rint(e_k Q) (half to even),
 *   S1_k += i_k, S2_kl += i_k i_l for k <= l: ten 64-bit integer sums, independent of every order.  Then in float64
 *     m_k = double(S1_k) / double(n),  C_kl = double(S2_kl) / double(n) - m_k m_l,
 *   C is diagonalised by cyclic Jacobi over (0,1), (0,2), (1,2) with 4 sweeps, never fewer (a rotation whose off-diagonal is exactly 0
 *   is skipped; theta = (a_qq - a_pp) / (2 a_pq), t = sign(theta) / (|theta| + sqrt(theta theta + 1)), c = 1 / sqrt(t t + 1), s = t c;
 *   the update formulas are cloud_normals.py's docstring), the normal is the eigenvector column of the smallest diagonal entry (lowest
 *   index among equal ones) divided by sqrt(((x x) + (y y)) + (z z)), its sign chosen so that the component of largest magnitude is
 *   positive (lowest index among ties); curvature = max(lambda_min, 0) / ((l0 + l1) + l2).
 *   normal [N,3] float64 (out): +0.0 in all three when the query has none;  curvature [N] float64 (out): +inf when undefined;
 *   count [N] int64 (out): n, 0 for an invalid query;  counters [5] int64, INCREMENTED (LDS first, then one 64-bit atomic per workgroup
 *   and counter), every query in exactly one, the first that holds: [4] invalid (not finite or outside the key range, as in
 *   td_nn_query), [1] few (n < min_neighbours), [2] degenerate (trace not > 0, middle eigenvalue not > 0, or anything not finite),
 *   [3] rough (curvature > max_curvature: the curvature is written, the normal is not), [0] valid.
 *   TD_ERR_BAD_ARG before any launch: a null query, cell_start or output, N, M or C < 0, C > M, tau not positive and finite, radius
 *     outside (0, tau], Q radius not within 2^-32 of 2^18 (Q is not 2^18 / radius to rounding), min_neighbours < 3, max_curvature not >= 0, points null with M > 0, cell_key null
 *     with C > 0.  TD_ERR_UNSUPPORTED: M >= 2^26 (with |i_k| <= 2^18 + 1 no sum can overflow below that).  N = 0 is a successful
 *     no-op without a launch.
 *
 * td_icp_plane_moments: td_icp_moments' contract (two launches, the same two-stage tree, the order of the sums depends on N alone)
 *   with one more input, normals [M,3] float64 in the reference's ORIGINAL order (NULL allowed with M = 0), and 37 slots.
 *   Row i is matched iff 0 <= index_i < M, d2_i <= trim2 (a NaN fails) and normals[index_i] is not all zero; a row that passes the
 *   first two tests and whose neighbour has no normal is counted as no_normal.  With p = cur_i - origin, q = ref[j] - origin,
 *   n = normals[j], g = p - q:
 *     a = (p_y n_z - p_z n_y,  p_z n_x - p_x n_z,  p_x n_y - p_y n_x,  n_x,  n_y,  n_z,  (p_x n_x + p_y n_y) + p_z n_z)
 *     r = (n_x g_x + n_y g_y) + n_z g_z
 *   and a matched row contributes, in this order,  a_i a_j for i <= j, row-major (28),  a_i r (7),  r r,  d2_i;  any other row +0.0.
 *   workspace: td_icp_plane_moments_workspace(N) bytes (37 float64 per workgroup of stage 1; 0 for N = 0), 8-byte aligned
 *     (TD_ERR_WORKSPACE if workspace_bytes is less)
 *   out: 40 x 8 bytes (out): the 37 sums as float64, then matched, bad_index and no_normal as int64.  All 40 are cleared first,
 *     also for N = 0, which launches nothing else.
 *   TD_ERR_BAD_ARG before any launch: as td_icp_moments, and normals null with N > 0 and M > 0.
 */
#define TD_NORMALS_SWEEPS 4          /* Jacobi sweeps of td_cloud_normals, never fewer */
int td_cloud_normals(const double* query, long long N, const double* points, long long M, const long long* cell_key,
                     const long long* cell_start, long long C, double tau, double radius, double Q, long long min_neighbours,
                     double max_curvature, double* normal, double* curvature, long long* count, long long* counters, td_stream_t stream);
#define TD_ICP_PLANE_SLOTS 37        /* the sums of td_icp_plane_moments: a_i a_j for i <= j, row-major (28), a_i r (7), r r, d2 */
long long td_icp_plane_moments_workspace(long long N);
int td_icp_plane_moments(const double* cur, long long N, const double* ref, const double* normals, long long M, const long long* index,
                         const double* d2, double trim2, TD_HOST const double* origin, void* workspace, long long workspace_bytes,
                         double* out, td_stream_t stream);

/*
 * Surfel rendering (csrc/td_surfel.hip, tripled_amd/cloud_normals.py, tripled_amd/render.py): normals oriented towards the nearest
 * camera, and a cloud drawn as oriented discs in space.  The reference has no such program: the statements are
 * cloud_normals.orient_numpy and render.render_surfels_numpy, which the kernels equal bit for bit.  float64, every product, sum and
 * quotient rounded on its own; integer atomics only; no kernel waits on another workgroup.
 *
 * td_normals_orient: one fill and one launch, one thread per point, the camera centres staged through LDS 256 at a time (any C).
 *   xyz [V,3] float32, normal [V,3] float32 (all three components zero: the point has none), poses [C,3,4] float64 camera-to-world,
 *   all on the device.  Per point p, with centre_c = pose_scale t_c and w = centre_c - (double)p:
 *     d2_c = ((w_x w_x) + (w_y w_y)) + (w_z w_z);  the viewpoint is the c of the smallest d2_c, the lowest c among equal ones; a NaN
 *     never wins;  s = ((n_x w_x) + (n_y w_y)) + (n_z w_z) with the winner's w;  the normal is negated (exactly) when s < 0.
 *   out_normal [V,3] float32 (out);  camera [V] int32 (out): the winner, -1 when every distance is a NaN;  stats [4] int64 (out, set):
 *   flipped, kept (s >= 0), none (no normal: copied as it is, the camera is still written), invalid (no camera won, or s is a NaN:
 *   the normal is copied as it is).  Every point is in exactly one.
 *   TD_ERR_BAD_ARG before any launch: a null or misaligned pointer, V < 0, C <= 0.  V = 0 clears the stats and launches nothing.
 *
 * td_cloud_render_surfels: two fills and two launches (one with V = 0), td_cloud_render's inputs, workspace
 *   (td_cloud_render_workspace_bytes) and table, plus normal [V,3] float32, radius > 0 (the disc's, in the cloud's units), cull 0/1,
 *   ambient in [0, 1] and form (0: the library's choice, 1: one thread per surfel, 2: boxes of more than 4 pixels go through an LDS
 *   queue and are rasterised by a wave each; all forms return the same bits).  K: K10 must be 0 and K00, K11 positive.
 *   Per point i and camera c, with e, q_0, q_1, z = q_2 as in td_cloud_render:
 *     m_k = (R_0k n_0 + R_1k n_1) + R_2k n_2;  a point without a normal gets m = (0, 0, -1) (a billboard)
 *     out of range unless z_near <= z <= z_far;  culled (cull = 1) when ((m_0 q_0) + (m_1 q_1)) + (m_2 z) > 0, orthographic m_2 > 0
 *     perspective:  u = ((K00 q_0 + K01 q_1) + K02 z) / z;  v = (K11 q_1 + K12 z) / z;  tm = max(z_near, z - radius);  g = radius / tm;
 *                   a_x = g (1 + |q_0| / z);  a_y = g (1 + |q_1| / z);  b_x = K00 a_x + |K01| a_y;  b_y = K11 a_y
 *     orthographic: u = (K00 q_0 + K01 q_1) + K02;  v = K11 q_1 + K12;  b_x = (K00 + |K01|) radius;  b_y = K11 radius
 *     ui = rint(u), vi = rint(v);  r = floor(max(b_x, b_y) + (1/2 + 2^-10));  capped when r > 16, then r = 16 (TD_SURFEL_MAX)
 *     outside unless ui + r >= 0, ui - r <= W-1, vi + r >= 0, vi - r <= H-1 (a NaN fails);  else drawn
 *   Per pixel (x, y) of the box [ui-r, ui+r] x [vi-r, vi+r] inside the image:
 *     d_1 = (y - K12) / K11;  d_0 = ((x - K02) - K01 d_1) / K00
 *     perspective:  den = ((m_0 d_0) + (m_1 d_1)) + m_2;  num = ((m_0 q_0) + (m_1 q_1)) + (m_2 z);  t = num / den;  hit = (t d_0, t d_1, t)
 *     orthographic: den = m_2;  num = ((m_0 (q_0 - d_0)) + (m_1 (q_1 - d_1))) + (m_2 z);  t = num / den;  hit = (d_0, d_1, t)
 *     covered when den < 0 or den > 0, ((e_0 e_0) + (e_1 e_1)) + (e_2 e_2) <= radius radius for e = hit - q, and z_near <= t <= z_far;
 *     a covered pixel takes the minimum of its entry and (bits of (float)t) << 32 | i
 *   depth, index, color: as td_cloud_render, the depth being (float)t;  normal_map [C,3,H,W] float32 (out): (float)m of the winner,
 *   negated when den > 0, +0.0 where nothing was drawn;  the colour is the point's own when ambient = 1, else per channel
 *   min(255, floor(c (ambient + (1 - ambient) shade) + 0.5)) with shade = |den| / sqrt(((d_0 d_0) + (d_1 d_1)) + 1) (orthographic: / sqrt(1)).
 *   stats [C,8] int64 (out), in this order: points, out_of_range, outside (the box misses the image), culled, capped, billboards,
 *   drawn, pixels_hit;  points = out_of_range + culled + outside + drawn;  capped and billboards count drawn surfels.
 *   TD_ERR_BAD_ARG before any launch: td_cloud_render's causes, a null normal or normal_map, radius not positive and finite, ambient
 *   outside [0, 1], form outside 0 ... 2, K not finite, K10 != 0, K00 or K11 not positive.  TD_ERR_UNSUPPORTED: as td_cloud_render.
 */
int td_normals_orient(const float* xyz, const float* normal, long long V, const double* poses, int C, double pose_scale,
                      float* out_normal, int* camera, long long* stats, td_stream_t stream);
#define TD_SURFEL_MAX 16             /* the largest r: the pixel box of a disc is at most 33 x 33 */
#define TD_SURFEL_SLACK 0.5009765625 /* 1/2 + 2^-10: 1/2 for rint(u) against u, 2^-10 for the rounding of the bound and of the pixel test */
int td_cloud_render_surfels(const float* xyz, const uint8_t* rgb, const float* normal, long long V, const double* poses,
                            TD_HOST const double* K, int C, int H, int W, double pose_scale, double z_near, double z_far, double radius, int ortho, int cull,
                            double ambient, int form, int bg_r, int bg_g, int bg_b, void* workspace, long long workspace_bytes,
                            float* depth, uint8_t* color, int* index, float* normal_map, long long* stats, td_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIPLED_HIP_H */

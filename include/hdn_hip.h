/*
 * hdn_hip.h — C ABI of libhdn_hip.so: the MI355X (gfx950) implementation of HDN's
 * per-frame homography-estimation hot path.
 *
 * The reference (zhanxinrui/HDN) has no native plugin ABI: its extension points are
 * module-level Python functions that are rebound.  Each entry point
 * below is what a binding for one of those functions calls; the reference interface it
 * replaces is cited as file:line under /root/reference.  INTEGRATION.md shows the
 * ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 unless stated otherwise;
 *   - tensors are NCHW exactly as the reference's torch tensors are laid out;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all calls are
 *     asynchronous on it and never synchronise or allocate;
 *   - return 0 on success, HDN_E_* (< 0) for argument errors, or -(1000 + hipError_t)
 *     when the launch itself failed; nothing is written on an argument error.
 */
#ifndef HDN_HIP_H
#define HDN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define HDN_OK 0
#define HDN_E_NULL (-1)  /* a required pointer is NULL            */
#define HDN_E_SHAPE (-2) /* non-positive size, or kernel > search */
#define HDN_E_LIMIT (-3) /* size exceeds what the kernels support */
#define HDN_E_ALIAS (-4) /* output aliases an input               */
#define HDN_E_NORCCL (-5) /* librccl.so.1 could not be loaded (collective entry points only) */
#define HDN_E_PEER (-6)   /* one-shot gather: an earlier call timed out waiting for a peer; the context is unusable */
/* RCCL failures are returned as -(2000 + ncclResult_t). */

/* ABI version of this header; hdn_abi_version() of the loaded library must match. */
#define HDN_ABI_VERSION 10
int hdn_abi_version(void);

/* Name of the kernel variant the last hdn_xcorr_* call on this thread dispatched to
 * ("f1_61x61_31x31", "generic_lds", ...).  For tests and profiles. */
const char* hdn_last_xcorr_variant(void);

/*
 * Kernel used for the 31x31 (x) 61x61 shape (BASELINE north-star shape).  v >= 0 selects it for the whole process,
 * v < 0 only queries; returns the previous value (or HDN_E_LIMIT for a value that is not one of the two below).  Both take any
 * pointer alignment and meet the same parity bar; they differ in rounding: the direct kernel accumulates each output in one fixed
 * fp32 chain (planes independent), the FFT kernel has a smaller error against float64 but transforms planes in pairs, so a plane's
 * rounding depends on its neighbour's magnitude, and a NaN / Inf anywhere in a plane reaches every output of that plane and of its
 * partner (the direct kernel keeps it to the windows that contain it, as the reference does).  For tests, benchmarks and A/B runs.
 * Error class of the FFT kernel (measured, post-ReLU N(0,1) data, outputs of O(300)): rms 2.0e-5, max 1.8e-4 ABSOLUTE against
 * float64 — i.e. it does NOT meet 1e-4 abs on the correlation outputs themselves (neither does the reference's own fp32 sum:
 * 1.8e-4); the bound it is held to is |hip - ref| <= 1e-4 + 2e-6 * sum|x*k| and an error against float64 of at most twice the
 * reference's.  The 1e-4 abs of BASELINE's north_star is on the predicted corner offsets, which no correlation feeds.
 * (Values 0, 2, 3, 4 named four more forms in ABI <= 4 — row-first FFT, dense direct sum, split-bf16 matrix cores, two-waves-per-SIMD
 * FFT — retired in round 4: none was faster.)
 */
#define HDN_NORTH_DIRECT 1       /* packed-FMA direct sum, exact-zero taps skipped */
#define HDN_NORTH_FFT_COL 5      /* (default) 64x64 fp32 FFT per pair of planes on the transposed problem: planes go HBM -> registers row by row */
int hdn_xcorr_north_variant(int v);

/*
 * Depthwise (per batch, per channel) valid cross-correlation, stride 1, no flip:
 *   out[b,c,i,j] = sum_{u,v} x[b,c,i+u,j+v] * k[b,c,u,v]
 *   x[B,C,Hx,Wx], k[B,C,Hk,Wk] -> out[B,C,Hx-Hk+1,Wx-Wk+1]
 * Replaces xcorr_depthwise(x, kernel), hdn/core/xcorr.py:37-46
 * (called from DepthwiseXCorr.forward, hdn/models/head/ban.py:76).
 */
int hdn_xcorr_depthwise_f32(const float* x, const float* k, float* out,
                            int B, int C, int Hx, int Wx, int Hk, int Wk, void* stream);

/*
 * The log-polar variant: x is first padded by Hx/2 rows on each side CIRCULARLY
 * (rows = angle), then by Wx/2 columns on each side by edge REPLICATION (columns =
 * log-radius), then correlated as above.  The pad is never materialised in HBM.
 *   out[B,C,Hx+2*(Hx/2)-Hk+1, Wx+2*(Wx/2)-Wk+1]
 * Replaces xcorr_depthwise_circular(x, kernel), hdn/core/xcorr.py:48-61
 * (called from DepthwiseXCorrCirc.forward, hdn/models/head/ban_lp.py:38).
 */
int hdn_xcorr_depthwise_circ_f32(const float* x, const float* k, float* out,
                                 int B, int C, int Hx, int Wx, int Hk, int Wk, void* stream);

/*
 * Several correlations of one frame in ONE launch (the 3 levels x
 * {cls,loc} of MultiBAN, ban.py:102-109, or of MultiCircBAN, ban_lp.py:69-73).
 * xs/ks/outs are HOST arrays of n device pointers; every problem has the same shape.
 */
int hdn_xcorr_depthwise_multi_f32(const float* const* xs, const float* const* ks, float* const* outs, int n,
                                  int circular, int B, int C, int Hx, int Wx, int Hk, int Wk, void* stream);

/*
 * Backward of the two depthwise correlations above (csrc/xcorr_bwd.hip): the gradients of a loss with respect to x and k,
 * given gout = d loss / d out.  The functions it differentiates are xcorr_depthwise / xcorr_depthwise_circular,
 * hdn/core/xcorr.py:37-61.  Per plane (b, c), with ph = Hx/2, pw = Wx/2 when `circular` (both 0 otherwise),
 * HP = Hx + 2 ph, WP = Wx + 2 pw, Ho = HP - Hk + 1, Wo = WP - Wk + 1 and the padded plane
 *   xp[P][Q] = x[(P - ph) mod Hx][clamp(Q - pw, 0, Wx - 1)]          (rows wrap first, then columns replicate)
 *   out[i][j] = sum_{u,v} xp[i+u][j+v] k[u][v]                        (the forward)
 * the gradients are
 *   gk[u][v]  = sum_{i,j} gout[i][j] xp[i+u][j+v]
 *   gxp[P][Q] = sum_{u,v} gout[P-u][Q-v] k[u][v]   over the (u, v) with 0 <= P-u < Ho and 0 <= Q-v < Wo
 *   gx[r][s]  = sum of gxp[P][Q] over the padded positions that are copies of (r, s):
 *                 rows    P in {r + ph - Hx, r + ph, r + ph + Hx} intersected with [0, HP);
 *                 columns Q in [0, pw] if s == 0, joined with [pw + Wx - 1, WP) if s == Wx - 1, else Q = s + pw
 *               (plain variant: gx = gxp).
 *   x[B,C,Hx,Wx], k[B,C,Hk,Wk], gout[B,C,Ho,Wo] -> gx[B,C,Hx,Wx], gk[B,C,Hk,Wk]
 * gx or gk may be NULL: that gradient is then neither computed nor written (both NULL: HDN_E_NULL).  fp32 fused multiply-adds in a
 * fixed order and no atomics: two calls are bit-equal and a plane's result does not depend on the number of planes.  The pad is never
 * materialised in HBM.  Checked before any launch, in this order: x, k, gout NULL or both outputs NULL -> HDN_E_NULL; the forward's
 * shape rules -> HDN_E_SHAPE / HDN_E_LIMIT; an output equal to an input or to the other output -> HDN_E_ALIAS; the forward's
 * plane-count limits -> HDN_E_LIMIT.
 */
int hdn_xcorr_depthwise_bwd_f32(const float* x, const float* k, const float* gout,
                                float* gx, float* gk, int circular,
                                int B, int C, int Hx, int Wx, int Hk, int Wk, void* stream);

/* Pure host query: the launch form hdn_xcorr_depthwise_bwd_f32 takes for a plane shape.  0: the LDS form,
 * (HP WP + Hk Wk + Ho Wo) 4 bytes <= 60 KiB; 1: the form that reads global memory; HDN_E_SHAPE / HDN_E_LIMIT as the entry point. */
int hdn_xcorr_bwd_form(int circular, int Hx, int Wx, int Hk, int Wk);

/*
 * Channel-contracting correlation of the alternative UPChannelBAN head (not on the production path):
 *   out[b,o,i,j] = sum_c sum_{u,v} x[b,c,i+u,j+v] * k[b,o*C+c,u,v]
 *   x[B,C,Hx,Wx], k[B,O*C,Hk,Wk] -> out[B,O,Hx-Hk+1,Wx-Wk+1],  1 <= O <= 8
 * Replaces xcorr_fast(x, kernel), hdn/core/xcorr.py:26-34, and xcorr_slow, :10-23 (same arithmetic).
 * No shipped configuration selects UPChannelBAN (0 calls per frame).  A workgroup owns 64 output positions of one batch
 * element; its 4 waves split the C channels, each lane accumulating its O outputs in registers (taps wave-uniform, through the
 * scalar cache), and the 4 partial sums meet through LDS in a fixed order (deterministic): 57 / 122 us for O = 2 / 4 at
 * B = 64, C = 256.  Exact fp32 on the vector pipe: with O <= 8 output columns a 32x32 MFMA tile would be 6-25 % used and the
 * f32-input MFMA rate equals the vector rate.
 */
int hdn_xcorr_fast_f32(const float* x, const float* k, float* out, int B, int C, int O, int Hx, int Wx, int Hk,
                       int Wk, void* stream);

/*
 * PreShareFeature.forward in eval mode, fused: 3 x (conv3x3 pad 1, no bias -> BatchNorm
 * (running stats) -> ReLU), channels 1 -> 4 -> 8 -> 1, img[B,1,H,W] -> out[B,1,H,W].
 * `folded` (HDN_SF_PARAMS floats, device) = conv weights re-laid for the kernel followed
 * by the per-channel BN scale/shift; build it with hdn_amd.share_feature.fold_params().
 *   [0,36)    w1t[k][co]          k = ky*3+kx, co in 0..3      (from ShareFeature.0.weight[co,0,ky,kx])
 *   [36,324)  w2p[ci/2][k][co][ci%2]   ci in 0..3, co in 0..7  (from ShareFeature.3.weight[co,ci,ky,kx])
 *   [324,396) w3p[ci/2][k][ci%2]       ci in 0..7              (from ShareFeature.6.weight[0,ci,ky,kx])
 *             (even/odd input channels adjacent: one SGPR pair feeds one v_pk_fma_f32)
 *   [396,409) alpha[13]           gamma / sqrt(var + 1e-5), layers concatenated (4+8+1)
 *   [409,422) beta[13]            bias - mean * alpha
 * Replaces PreShareFeature.forward, .../Oneline_DLTv1/preprocess/input_feature_extractor.py:27-29.
 */
#define HDN_SF_PARAMS 422
int hdn_share_feature_f32(const float* img, const float* folded, float* out, int B, int H, int W, void* stream);

/*
 * PreShareFeature for training (csrc/share_feature_train.hip): the same chain with BatchNorm on this call's batch statistics, and its backward.
 *   c1 = conv1(x), a1 = relu(bn1(c1)), c2 = conv2(a1), a2 = relu(bn2(c2)), c3 = conv3(a2), y = relu(bn3(c3))
 * Per channel over the N = B H W values of a pre-normalisation plane c: mean, var (biased), invstd = 1 / sqrt(var + eps), then
 *   alpha = gamma invstd,  beta = bias - mean alpha,  z = c alpha + beta,  a = relu(z),  x^ = (c - mean) invstd.
 * Layout: img / out / grad_out / grad_img [B,1,H,W]; w1[4][1][3][3], w2[8][4][3][3], w3[1][8][3][3] in PyTorch's own order; gamma[13], bias[13]
 * the three BatchNorms' weight / bias concatenated (4 + 8 + 1 channels); `saved` = c1 [B,4,H,W], c2 [B,8,H,W], c3 [B,1,H,W] one after the other
 * (13 N floats, hdn_share_feature_train_saved_bytes); `stats` = mean[13], invstd[13], unbiased variance[13] (39 floats).  The activations are never
 * stored: every consumer recomputes relu(c alpha + beta) on load, so forward and backward read the same ReLU masks.
 *
 * hdn_share_feature_train_fwd_f32.  stats_mode 0: batch statistics (N >= 2, else HDN_E_SHAPE); per layer one convolution launch that also writes
 * per-workgroup partial sums of c and c^2, and a one-workgroup launch that adds them in a fixed order and writes the layer's stats; the sums are
 * float64 from the first add on, var = sum c^2 / N - mean^2 in float64, unbiased = var N / (N - 1); mean, invstd, unbiased are rounded to fp32 once
 * and alpha / beta are built from the rounded values.  stats_mode 1 (eval): mean_var_or_null = the caller's mean[13], var[13]; stats_out receives
 * (mean, 1 / sqrt(var + eps), var) and nothing is reduced.  eps1 .. eps3: each BatchNorm's own eps.  mean_var_or_null is not read in mode 0.
 *
 * hdn_share_feature_bwd_f32: for grad_out = d loss / d y, with dz = g [z > 0] per layer from layer 3 down to layer 1 (g = grad_out, then grad_a):
 *   S1 = sum dz = grad_bias,   S2 = sum dz x^ = grad_gamma                     (float64 partials, fixed order)
 *   dc = alpha (dz - S1 / N - x^ S2 / N)   (stats_mode 0),   dc = alpha dz     (stats_mode 1: the statistics are constants)
 *   grad_a[ci](p) = sum over co, k of w[co][ci][k] dc[co](p - k)               (a gather over 9 CO taps)
 *   grad_w[co][ci][k] = sum over p of dc[co](p) a[ci](p + k)                   (fp32 in a workgroup, float64 across workgroups, fixed order)
 * `stats` is the forward's stats_out, stats_mode the forward's.  grad_params_or_null = grad_w1[36], grad_w2[288], grad_w3[72], grad_gamma[13],
 * grad_bias[13] (422 floats); grad_img_or_null = d loss / d img.  A NULL output is neither computed nor written (NULL grad_img skips layer 1's data
 * adjoint, NULL grad_params every weight adjoint and, in mode 1, every S1 / S2 reduction); both NULL: HDN_E_SHAPE.
 *
 * No atomics anywhere: every output of both calls, grad_img included, is bit-reproducible between calls.  One launch form (a workgroup owns 1024
 * consecutive pixels of one image), so there is no form query.  workspace: hdn_share_feature_train_workspace_bytes(B, H, W) bytes for either call,
 * 16-byte aligned; the other pointers need only float alignment.  The two queries are host only; negative = HDN_E_*.
 * Checked before the first HIP call: a NULL pointer (mean_var in mode 1 included) -> HDN_E_NULL; B, H or W <= 0, a stats_mode other than 0 / 1,
 * N < 2 in mode 0, no gradient asked for -> HDN_E_SHAPE; 13 N > 2^31 - 1, a workspace that is unaligned or too small -> HDN_E_LIMIT; the byte
 * range of an output (the workspace included) overlapping an input's or another output's -> HDN_E_ALIAS.  Asynchronous on `stream`, allocates nothing.
 * Differentiates PreShareFeature.forward in train() mode, .../Oneline_DLTv1/preprocess/input_feature_extractor.py:27-29 (six calls per training
 * step: model_builder_e2e_unconstrained_v2.py:420-427, homo_model_builder.py:154-171).
 */
long long hdn_share_feature_train_workspace_bytes(int B, int H, int W);
long long hdn_share_feature_train_saved_bytes(int B, int H, int W);
int hdn_share_feature_train_fwd_f32(const float* img, const float* w1, const float* w2, const float* w3, const float* gamma, const float* bias,
                                    const float* mean_var_or_null, float eps1, float eps2, float eps3, int stats_mode, float* out, float* saved,
                                    float* stats_out, float* workspace, long long workspace_bytes, int B, int H, int W, void* stream);
int hdn_share_feature_bwd_f32(const float* img, const float* w1, const float* w2, const float* w3, const float* gamma, const float* bias,
                              const float* saved, const float* stats, const float* grad_out, float* grad_img_or_null, float* grad_params_or_null,
                              float* workspace, long long workspace_bytes, int stats_mode, int B, int H, int W, void* stream);

/*
 * 4-point DLT: H (3x3, H[2][2] = 1) with H * src_i ~ src_i + off_i.
 *   src[B,8], off[B,8] = (x,y) of 4 points in the caller's order (the reference's internal
 *   reordering, utils.py:18-26, does not change the solution); H_out[B,9] row-major.
 * The 8x8 system is solved in float64 (Gauss-Jordan, partial pivoting) and rounded once.
 * Replaces DLT_solve(src_p, off_set), .../Oneline_DLTv1/utils.py:7-67.
 */
int hdn_dlt_solve_f32(const float* src, const float* off, float* H_out, int B, void* stream);

/*
 * Projective bilinear sampler on the [-1,1]^2 grid with the reference's exact tap/clamp
 * /weight rules (see DESIGN.md "warp semantics"): img[B,C,H,W] (NCHW), theta[B,9]
 * -> out[B,H,W,C] (NHWC, as the reference returns it).
 * Replaces transformer(U, theta, out_size), .../Oneline_DLTv1/utils.py:70-254.
 */
int hdn_warp_f32(const float* img, const float* theta, float* out, int B, int C, int H, int W, void* stream);

/* The same sampler, also returning the second value of the reference's transformer(): `condition` = the number of
 * output pixels (over the whole batch) whose projective denominator satisfies |t| > 1e-7 after the 1e-6 nudge
 * (utils.py:236-241).  count_or_null: one device uint32, zeroed by the call on `stream` before the launch. */
int hdn_warp_count_f32(const float* img, const float* theta, float* out, unsigned int* count_or_null, int B, int C,
                       int H, int W, void* stream);

/*
 * Fused DLT_solve + transform for the full-patch case: H = DLT(h4p, off);
 * theta = M^-1 H M with M = [[W/2,0,W/2],[0,H/2,H/2],[0,0,1]]; warped = sampler(img, theta).
 *   h4p[B,8], off[B,8], img[B,1,H,W] -> H_out[B,9] (the un-normalised H), warped[B,1,H,W]
 * Replaces the DLT_solve + Homo_STN pair of ModelBuilder.track_proj,
 * hdn/models/model_builder_e2e_unconstrained_v2.py:195-210, and of HomoModelBuilder.forward,
 * .../models/homo_model_builder.py:166-170.
 */
int hdn_dlt_warp_f32(const float* h4p, const float* off, const float* img, float* H_out, float* warped,
                     int B, int H, int W, void* stream);
/* The same with the images `img_batch_stride` floats apart (>= H * W): one channel of a [B,C,H,W] tensor without a copy (HomoModelBuilder.forward
 * warps channel 0 of the pair, homo_model_builder.py:166-170). */
int hdn_dlt_warp_strided_f32(const float* h4p, const float* off, const float* img, long long img_batch_stride, float* H_out, float* warped, int B,
                             int H, int W, void* stream);

/*
 * One step of the tracker's refinement loop (hdn/tracker/hdn_tracker_proj_e2e.py:242-250; trip count 1 in the shipped
 * tracker, 2 in BASELINE config 5):  H_hm = inv(H) / inv(H)[2,2];  warped = cv2.warpPerspective(search, inv(H_hm),
 * (W,H), INTER_LINEAR, BORDER_REPLICATE);  H_comp <- H_comp @ H_hm.
 *   H_mat[B,9] (what hdn_dlt_solve_f32 / hdn_dlt_warp_f32 returned), search[B,1,H,W] -> warped[B,1,H,W];
 *   H_comp_or_null[B,9] float64, updated in place (start it at the identity).
 * The sampler restates OpenCV's INTER_LINEAR warpPerspective (1/32-pixel source coordinates rounded half-to-even,
 * float32 weights, replicate border); OpenCV is not available to this build, so this entry point is PARITY-UNPINNED: it
 * is held to the oracle's restatement of the same algorithm, not to cv2 output.
 */
int hdn_refine_warp_f32(const float* H_mat, const float* search, float* warped, double* H_comp_or_null, int B, int H,
                        int W, void* stream);

/*
 * sum_i |a[i] - b[i]| * scale over n floats into out[0] (one block, deterministic order).
 * The two feature-distance scores of track_proj, model_builder_e2e_unconstrained_v2.py:213-216.
 */
int hdn_l1_score_f32(const float* a, const float* b, float* out, int n, float scale, void* stream);

/* Both scores of a frame in one launch: out2[j] = sum_i |a[i] - b_j[i]| * scale, j = 0, 1 (bit-identical to two calls
 * of hdn_l1_score_f32). */
int hdn_l1_score2_f32(const float* a, const float* b0, const float* b1, float* out2, int n, float scale, void* stream);

/* The same for B samples in one launch (the lock-step multi-sequence tracker, hdn_amd.batched_tracker): sample s reads its three planes
 * `plane_stride` floats (>= n) after sample s - 1's and writes out[2 s], out[2 s + 1]; every sample's sums run in the order of
 * hdn_l1_score2_f32, so each is bit-identical to its own single call.  The reference scores sample 0 only
 * (model_builder_e2e_unconstrained_v2.py:213-216: `[0][0]`), because its tracker holds one sequence per process. */
int hdn_l1_score2_batch_f32(const float* a, const float* b0, const float* b1, float* out, int n, long long plane_stride, int B, float scale,
                            void* stream);

/*
 * Log-polar resample of the search crop: out[b,c,a,r] = bilinear(img[b,c], p(a,r)) with
 *   g = (rho[r]*cos_theta[a] + polar[b,0], rho[r]*sin_theta[a] + polar[b,1]) / (size//2)   (the reference's grid)
 *   p = PyTorch grid_sample's align_corners=False pixel position, padding_mode='border'.
 * img[B,C,H,W], polar[B,2], rho[S], cos_theta[S], sin_theta[S] -> out[B,C,S,S]; grid_or_null[B,S,S,2] receives g.
 * The three tables are rho[r] = exp(r*log(S/2)/S) - 1 and cos/sin(a*2*pi/S + rot): build them with
 * hdn_amd.logpolar.tables() (host, same ops as the reference) and keep them on the device.
 * Replaces STN_Polar.forward(x, polar, delta), hdn/models/logpolar.py:58-74,100-124
 * (called from ModelBuilder.track_new_lp, model_builder_e2e_unconstrained_v2.py:147).
 */
int hdn_logpolar_sample_f32(const float* img, const float* polar, const float* rho, const float* cos_theta,
                            const float* sin_theta, float* out, float* grid_or_null, int B, int C, int H, int W,
                            int S, void* stream);

/*
 * Backward of the three geometry operators (csrc/geometry_bwd.hip; training only).  Common rules:
 *   - an output pointer that is NULL means that gradient is neither computed nor written; asking for no gradient at all is HDN_E_SHAPE;
 *   - checked before any launch, in this order: an input NULL -> HDN_E_NULL; the forward's shape rules (and "no gradient") -> HDN_E_SHAPE; the
 *     forward's limits -> HDN_E_LIMIT; the workspace, where one is needed (NULL -> HDN_E_NULL, not 16-byte aligned or too small -> HDN_E_LIMIT,
 *     overlapping img or grad_out -> HDN_E_ALIAS); an output equal to an input, the workspace or the other output -> HDN_E_ALIAS;
 *   - every kernel recomputes the forward's sample point with the forward's own statements, so it differentiates through the taps the forward read;
 *   - grad_polar, grad_theta, grad_src and grad_off are DETERMINISTIC: no atomics, a fixed-order reduction in the block (wave shuffles, then LDS),
 *     one partial per (sample, block) in `workspace`, and a second launch of the same call that adds the partials in a fixed order.  Two calls are
 *     bit-equal, and sample b of a batch has the bits of that sample run alone;
 *   - grad_img is a scatter by plain fp32 atomicAdd into the buffer the call zero-fills on `stream`: it is the one output that is NOT
 *     bit-reproducible between calls on arbitrary data (the order in which colliding taps are added is not fixed).  Neither the reference's
 *     `search` (model_builder_e2e_unconstrained_v2.py:379) nor its `org_imgs` (homo_model_builder.py:168) requires grad in training.
 *
 * hdn_logpolar_sample_bwd_f32: the sampler above.  With the forward's clamped pixel position (px, py), w = px - floor(px), e = 1 - w,
 * n = py - floor(py), s = 1 - n, the four taps I_nw, I_ne, I_sw, I_se masked as in the forward (an east / south tap beyond the last index is 0):
 *   d out / d px = s (I_ne - I_nw) + n (I_se - I_sw)
 *   d out / d py = e (I_sw - I_nw) + w (I_se - I_ne)
 *   d px / d polar_x = (W/2) / (H//2),  d py / d polar_y = (H/2) / (W//2)      (the forward's (sic) pairing of x with H//2 and y with W//2)
 * both times PyTorch's border rule (clip_coordinates_set_grad, what F.grid_sample(padding_mode='border') differentiates with): a coordinate the
 * clamp moved has derivative 0, i.e. p <= 0 or p >= size - 1 before clamping.
 *   grad_polar[b] = sum over c, a, r of grad_out[b,c,a,r] (d out / d px d px / d polar_x, d out / d py d py / d polar_y)
 *   grad_img[b,c] += grad_out[b,c,a,r] {s e, s w, n e, n w} at the four taps; masked taps receive nothing.
 * img[B,C,H,W], polar[B,2], the three tables [S], grad_out[B,C,S,S] -> grad_polar[B,2] and/or grad_img[B,C,H,W].
 * workspace: hdn_logpolar_sample_bwd_workspace_bytes(B, S) bytes, 16-byte aligned, needed for grad_polar only (else it may be NULL).
 * Differentiates STN_Polar.forward, hdn/models/logpolar.py:100-124 (training forward: model_builder_e2e_unconstrained_v2.py:377-379).
 */
long long hdn_logpolar_sample_bwd_workspace_bytes(int B, int S);
int hdn_logpolar_sample_bwd_f32(const float* img, const float* polar, const float* rho, const float* cos_theta, const float* sin_theta,
                                const float* grad_out, float* grad_polar_or_null, float* grad_img_or_null, float* workspace,
                                long long workspace_bytes, int B, int C, int H, int W, int S, void* stream);

/*
 * hdn_dlt_solve_bwd_f32: hdn_dlt_solve_f32.  [A|b] is rebuilt as the forward builds it (the reference's point order, dst = src + off as an fp32
 * add), with rows (x, y, 1, 0, 0, 0, -u x, -u y | u) and (0, 0, 0, x, y, 1, -v x, -v y | v) per point.  In float64, by elimination with partial
 * pivoting within an 8-lane group like the forward:
 *   A h = b,   A^T lambda = grad_H[0:8]        (grad_H[8] meets the constant 1 and is ignored)
 *   grad_b = lambda,   grad_A = -lambda h^T
 * pushed through the rows to x, y, u, v; then grad_off = (grad_u, grad_v), grad_src = (grad_x + grad_u, grad_y + grad_v), in the caller's point
 * order, each rounded to fp32 once.
 * src[B,8], off[B,8], grad_H[B,9] -> grad_src[B,8] and/or grad_off[B,8].
 * Differentiates DLT_solve, .../Oneline_DLTv1/utils.py:7-67 (training forward: homo_model_builder.py:166).
 */
int hdn_dlt_solve_bwd_f32(const float* src, const float* off, const float* grad_H, float* grad_src_or_null, float* grad_off_or_null, int B,
                          void* stream);

/*
 * hdn_warp_bwd_f32: hdn_warp_f32.  x, y, the clamped taps x0, x1, y0, y1 and Ia = img[y0][x0], Ib = img[y1][x0], Ic = img[y0][x1],
 * Id = img[y1][x1] are the forward's.  What the reference's autograd differentiates: the integer taps are constants, the nudge has derivative 1.
 *   d out / d x = (Ic - Ia)(y1 - y) + (Id - Ib)(y - y0)
 *   d out / d y = (Ib - Ia)(x1 - x) + (Id - Ic)(x - x0)
 *   d x / d xs = W/2,  d y / d ys = H/2;   xs = T0 / t:  d xs / d T0 = 1 / t,  d xs / d t = -xs / t  (ys likewise)
 *   T_r = theta[3r] gx + theta[3r+1] gy + theta[3r+2]
 *   grad_theta[b] = the nine sums over the H W C terms of sample b
 *   grad_img[b,c] += grad_out {wa, wb, wc, wd} at (y0,x0), (y1,x0), (y0,x1), (y1,x1); coinciding clamped taps simply add.
 * img[B,C,H,W], theta[B,9], grad_out[B,H,W,C] (NHWC, the forward's output layout) -> grad_theta[B,9] and/or grad_img[B,C,H,W].
 * workspace: hdn_warp_bwd_workspace_bytes(B, H, W) bytes, 16-byte aligned, needed for grad_theta only (else it may be NULL).
 * Differentiates transformer, .../Oneline_DLTv1/utils.py:70-254 (training forward: homo_model_builder.py:168).
 */
long long hdn_warp_bwd_workspace_bytes(int B, int H, int W);
int hdn_warp_bwd_f32(const float* img, const float* theta, const float* grad_out, float* grad_theta_or_null, float* grad_img_or_null,
                     float* workspace, long long workspace_bytes, int B, int C, int H, int W, void* stream);

/*
 * Affine spatial transformer (csrc/affine_stn.hip): out[b,c,i,j] = bilinear(img[b,c], p(i,j)) where p is what F.affine_grid(theta, size) followed
 * by F.grid_sample with PyTorch's defaults (mode='bilinear', padding_mode='zeros', align_corners=False) samples; the grid is never materialised.
 *   X_j = (2j+1)/Wo - 1,  Y_i = (2i+1)/Ho - 1
 *   gx = t00 X_j + t01 Y_i + t02,   gy = t10 X_j + t11 Y_i + t12            (t = theta[b])
 *   px = ((gx+1) W - 1)/2,          py = ((gy+1) H - 1)/2
 *   x0 = floor(px), y0 = floor(py), w = px - x0, n = py - y0
 *   out = (1-n)(1-w) I_nw + (1-n) w I_ne + n (1-w) I_sw + n w I_se          a tap outside [0,W) x [0,H) reads 0
 * px, py, x0, y0 and the differences px - x0, py - y0 are formed in float64 from the fp32 theta (every operation rounded on its own, in the order
 * written) and w, n, e = 1 - w, s = 1 - n each rounded to fp32 once: an fp32 px of size 100 would leave a bilinear weight 1e-5 of absolute error.
 * The blend is fp32, every operation rounded on its own: out = ((I_nw (s e) + I_ne (s w)) + I_sw (n e)) + I_se (n w).  Guard: a sample whose px is not strictly inside (-1, W) or whose
 * py is not strictly inside (-1, H) - NaN, +-inf and values beyond any int included - gives out = 0 and contributes to no gradient; the decision is
 * a float comparison made before any conversion to an integer and before any address is formed (PyTorch's zeros padding gives 0 for a finite position outside too).
 * img[B,C,H,W], theta[B,2,3] -> out[B,C,Ho,Wo], all fp32 contiguous.  Checked before the launch, in this order: a NULL pointer -> HDN_E_NULL; a size
 * <= 0 -> HDN_E_SHAPE; B > 65535, H W or Ho Wo > 2^30 -> HDN_E_LIMIT; out equal to img or theta -> HDN_E_ALIAS.
 * Replaces ModelBuilder.stn_with_theta(x, theta, size), model_builder_e2e_unconstrained_v2.py:233-237 (training forward: :407, :408, :418).
 */
int hdn_affine_sample_f32(const float* img, const float* theta, float* out, int B, int C, int H, int W, int Ho, int Wo, void* stream);

/*
 * hdn_affine_sample_bwd_f32: the sampler above, under the common rules of the geometry backwards (see hdn_logpolar_sample_bwd_f32 above): a NULL
 * output is not computed and asking for no gradient is HDN_E_SHAPE; the checks run in the same order (NULL, shape, limit, workspace, alias); the
 * sample point, the guard included, is recomputed by the forward's own statements (one __device__ function shared by both kernels); grad_theta is
 * DETERMINISTIC (no atomics, fixed-order block reduction by wave shuffles then LDS, one partial of six floats per (sample, block) in `workspace`, a
 * second launch of the same call adds the partials in a fixed order: two calls are bit-equal and sample b of a batch has the bits of that sample run
 * alone); grad_img is an fp32 atomicAdd scatter into the buffer the call zero-fills on `stream` and is NOT bit-reproducible between calls.
 * With the forward's w, n and the four taps (a tap outside the plane is 0; zeros padding has no clip mask):
 *   d out / d px = (1-n)(I_ne - I_nw) + n (I_se - I_sw)
 *   d out / d py = (1-w)(I_sw - I_nw) + w (I_se - I_ne)
 *   d px / d gx = W/2,  d py / d gy = H/2
 *   grad_theta[b,0,:] = sum over c, i, j of grad_out[b,c,i,j] d out / d px (W/2) (X_j, Y_i, 1)
 *   grad_theta[b,1,:] = sum over c, i, j of grad_out[b,c,i,j] d out / d py (H/2) (X_j, Y_i, 1)
 *   grad_img[b,c] += grad_out[b,c,i,j] {(1-n)(1-w), (1-n) w, n (1-w), n w} at the four taps; outside taps receive nothing.
 * A guarded sample (see the forward) contributes 0 to both.
 * img[B,C,H,W], theta[B,2,3], grad_out[B,C,Ho,Wo] -> grad_theta[B,2,3] and/or grad_img[B,C,H,W].  Limits: the forward's.
 * workspace: hdn_affine_sample_bwd_workspace_bytes(B, Ho, Wo) bytes (B ceil(Ho Wo / 256) partials of 24 bytes; negative = HDN_E_*), 16-byte aligned,
 * needed for grad_theta only (else it may be NULL).
 * Differentiates ModelBuilder.stn_with_theta; two of the step's three calls take affine_m, which carries sim_loss and homo_unsup_loss to both heads.
 */
long long hdn_affine_sample_bwd_workspace_bytes(int B, int Ho, int Wo);
int hdn_affine_sample_bwd_f32(const float* img, const float* theta, const float* grad_out, float* grad_theta_or_null, float* grad_img_or_null,
                              float* workspace, long long workspace_bytes, int B, int C, int H, int W, int Ho, int Wo, void* stream);

/*
 * L1 triplet margin loss over rows (csrc/triplet_loss.hip): what nn.TripletMarginLoss(margin, p=1, eps, swap=False, reduction='none') computes on
 * three [N,R,D] tensors, one loss per row, with the x[ids] gather of the reference's two call sites folded into the addressing.  Per row, in fp32:
 *   d_ap = sum_j |(a_j - p_j) + eps|,   d_an = sum_j |(a_j - n_j) + eps|
 *   v = (margin + d_ap) - d_an
 *   loss = v if v >= 0, 0 if v < 0
 * The subtraction is rounded, then the add of eps (F.pairwise_distance's two elementwise operations); eps is inside the absolute value.  A NaN v
 * stays NaN (clamp_min's rule, not fmaxf's).  The sums are taken by one wave: lane l adds the elements l, l + 64, ... in ascending order, a xor
 * butterfly adds the 64 lanes; the order is fixed, so two calls are bit-equal.
 * anchor, positive, negative [N,R,D] fp32 contiguous, 4-byte aligned (every access is one dword); the three may alias each other.  ids: NULL, or
 * n_ids sample indices (int64, 8-byte aligned, unique, as nonzero() gives them): row r of `loss` is then row r % R of sample ids[r / R].
 * loss [n_sel R], n_sel = n_ids with ids, N without.  An ids entry outside [0, N) is checked before any address is formed: nothing is read for it
 * and its R loss rows are NaN.
 * Checked before the launch, in this order: anchor, positive, negative or loss NULL -> HDN_E_NULL; N, R or D <= 0, or ids with n_ids <= 0 ->
 * HDN_E_SHAPE; N R > 2^30, n_ids R > 2^30 or D > 2^20 -> HDN_E_LIMIT; the byte range of loss overlapping an input's or ids' -> HDN_E_ALIAS.
 * Replaces triplet_loss(...) at model_builder_e2e_unconstrained_v2.py:438 and homo_model_builder.py:197 (with the gathers of :428-436 / :185-187).
 */
int hdn_triplet_l1_f32(const float* anchor, const float* positive, const float* negative, const long long* ids_or_null, float* loss,
                       int N, int R, int D, int n_ids, float margin, float eps, void* stream);

/*
 * hdn_triplet_l1_bwd_f32: the gradients of the loss above for grad_loss [n_sel R] = d L / d loss.  v is recomputed by the forward's own device
 * function, so the bits are the forward's.  A row is active iff v >= 0 (clamp_min's rule: the gradient passes at exactly 0, not at NaN).
 * With g = grad_loss[row], s_ap = sgn((a - p) + eps), s_an = sgn((a - n) + eps), sgn(0) = 0, per element of an active row:
 *   grad_a = g (s_ap - s_an),   grad_p = -g s_ap,   grad_n = g s_an
 * and 0 in a row that is not active.  g {0, +-1, +-2} is exact: every gradient is exact given the row's activity.
 * grad_a, grad_p, grad_n are full size [N,R,D]; with ids, the rows of samples that ids does not name are zero, written by this call (no zero-fill
 * is needed before it), and an ids entry outside [0, N) names no sample.  A NULL gradient is neither computed nor written; all three NULL is
 * HDN_E_SHAPE.  One wave per gradient row writes every element exactly once: no atomics, bit-reproducible.  (A wave finds its sample in ids by
 * scanning the list, the lowest position wins: n_ids / 64 steps per row.)
 * Checked in the forward's order: an input or grad_loss NULL -> HDN_E_NULL; the forward's shape rules and "no gradient asked for" -> HDN_E_SHAPE;
 * the forward's limits -> HDN_E_LIMIT; the byte range of a gradient overlapping an input's, ids', grad_loss's or another gradient's -> HDN_E_ALIAS.
 */
int hdn_triplet_l1_bwd_f32(const float* anchor, const float* positive, const float* negative, const long long* ids_or_null, const float* grad_loss,
                           float* grad_a_or_null, float* grad_p_or_null, float* grad_n_or_null, int N, int R, int D, int n_ids, float margin,
                           float eps, void* stream);

/*
 * hdn_triplet_l1_mean_f32: the flag-selected mean of the loss rows above, the two triplet terms of the training forwards with their nonzero()
 * selections and host-read divisors decided in the kernels (csrc/triplet_loss.hip); nothing is read by the host.  anchor, positive, negative
 * [N,R,D], if_pos, if_unsup [N], all fp32 -> out [1] fp32, counts [2] int32 = n_sel, n_neg.  partial: N R floats of scratch, supplied by the caller.
 *   The sets, float comparisons as .eq() makes them (a flag of 0.5 or NaN fails both):  sel: fp32(if_pos[b] if_unsup[b]) == 1;  neg: if_pos[b] == 0.
 *   loss(b, r) = the row loss of hdn_triplet_l1_f32, computed by the same device function (the decision v >= 0 is made on the same bits).
 *   S = sum of loss(b, r) over the rows of the used samples.
 *   rule 0 (similarity model, model_builder_e2e_unconstrained_v2.py:430-440):  used = sel;  out = (S / denom) / n_sel
 *   rule 1 (homography estimator, homo_model_builder.py:174-199):  used = sel where n_neg > 0, every sample where n_neg == 0;
 *          out = (S / n_sel) / denom.  The divisor is n_sel in both cases: with no negative in the batch the reference sums every sample and
 *          still divides by the number of selected ones (its own quirk, kept).
 *   Empty selection: n_sel == 0 gives out = 0 and, in the backward, zero gradients, and nothing is read.  This differs from the reference on
 *   purpose: it skips the term under rule 0 and divides by zero under rule 1 (a batch whose unsupervised samples are all negative makes its
 *   total_loss NaN); a kernel cannot skip, and a caller that gates with torch.where passes a zero upstream gradient, which must not become 0 inf.
 *   The data of a sample that is not used is not read: a NaN there reaches nothing.  S is summed in an order fixed by (N, R) alone (a row per
 *   wave into partial, then one workgroup: thread t adds partial[t], partial[t + 1024], ..., a xor tree adds a wave's lanes, the sixteen waves
 *   are added in ascending order): no float atomics, two calls are bit-equal.  Two launches on `stream`.
 * hdn_triplet_l1_mean_bwd_f32: grad_out [1] -> grad_a, grad_p, grad_n [N,R,D]; each may be NULL (not all).  The sets are recounted from the flags.
 *   Every element is written exactly once: rows of unused samples and inactive rows (v < 0 or NaN) are 0; an element of an active row is c k with
 *   k = s_ap - s_an, -s_ap, s_an {0, +-1, +-2} as in hdn_triplet_l1_bwd_f32 and ONE fp32 factor per call, in the rule's order:
 *   rule 0: c = (grad_out / denom) / n_sel;  rule 1: c = (grad_out / n_sel) / denom.  First order only; the flags get no gradient.
 * Checked before the launch, in this order: a required pointer NULL -> HDN_E_NULL; N, R or D <= 0, rule outside {0, 1}, denom not > 0, or no
 * gradient asked for -> HDN_E_SHAPE; N > 65536, N R > 2^30 or D > 2^20 -> HDN_E_LIMIT; the byte range of an output (partial, out, counts, a
 * gradient) overlapping an input's, grad_out's or another output's -> HDN_E_ALIAS.  The three inputs may alias each other.
 */
int hdn_triplet_l1_mean_f32(const float* anchor, const float* positive, const float* negative, const float* if_pos, const float* if_unsup,
                            float* partial, float* out, int* counts, int N, int R, int D, int rule, float denom, float margin, float eps,
                            void* stream);
int hdn_triplet_l1_mean_bwd_f32(const float* anchor, const float* positive, const float* negative, const float* if_pos, const float* if_unsup,
                                const float* grad_out, float* grad_a_or_null, float* grad_p_or_null, float* grad_n_or_null, int N, int R, int D,
                                int rule, float denom, float margin, float eps, void* stream);

/*
 * The similarity model's supervised head losses (csrc/sup_losses.hip): up to five scalar losses of hdn/models/loss.py in one launch, one workgroup
 * per loss, as model_builder_e2e_unconstrained_v2.py:457-478 and :516-523 use them (WEIGHTED_MAP_LP: False).  All selection - the sample mask, the
 * label predicates, the label maximum, the counts, the top-k - happens in the kernel: no nonzero(), no host read, capturable in a graph.
 * "selected" below means: label predicate AND sample selected.  losses [5] receives (a) .. (e) at index 0 .. 4; a loss whose pointers are all NULL is
 * skipped and its entry is not written.
 *
 * (a) select_xr_focal_fuse_smooth_l1_loss_top_k: cls + label_cls (float [n,S,S]); p1 = the class-1 probability.
 *   pos = sum{label > 0} |label - p1| / (n_pos + 1)
 *   l = -log(1 - clamp(p1, 0.000001f, 0.9999999f)) over the cells with label == 0
 *   neg = (sum of the k_eff largest l) / (k_eff + 1),  k = topk_per_sample n,  k_eff = min(k, n_neg)
 *   loss = pos + neg
 *   The k-th largest l, t, is found by a radix select on the bit patterns (l > 0); the sum is sum{l > t} + (k_eff - count_gt) t.  Where the reference
 *   raises (fewer negatives than k) k_eff is used instead: a kernel cannot raise without a host read.  Python passes topk_per_sample = 100.
 * (b) select_l1_loss_c: loc, label_loc_c [n,2,S,S] + label_cls.  max_c = the largest label_cls of the selected samples; cells: label > max_c - 0.2f;
 *   loss = sum over the cells and both channels of smooth(pred - target) / (2 n_sel + 1),  smooth(d) = 0.5 d^2 if |d| < 1, |d| - 0.5 otherwise
 *   A NaN label makes max_c NaN (torch.max), which selects nothing.  Labels that are all negative select every cell within 0.2 of their maximum.
 * (c) select_cross_entropy_loss: cls_lp + label_cls_lp (int64 [n,S',S']);
 *   loss = 0.5 mean{label == 1}(-logp1) + 0.5 mean{label == 0}(-logp0)
 * (d) select_l1_loss: loc_lp, label_loc_lp [n,4,S',S'] + label_cls_lp; cells: label > 0;  loss = sum smooth(pred - target) / (4 n_sel + 1)
 * (e) kalyo_l1_loss: rows, rows_target [n_rows,C], every row;  loss = sum smooth(rows - target) / (n_rows C + 1)
 * The one-hit rule (the reference's nonzero().squeeze() turns one hit into a 0-d tensor, which its emptiness test takes for empty): with exactly
 * one selected cell the term is 0 in (a) pos, (a) neg, (b) and both terms of (c); not in (d), where one row gives the ordinary value.  With no
 * selected cell every term is 0.  A NaN in a selected prediction makes that loss NaN.
 *
 * form 0: the raw head maps cls [B,2,S,S], loc [B,2,S,S], cls_lp [B,2,S',S'], loc_lp [B,4,S',S']; F.softmax for (a) and F.log_softmax for (c) are
 *   folded in, evaluated as PyTorch does: exp(x - max) / sum and (x - max) - log(sum exp(x - max)), with expf / logf (not the fast intrinsics).
 *   if_unsup [B] (float, may be NULL = every sample): sample b is selected iff if_unsup[b] == 0; n is counted in the kernel.  No sample selected:
 *   every loss is 0.
 * form 1: what the reference's functions receive: cls / cls_lp [n,S,S,2] already softmaxed / log-softmaxed, B = n, if_unsup NULL.
 * Every sum has a fixed order (thread t adds the cells t, t + 1024, ... ascending; a xor butterfly; the 16 wave sums in order): no float atomics,
 * every output is bit-reproducible.  Integer LDS histograms only.
 * Checked before the launch, in this order: losses NULL, a loss with some but not all of its pointers, or no loss at all -> HDN_E_NULL; form not 0
 * or 1, if_unsup with form 1, B, S, S_lp, n_rows, C or topk_per_sample <= 0 where a present loss uses it -> HDN_E_SHAPE; B S^2 or B S_lp^2 > 40000
 * (64 x 25 x 25: the l of (a) live in LDS), n_rows C > 2^20 -> HDN_E_LIMIT; losses overlapping an input -> HDN_E_ALIAS.
 */
int hdn_sup_losses_f32(const float* cls, const float* label_cls, const float* loc, const float* label_loc_c, const float* cls_lp,
                       const long long* label_cls_lp, const float* loc_lp, const float* label_loc_lp, const float* rows, const float* rows_target,
                       const float* if_unsup_or_null, float* losses, int B, int S, int S_lp, int n_rows, int C, int topk_per_sample, int form,
                       void* stream);

/*
 * hdn_sup_losses_bwd_f32: the gradients of the losses above for grad_losses [5] = d L / d losses, one launch.  Every selection is repeated by the
 * forward's own device functions, so the decisions are made on the forward's bits.  A gradient pointer that is NULL is neither computed nor written;
 * the others are written in full (zero where nothing is selected, zero rows for unselected samples: no zero-fill is needed before the call).
 * (a) positives: g sgn(p1 - label) / (n_pos + 1), sgn(0) = 0.  Negatives: every cell with l > t, and among the cells with l == t the lowest flat
 *     indices (b S^2 + cell) until k_eff are reached - torch.topk's own choice among ties is unspecified - receive g / ((k_eff + 1)(1 - p1)) where
 *     0.000001f <= p1 <= 0.9999999f (clamp passes the gradient on its closed interval) and 0 outside.  form 0: grad x1 = gp p1 p0, grad x0 = -grad x1;
 *     form 1: channel 1 receives gp, channel 0 is written as zero.
 * (b), (d), (e): g (d if |d| < 1, sgn(d) otherwise) / (C n_sel + 1), d = pred - target, on the selected cells.
 * (c) a_1 = -0.5 g / n_1 on label == 1, a_0 = -0.5 g / n_0 on label == 0; form 1: written to those channels; form 0: grad x_j = a_j - softmax_j (a_0 + a_1).
 * A term that the one-hit rule makes 0 has gradient 0.
 * Checked in the forward's order: grad_losses NULL, or a gradient asked for a loss whose inputs are missing -> HDN_E_NULL (with the forward's NULL
 * rules); the forward's shape rules and "no gradient asked for" -> HDN_E_SHAPE; the forward's limits -> HDN_E_LIMIT; a gradient overlapping an
 * input, grad_losses or another gradient -> HDN_E_ALIAS.
 */
int hdn_sup_losses_bwd_f32(const float* cls, const float* label_cls, const float* loc, const float* label_loc_c, const float* cls_lp,
                           const long long* label_cls_lp, const float* loc_lp, const float* label_loc_lp, const float* rows,
                           const float* rows_target, const float* if_unsup_or_null, const float* grad_losses, float* grad_cls_or_null,
                           float* grad_loc_or_null, float* grad_cls_lp_or_null, float* grad_loc_lp_or_null, float* grad_rows_or_null, int B, int S,
                           int S_lp, int n_rows, int C, int topk_per_sample, int form, void* stream);

/*
 * The similarity model's training geometry between the head maps and the samplers (model_builder_e2e_unconstrained_v2.py:377, :390-415), csrc/simi_geometry.hip.
 * fp32 throughout, every operation individually rounded (no contraction), no atomics, no host read; argmax order: csrc/argmax_order.h (NaN first, the
 * larger value, the lower index).  n = S S; point(i) = (ori + stride (i % S), ori + stride (i / S)), ori = -(S / 2) stride, as generate_points(stride, S).
 *
 * hdn_point_pick_f32: one wave per sample.  cls [B,2,S,S], loc [B,2,S,S] (mode 0) or [B,4,S,S] (mode 1), best_idx int32 [B].
 *   mode 0 (Polar_Pick.get_polar_from_two_para_loc, logpolar.py:304-324): best = argmax_i cls[b,1,i]; out [B,2]: out[b,c] = point_c(best) - mult loc[b,c,best].
 *   mode 1 (lp_pick, point.py:35-53): best = argmax_i softmax2_class1(cls[b,0,i], cls[b,1,i]); out [2,B]: out[0,b] = scale =
 *          expf((px - mult loc[b,0,best]) (float)mag), out[1,b] = rot = (py - mult loc[b,2,best]) (float)rot_unit.
 * hdn_point_pick_bwd_f32: grad_loc (the shape of loc), every element written: zero, except [b,c,best] = -grad_out[b,c] mult (mode 0), [b,0,best] =
 *   -((grad_out[0,b] out[0,b]) mag) mult and [b,2,best] = -(grad_out[1,b] rot_unit) mult (mode 1; `out` is the forward's, unused in mode 0).  A best_idx
 *   outside [0, n) gives a zero row.
 * cls_channels != 2, B < 1, S < 1, stride < 1, a mode that is not 0 or 1 -> HDN_E_SHAPE; S > 1024 or stride > 4096 -> HDN_E_LIMIT; a NULL pointer -> HDN_E_NULL.
 */
int hdn_point_pick_f32(const float* cls, const float* loc, float* out, int* best_idx, int B, int S, int cls_channels, int mode, int stride, float mult,
                       double mag, double rot_unit, void* stream);
int hdn_point_pick_bwd_f32(const int* best_idx, const float* grad_out, const float* out_or_null, float* grad_loc, int B, int S, int mode, float mult,
                           double mag, double rot_unit, void* stream);

/*
 * hdn_simi_affine_f32: out [B,2,3] = [[a, -c, t0], [c, a, t1]], a = sc cosf(rot), c = sc sinf(rot), t0 = ((-a U - (-c) V) + W0) [/ out_sz],
 * t1 = ((-c U - a V) + W1) [/ out_sz]; one thread per sample.  nm_shift [B,2], scale, rot [B]; cx, cy [B] or both NULL (then the scalars are used).
 *   kind 0 (combine_affine_c0_v2, transform.py:442): sc = (float)(out_sz / in_sz) scale, U = (cx - out_sz / 2) in_sz / out_sz (fp32 steps for a vector,
 *          double then rounded for the scalar), V likewise from cy, W = nm_shift, the division iff scale_h.
 *   kind 1 (combine_affine_lt0, transform.py:486): sc = scale, U = nm_shift[b,0] + in_sz / 2, V = nm_shift[b,1] + in_sz / 2, W = (cx, cy), no division.
 * hdn_simi_affine_bwd_f32: grad [B,2,3] -> the gradients of nm_shift [B,2], scale [B], rot [B]; each may be NULL (not all).
 * B < 1, a kind that is not 0 or 1, in_sz or out_sz not positive, no gradient asked for -> HDN_E_SHAPE; exactly one of cx, cy NULL, or a NULL required pointer -> HDN_E_NULL.
 */
int hdn_simi_affine_f32(const float* nm_shift, const float* scale, const float* rot, const float* cx_or_null, const float* cy_or_null, double cx_scalar,
                        double cy_scalar, float* out, int B, int kind, int scale_h, double in_sz, double out_sz, void* stream);
int hdn_simi_affine_bwd_f32(const float* nm_shift, const float* scale, const float* rot, const float* cx_or_null, const float* cy_or_null,
                            double cx_scalar, double cy_scalar, const float* grad, float* grad_nm_shift_or_null, float* grad_scale_or_null,
                            float* grad_rot_or_null, int B, int kind, int scale_h, double in_sz, double out_sz, void* stream);

/*
 * hdn_simi_warps_f32: model_builder_e2e_unconstrained_v2.py:390-415 in one launch, one wave per sample.  cls_lp [B,2,S,S], loc_lp [B,4,S,S], polar [B,2],
 * temp_cx, temp_cy [B], search_poly [B,4,2] ->
 *   best_idx int32 [B], scale, rot [B]          mode 1 of hdn_point_pick_f32 with mult = stride_lp
 *   affine_m          kind 0 (out_sz / 2, out_sz / 2, polar, scale, rot, scale_h)          affine_m_c_aug    kind 0 (temp_cx, temp_cy, 0, 1, 0, scale_h)
 *   affine_m_lt0      kind 1 (out_sz / 2, out_sz / 2, polar, 1 / scale, -rot)              affine_m_lt0_aug  kind 1 (temp_cx, temp_cy, 0, 1, 0)      each [B,2,3]
 *   pred_points [B,3,4] = [affine_m_lt0; 0 0 1] [x; y; 1] of the four corners of search_poly, aug_sear_points likewise from affine_m_lt0_aug
 *   (a row is (m0 x + m1 y) + m2 1).
 * hdn_simi_warps_bwd_f32: upstream gradients of scale, rot [B], affine_m, affine_m_lt0 [B,2,3], pred_points [B,3,4] (each may be NULL = zero) ->
 *   grad_loc_lp [B,4,S,S] (every element written) and grad_polar [B,2]; each may be NULL (not both).  best_idx, scale, rot are the forward's.
 * Error rules of hdn_point_pick_f32 and hdn_simi_affine_f32.
 */
int hdn_simi_warps_f32(const float* cls_lp, const float* loc_lp, const float* polar, const float* temp_cx, const float* temp_cy,
                       const float* search_poly, int* best_idx, float* scale, float* rot, float* affine_m, float* affine_m_lt0, float* affine_m_c_aug,
                       float* affine_m_lt0_aug, float* pred_points, float* aug_sear_points, int B, int S, int cls_channels, int stride, float stride_lp,
                       double mag, double rot_unit, double in_sz, double out_sz, void* stream);
int hdn_simi_warps_bwd_f32(const int* best_idx, const float* scale, const float* rot, const float* polar, const float* search_poly,
                           const float* grad_scale_or_null, const float* grad_rot_or_null, const float* grad_affine_m_or_null,
                           const float* grad_affine_m_lt0_or_null, const float* grad_pred_points_or_null, float* grad_loc_lp_or_null,
                           float* grad_polar_or_null, int B, int S, float stride_lp, double mag, double rot_unit, double in_sz, double out_sz,
                           void* stream);

/*
 * hdn_corner_losses_f32: the corner supervision of model_builder_e2e_unconstrained_v2.py:441-444, :481-523 and :552-556 in one launch (one workgroup;
 * a sample on eight lanes), nothing read by the host.  H_mat [B,3,3], pred_points [B,3,4] (rows x, y, w), aug_sear_points [B,3,4] or NULL,
 * template_poly [B,4,2], x [B,8] (batch_out['x']), if_pos, if_unsup [B], all fp32 -> out [6] fp32, counts [6] int32.
 *   The sets, float comparisons as .eq() makes them (a flag that is neither 0 nor 1 fails them): sup: if_unsup == 0; sup_pos: if_unsup == 0 and
 *   if_pos == 1; sup_neg: if_unsup == 0 and if_pos == 0; unsup: if_unsup == 1; unsup_pos: if_pos if_unsup == 1; neg: if_pos == 0.
 *   counts = n_sup, n_sup_pos, n_sup_neg, n_unsup, n_unsup_pos, n_neg.   c_j = column j of [[0,0],[0,127],[127,127],[127,0]].
 *   out[0] cor_err      = (sum over sup_pos, j, xy of |P_xy / P_w - template_poly|) / n_sup_pos / 4,  P = H_mat[b] pred_points[b]
 *   out[1] cor_err_aug  = the same sum of |aug_sear_points[b][0:2] - template_poly| (no division by w); 0 when the pointer is NULL
 *   out[2] cor_err_sim  = (sum over unsup_pos of |pred_points[b][0:2] - template_poly|) / n_unsup_pos / 4 (no division by w)
 *   out[3] cor_pos_loss = (sum over sup_pos and r < 8 of k(delta[b][r] - x[b][r])) / (8 n_sup_pos + 1), k(d) = d d / 2 where |d| < 1, else |d| - 1/2;
 *          off = pred_points_xy / pred_points_w - template_poly (fp32), H_gt = the system and elimination of hdn_dlt_solve_f32 on
 *          (template_poly[b], off) in float64, rounded to fp32 once, Q = H_gt [c_j; 1], delta[b][2 j + c] = Q_c / Q_w - c_j[c]
 *   out[4] cor_neg_loss = (sum over neg - supervised or not - of k(-x[b][r])) / (8 n_neg + 1) where n_sup_neg > 0, else 0 (the reference computes it
 *          over every negative and reports it with a supervised one)
 *   out[5] cor_loss     = out[3] + out[4]
 *   An empty set gives 0.  A sample contributes to a term only through the sets above; its data is not read for the others.  Sums have a fixed
 *   order: the outputs are bit-reproducible.  Unlike the reference, whose DLT_solve inverts every sample of the batch (torch.inverse raises for the
 *   whole batch on one singular system), only the sup_pos samples are solved here.
 * hdn_corner_losses_bwd_f32: grad_out [6] -> grad_H_mat [B,3,3], grad_pred_points [B,3,4] (the w row included), grad_aug_sear_points [B,3,4],
 *   grad_x [B,8]; each may be NULL (not all).  Every element is written, rows of samples outside the sets are 0.  abs'(0) = 0, |d| = 1 takes the
 *   linear branch; the path through H_gt is the adjoint solve of hdn_dlt_solve_bwd_f32, recomputed from the inputs.  First order only;
 *   template_poly and the flags get no gradient.
 * B < 1 or no gradient asked for -> HDN_E_SHAPE; B > 65536 -> HDN_E_LIMIT; a NULL required pointer, or grad_aug_sear_points without
 * aug_sear_points -> HDN_E_NULL; nothing is launched then.
 */
int hdn_corner_losses_f32(const float* H_mat, const float* pred_points, const float* aug_sear_points_or_null, const float* template_poly,
                          const float* x, const float* if_pos, const float* if_unsup, float* out, int* counts, int B, void* stream);
int hdn_corner_losses_bwd_f32(const float* H_mat, const float* pred_points, const float* aug_sear_points_or_null, const float* template_poly,
                              const float* x, const float* if_pos, const float* if_unsup, const float* grad_out, float* grad_H_mat_or_null,
                              float* grad_pred_points_or_null, float* grad_aug_sear_points_or_null, float* grad_x_or_null, int B, void* stream);

/*
 * The optimizer stretch of a training iteration, tools/train.py:271-281 of the reference (is_valid_number(loss), clip_grad_norm_(10),
 * Adam(amsgrad=True).step()), with nothing read by or uploaded from the host (csrc/opt_step.hip).  The three calls are made in this order on one
 * stream.  `grads`, `params` and `numel` are HOST arrays of n entries; the device pointers in them travel to the kernels by value, at most
 * hdn_opt_tensors_per_launch() tensors per launch (every launch's arguments stay within 4 KB), so a gradient allocated inside a graph capture is
 * served; a NULL gradient is a tensor without a gradient in this step.  A launch's work items are chunks of hdn_opt_chunk() elements.
 *
 * hdn_grad_sqnorm_f32: partials[j] (float64) = the sum of squares of chunk j, chunks counted through the tensors in order, ceil(numel / chunk) per
 *   tensor whether it has a gradient or not (0 then): hdn_grad_sqnorm_partials(numel, n) of them, a layout the sizes alone decide.  One writer per
 *   partial, float64 accumulation in a fixed order, no atomics.
 * hdn_opt_gate_f32: one workgroup.  norm = sqrt(the partials added in a fixed order, float64).  ctrl (four 32-bit words):
 *     ctrl[0] status (int32): 1 when loss is given and isnan(loss) or isinf(loss) or loss > loss_limit (train.py:220-221: -inf is rejected, a loss
 *             equal to the limit is not); else 2 when norm is not finite; else 0
 *     ctrl[1] grad_norm = (float)norm, before clipping       ctrl[2] clip_coef = (float)min(1, max_norm / (norm + 1e-6)), 1 when clip == 0
 *   and, only when status == 0, for every tensor i with a gradient: steps[i] += 1 (fp32), coef[i] = (float)(lr[group[i]] / (1 - beta1^t)),
 *   coef[n + i] = (float)(1 / sqrt(1 - beta2^t)), t = the new steps[i], in float64.  lr (float64, one per group), group (int32 [n]), steps and coef
 *   are device arrays; lr is read when the kernel runs.  n may be 0 (the norm alone); n <= 28672.
 * hdn_amsgrad_apply_f32: returns after reading ctrl[0] when it is not 0 (no byte is written).  Else per element of every tensor with a gradient,
 *   each operation rounded to fp32 on its own, sqrt and / correctly rounded, c = ctrl[2]:
 *     g' = c g;  ge = g' + wd p;  m = b1 m + (1 - b1) ge;  v = b2 v + ((1 - b2) ge) ge;  vmax = max(vmax, v);
 *     p = p - (coef[i] m) / (sqrt(vmax) coef[n + i] + eps);   write_grads != 0: g = g' (what clip_grad_norm_ leaves behind)
 *   The moments are three flat buffers of state_floats >= hdn_opt_state_floats(numel, n) floats, 16-byte aligned; tensor i's slot starts at the sum
 *   of the earlier sizes, each rounded up to a multiple of 4.  16-byte loads and stores where p and g are 16-byte aligned, a scalar path for the
 *   last numel % 4 elements and for a misaligned view.  Bit-reproducible.
 * Checked before any launch: a required pointer NULL (a parameter included) -> HDN_E_NULL; n < 0, a negative size, clip with max_norm not > 0, a
 * beta outside [0, 1) -> HDN_E_SHAPE; a size above 2^40, too few partials or state floats, a misaligned pointer, n above the gate's limit ->
 * HDN_E_LIMIT; a gradient overlapping its parameter -> HDN_E_ALIAS.  The two size queries are host only; negative = HDN_E_*.
 */
int hdn_opt_tensors_per_launch(void);
int hdn_opt_chunk(void);
long long hdn_grad_sqnorm_partials(const long long* numel, int n);
long long hdn_opt_state_floats(const long long* numel, int n);
int hdn_grad_sqnorm_f32(const float* const* grads, const long long* numel, int n, double* partials, long long n_partials, void* stream);
int hdn_opt_gate_f32(const double* partials, long long n_partials, const float* loss_or_null, float loss_limit, int clip, double max_norm,
                     const double* lr, const int* group, const float* const* grads, int n, double beta1, double beta2, float* ctrl, float* steps,
                     float* coef, void* stream);
int hdn_amsgrad_apply_f32(float* const* params, float* const* grads, const long long* numel, int n, float* exp_avg, float* exp_avg_sq,
                          float* max_exp_avg_sq, long long state_floats, const float* ctrl, const float* coef, double beta1, double beta2,
                          double eps, double weight_decay, int write_grads, void* stream);

/*
 * Device-resident frame handling: the uint8 frame [H,W,C] (HWC, BGR as cv2.imread delivers it) is
 * uploaded once; crops and warps are kernels.  `params` / `M` are DEVICE float64 arrays so that positions and homographies
 * produced on the device never visit the host.
 *
 * hdn_subwindow_f32: params = [cx, cy, original_sz, avg_chans[0..C)]; the P x P patch around (cx, cy) with
 *   uint8(avg_chans) outside the frame, resized to model_sz x model_sz (restated cv2.resize, INTER_LINEAR) when P != model_sz;
 *   mode 0: out[C, model_sz, model_sz] float32 (uint8-valued);  mode 1 (C = 3): out[model_sz, model_sz] = mean over channels of
 *   (x - [118.93,113.97,102.60]) / [69.85,68.81,72.45] in float64, i.e. get_search_info / get_template_info fused in.
 *   Replaces SiameseTracker.get_subwindow / get_subwindow_for_homo, hdn/tracker/base_tracker.py:61-213, and
 *   get_search_info, .../Oneline_DLTv1/tools/get_img_info.py:42-70.  Crop / padding / normalisation arithmetic is pinned to
 *   fixtures from the reference; the resize is a restatement of OpenCV's and parity-unpinned.
 * hdn_frame_warp_perspective_u8: dst = cv2.warpPerspective(src, M, (W,H), INTER_LINEAR, BORDER_REPLICATE), M[9];
 *   replaces hdn/tracker/hdn_tracker_proj_e2e.py:154.  Restated OpenCV, parity-unpinned.
 * hdn_frame_warp_affine_cubic_u8: dst = cv2.warpAffine(src, M, (W,H), INTER_CUBIC, BORDER_REPLICATE), M[6];
 *   replaces img_rot_around_center, hdn/utils/transform.py:69-100.  Restated OpenCV, parity-unpinned.  (Its first call on
 *   a device uploads a 32 KB coefficient table synchronously.)
 * hdn_remap_linear_f32: dst[c] = cv2.remap(src[c] as uint8, mapx, mapy, INTER_LINEAR, BORDER_CONSTANT 0) on C planes of
 *   uint8-valued float32 (what hdn_subwindow_f32 mode 0 returns), float32 maps [Hd, Wd] on the device.  With the maps of
 *   cv::warpPolar (hdn_amd.frame.log_polar_maps builds them on the host as OpenCV >= 3.4.2 / 4.x does) this is
 *   cv2.logPolar(img, center, M, WARP_FILL_OUTLIERS + INTER_LINEAR): replaces getPolarImg, hdn/models/logpolar.py:11-29, called on
 *   every template crop by get_subwindow(islog=1), hdn/tracker/base_tracker.py:119-126.  Restated OpenCV, parity-unpinned.
 */
int hdn_subwindow_f32(const unsigned char* frame, const double* params, float* out, int H, int W, int C, int model_sz, int mode,
                      void* stream);
int hdn_frame_warp_perspective_u8(const unsigned char* src, const double* M, unsigned char* dst, int H, int W, int C, void* stream);
int hdn_frame_warp_affine_cubic_u8(const unsigned char* src, const double* M, unsigned char* dst, int H, int W, int C, void* stream);
/*
 * The three calls above for B frames at once (B independent sequences advancing in lock step; the reference's only inference-time
 * parallelism is several videos at once, tools/test.py:91-103): frames / crops contiguous [B, ...]; frame b takes its parameter record /
 * matrix at params + b * params_stride (>= 3 + C doubles) / M + b * m_stride (>= 9 / 6 doubles), so the records may be columns of a wider
 * per-sequence array (the similarity state record).  Per frame bit-identical to the single-frame call (same kernel, blockIdx.y = b).
 */
int hdn_subwindow_batch_f32(const unsigned char* frames, const double* params, int params_stride, float* out, int B, int H, int W, int C,
                            int model_sz, int mode, void* stream);
int hdn_frame_warp_perspective_batch_u8(const unsigned char* src, const double* M, int m_stride, unsigned char* dst, int B, int H, int W, int C,
                                        void* stream);
int hdn_frame_warp_affine_cubic_batch_u8(const unsigned char* src, const double* M, int m_stride, unsigned char* dst, int B, int H, int W, int C,
                                         void* stream);
/*
 * The three calls for B frames of DIFFERENT sizes (the videos of a dataset streamed through the slots of the lock-step tracker; the
 * reference's tools/test.py:91-103 splits such a list by hand across processes, one video at a time in each).  frames / src / dst: an arena
 * of B slots `slot_stride` bytes apart (>= Hmax * Wmax * C), slot b holding a dense [H_b, W_b, C] frame at its start; dims: DEVICE int32
 * [B][2] = (H_b, W_b).  The sizes are data, not launch arguments, so a captured hipGraph keeps replaying while slots change their frame
 * size.  The grid is sized from the capacity (Hmax, Wmax); every workgroup reads its slot's record and runs the single-frame loop over its
 * own H_b * W_b, with the perspective warp's block width (OpenCV's summation order of x) and the bounds of the 4-byte loads taken from
 * the slot's own size.  params / M / out (crops, contiguous [B, ...]) as in the batch calls.  Per slot bit-identical to the single-frame
 * call on that slot's frame.  The host cannot see dims: a slot whose record has H < 1, W < 1, H > Hmax, W > Wmax or H * W * C >
 * slot_stride is skipped (nothing of it read, nothing written for it), and the bytes of a slot beyond H_b * W_b * C are never written.
 * HDN_E_SHAPE also for slot_stride < Hmax * Wmax * C; HDN_E_ALIAS when the two arenas (the arena and the crops) overlap anywhere.
 */
int hdn_subwindow_ragged_f32(const unsigned char* frames, long long slot_stride, const int* dims, const double* params, int params_stride,
                             float* out, int B, int Hmax, int Wmax, int C, int model_sz, int mode, void* stream);
int hdn_frame_warp_perspective_ragged_u8(const unsigned char* src, long long slot_stride, const int* dims, const double* M, int m_stride,
                                         unsigned char* dst, int B, int Hmax, int Wmax, int C, void* stream);
int hdn_frame_warp_affine_cubic_ragged_u8(const unsigned char* src, long long slot_stride, const int* dims, const double* M, int m_stride,
                                          unsigned char* dst, int B, int Hmax, int Wmax, int C, void* stream);
int hdn_remap_linear_f32(const float* src, const float* mapx, const float* mapy, float* dst, int C, int Hs, int Ws, int Hd, int Wd,
                         void* stream);

/*
 * Decode of the similarity branch's head maps (BASELINE configs[3]: the tracker loop), one wave per
 * pair, nothing leaves the device.  Replaces the numpy half of hdnTrackerHomo.track_new between the two network calls and the
 * homography crop, hdn/tracker/hdn_tracker_proj_e2e.py:169-186 and :197-214, i.e. hdnTracker._convert_score
 * (hdn/tracker/hdn_tracker.py:84-91), SiameseTracker._convert_c (hdn/tracker/base_tracker.py:54-59), the Hanning-window blend /
 * argmax / 0.05 gate, hdnTracker._convert_logpolar_simi (hdn_tracker.py:51-67), the 0.25 gate and
 * rot_scale_around_center_shift_tran (hdn/utils/transform.py:250-298) — with their four .cpu().numpy() reads per frame.
 *
 * seq[B][HDN_SIM_SEQ_DOUBLES] (float64, constants of a sequence, written by the host at init):
 *   [0] init_pos.x  [1] init_pos.y  [2] init_s_z  [3] s_x = floor(init_s_z * round(INSTANCE / EXEMPLAR))  [4] init_s_z_sm
 *   [5..7] channel_average (B, G, R)
 * state[B][HDN_SIM_STATE_DOUBLES] (float64, written by the two calls, read by hdn_subwindow_f32 / hdn_frame_warp_affine_cubic_u8
 * and the caller's 3x3 bookkeeping):
 *   translation call: [0] delta_cx [1] delta_cy [2] cx [3] cy [4] stop_update_flag [5] best_score = score[best_idx]
 *                     [6] best_idx [7] pscore[best_idx]  [8..13] hdn_subwindow_f32 params of the moved search crop (cx, cy, s_x, avg)
 *   log-polar call:   [16] scale_delta [17] rot_delta [18] best_idx_lp [19] score_lp[best_idx_lp]  [20..28] H_sim (row major)
 *                     [32..37] 2x3 matrix of img_rot_around_center(img, cx, cy, w, h, -rot_delta) (transform.py:69-100)
 *                     [40..45] hdn_subwindow_f32 params of the homography crop (cx, cy, init_s_z_sm * scale_delta, avg)
 *                     [46] sim_lp[0] as hdnTracker.track_new reads it (the float32 scale, 1 when gated) [47] 1 when the 0.25 / stop gate replaced sim_lp
 * cls[B,cls_channels,S,S], loc_c[B,2,S,S], cls_lp[B,cls_channels,S,S], loc_lp[B,4,S,S]: the heads' outputs (ModelBuilder.track_new / track_new_lp,
 * hdn/models/model_builder_e2e_unconstrained_v2.py:131-158).  window[S*S] float64 and points[S*S,2] float32: the tables the
 * reference's constructor builds (hdn_tracker_proj_e2e.py:26-32).  mag = log(EXEMPLAR / 2) / EXEMPLAR and
 * rot_unit = (float)(2 pi / EXEMPLAR) are passed in as the host computed them.  The log-polar call reads the state record the
 * translation call wrote.  np.argmax semantics throughout: the first maximum; a NaN (blended) score is the maximum, the first NaN wins,
 * an all-NaN map answers cell 0.  best_idx / best_idx_lp lie in [0, S*S) for any input.  The gates are `score < 0.05` / `< 0.25`, false for a
 * NaN: a NaN winner is decoded from its cell's regression values and reported with NaN scores, as the reference's numpy does.
 * cls_channels = cfg.BAN.KWARGS.cls_out_channels: 2 -> score = softmax over the two planes, class 1 (every shipped configuration);
 * 1 -> score = sigmoid of the single plane (hdn_tracker.py:85-87); anything else HDN_E_SHAPE.
 */
#define HDN_SIM_SEQ_DOUBLES 8
#define HDN_SIM_STATE_DOUBLES 48
int hdn_similarity_translation_f32(const float* cls, const float* loc_c, const double* window, const float* points, const double* seq,
                                   double* state, int B, int S, double window_influence, float stride_c, double exemplar_size,
                                   int cls_channels, void* stream);
int hdn_similarity_logpolar_f32(const float* cls_lp, const float* loc_lp, const float* points_lp, const double* seq, double* state, int B,
                                int S, float stride_lp, double mag, float rot_unit, int cls_channels, void* stream);

/*
 * hdn_simi_track_update_f64: the numpy lines of hdnTracker.track_new behind the two decodes (hdn/tracker/hdn_tracker.py:213-301) and the first
 * lines of the NEXT frame's (:176-192) — TRACKS['hdnTracker'] (hdn/tracker/tracker_builder.py:13), the similarity-only tracker whose search
 * window follows the target and whose template is refreshed every frame (update_template, :156-162).  One lane per sequence; nothing leaves
 * the device, so hdn_amd.simi_tracker replays a frame as one hipGraph.  Reads the state record of the two decode calls above (which were
 * given THIS frame's seq record), updates the track record, writes the next frame's seq record and the result.
 *   tr[B][HDN_SIMI_TRACK_DOUBLES] float64: [0..1] center_pos [2..3] size [4] rot [5] lp_shift[1] [6] scale [7] v [8] window_scale_factor
 *     [9] lost_count [10] last_lost [11] rot is np.float32 [12] lp_shift[1] is np.float32 (NumPy 2 turns both into float32 at the first un-gated
 *     frame: python number += np.float32) [13] frames tracked [14..15] init_size [16] init_s_z [17..18] init_pos [19] poly_shift_l
 *     [20..22] channel average [24..29] hdn_subwindow_f32 params of the next frame's first search crop (center_pos, s_x, avg)
 *     [32..37] 2x3 matrix of img_rot_around_center(init_img, init_pos, lp_shift[1]) (hdn/utils/transform.py:69-100) for update_template
 *     [40..45] hdn_subwindow_f32 params of the template crop (init_pos, init_s_z, avg; written by the host at init)
 *   seq[B][HDN_SIM_SEQ_DOUBLES]: rewritten for the next frame (center_pos, s_z, s_x, -, avg)
 *   out[B][HDN_SIMI_OUT_DOUBLES] float64: [0..3] bbox [4..7] bbox_aligned [8] best_score [9] rot [10..17] polygon (4 x (x, y), rolled by
 *     4 - poly_shift_l) [18] stop_update_flag [19] pscore[best_idx]
 * img_w / img_h: the frame's size (the clamps of :249-250); scale_score_thresh = cfg.TRACK.SCALE_SCORE_THRESH; context_amount =
 * cfg.TRACK.CONTEXT_AMOUNT; instance_exemplar_ratio = np.round(INSTANCE_SIZE / EXEMPLAR_SIZE).
 */
#define HDN_SIMI_TRACK_DOUBLES 48
#define HDN_SIMI_OUT_DOUBLES 20
int hdn_simi_track_update_f64(const double* state, double* tr, double* seq, double* out, int B, int img_w, int img_h, double scale_score_thresh,
                              double context_amount, double instance_exemplar_ratio, void* stream);
/*
 * hdn_simi_track_update_ragged_f64: the same lines for the B slots of an arena of frames of DIFFERENT sizes (the hdn_*_ragged_* frame calls above;
 * hdn_amd.simi_tracker.BatchedSimiTracker with frame_capacity).  dims: DEVICE int32 [B][2] = (H_b, W_b), the table those calls read - mind
 * the order: lane b clamps at img_h = H_b, img_w = W_b.  The frame size is data, not a launch argument, so a captured hipGraph goes on
 * replaying while a slot is handed a video of another size.  Everything else is hdn_simi_track_update_f64 (one device function is the body
 * of both kernels): per slot bit-identical to that call on the slot's rows with (img_w, img_h) = (W_b, H_b).  The host cannot see dims: a
 * slot whose record has H < 1, W < 1, H > Hmax or W > Wmax is skipped, nothing of its tr / seq / out row read or written.
 * HDN_E_NULL for any null pointer (dims too); HDN_E_SHAPE for B <= 0, Hmax <= 0, Wmax <= 0 or a ratio that is not > 0.
 */
int hdn_simi_track_update_ragged_f64(const double* state, double* tr, double* seq, double* out, const int* dims, int B, int Hmax, int Wmax,
                                     double scale_score_thresh, double context_amount, double instance_exemplar_ratio, void* stream);

/*
 * The tracker's 3x3 float64 bookkeeping, one lane per sequence (BASELINE configs[3]): the numpy lines of
 * hdnTrackerHomo.track_new either side of the networks, hdn/tracker/hdn_tracker_proj_e2e.py.
 *
 * hdn_track_prepare_f64 (:150-155): Ht = H_total, or the identity when det(H_total) == 0; Hinv = inv(Ht) = adj(Ht) / det(Ht)
 * (closed form; the reference calls np.linalg.inv) — the matrix handed to cv2.warpPerspective, i.e. to
 * hdn_frame_warp_perspective_u8.  H_total, Ht, Hinv: [B][9] row major; Ht may alias H_total.
 *
 * hdn_track_accumulate_f64 (:251-272): H_homo = inv(shift_H) @ (inv(scale_H_1) @ H_comp @ scale_H_1) @ shift_H;
 * H = Ht @ H_sim if homo_score > gate else Ht @ H_sim @ H_homo; H *= 1 / H[8]; out = cv2.perspectiveTransform(init_points, H)
 * (restated from OpenCV's published algorithm: double arithmetic on float32 points, multiplication by 1 / w, zeros when
 * |w| <= DBL_EPSILON) followed by best_score.
 *   consts[B][HDN_TRACK_CONST_DOUBLES]: [0..8] inv(scale_H_1) [9..17] scale_H_1 [18..26] inv(shift_H) [27..35] shift_H
 *                                       [36] the gate (2.5 in the reference), rest unused
 *   sim_state: the similarity record (HDN_SIM_STATE_DOUBLES per sequence; H_sim at [20..28], best_score at [5]) or NULL
 *              (H_sim = identity, best_score = 0)
 *   H_comp [B][9] float64 (hdn_refine_warp_f32's product), homo_score [B] float32, init_points [B][n_points][2] float64 (rounded to
 *   float32 as the reference's .astype(np.float32) does), H_out [B][9] (may alias H_total, not Ht), out [B][2 * n_points + 1] float32.
 */
#define HDN_TRACK_CONST_DOUBLES 40
int hdn_track_prepare_f64(const double* H_total, double* Ht, double* Hinv, int B, void* stream);
int hdn_track_accumulate_f64(const double* Ht, const double* sim_state, const double* H_comp, const float* homo_score, const double* consts,
                             const double* init_points, int n_points, double* H_out, float* out, int B, void* stream);

/*
 * First stage of the homography regressor's trunk, fused:
 *   out = maxpool3x3/s2/p1( relu( conv7x7/s2/p3(x, w) + b ) ),  x [B,2,H,W] (NCHW) -> out [B,64,Hp,Wp],
 *   Hc = (H-1)/2 + 1, Hp = (Hc-1)/2 + 1 (127 -> 64 -> 32); 2 <= W <= 128 (else HDN_E_LIMIT).
 * wT: the conv weights with eval-mode BatchNorm folded in, transposed to [ci=2][ky=7][kx=7][co=64]; bias[64] = the folded
 * shift.  nhwc != 0: out is written channels-last ([B,Hp,Wp,64] in memory), else NCHW.  fp32; summation order per output =
 * (input channel, input row, kx).  Replaces conv1 / bn1 / relu / maxpool of ResNet.forward,
 * homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:141-147,183-186 (eval mode only).
 */
int hdn_trunk_stem_f32(const float* x, const float* wT, const float* bias, float* out, int B, int H, int W, int nhwc, void* stream);

/*
 * The same stage on the matrix cores, for the batches that fill the chip (one workgroup per quarter image: B >= 32 at 127 px is where it pays;
 * hdn_amd.trunk.FusedStem dispatches): x [B,2,127,127] (NCHW) -> out [B,32,32,64] (channels-last in memory).  H, W: 127 only (else
 * HDN_E_LIMIT).  fp32 carried as two fp16 pieces, three piece products, fp32 accumulation: the error of an fp32 convolution.
 * wfrag: the stream hdn_pack_stem_mfma_f32 wrote (opaque since ABI 10).  Current order, informative: the folded conv weights in MFMA-fragment order, [7 k steps][2 n tiles][2 pieces][64 lanes = (k half g, n)][8] fp16: element j is
 * piece pc (p0 = fp16(w), p1 = fp16((w - p0) * 2048)) of w[co = 32 tile + n][ci][ky][kx = j], ci * 7 + ky = 2 * k step + g, and 0 at j = 7
 * (hdn_amd.trunk.pack_stem_mfma); 16-byte aligned, 28,672 bytes.  bias[64] as above.  Same reference lines as hdn_trunk_stem_f32.
 */
int hdn_trunk_stem_mfma_f32(const float* x, const void* wfrag, const float* bias, float* out, int B, int H, int W, int out_domain, void* stream);

/*
 * Residual-block epilogues of the same trunk, in place:
 *   y = relu(y + bias[c])                (residual == NULL)     after conv1 of a BasicBlock, bn1 folded into the conv
 *   y = relu((y + bias[c]) + residual)                          after conv2: `out += residual; out = relu(out)`
 * y / residual: [B,C,H,W] fp32 with HW = H*W, either NCHW-contiguous (nhwc == 0) or channels-last in memory (nhwc != 0);
 * bias[C] = the folded BatchNorm shift (plus the downsample branch's, when that branch is a folded conv).  One pass, 16 bytes
 * per lane when the layout allows (NHWC: C % 4 == 0; NCHW: HW % 4 == 0; 16-byte aligned pointers), one float per lane otherwise.
 * Replaces the bias-add / residual-add / ReLU launches around the convolutions of BasicBlock.forward,
 * homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:78-94 (eval mode only).
 */
int hdn_bias_relu_f32(float* y, const float* bias, const float* residual, int B, int C, int HW, int nhwc, void* stream);

/*
 * The regressor's tail as one launch: out[b, o] = bias[o] + sum_c W[o, c] * mean_p x[b, c, p], i.e. AdaptiveAvgPool2d(1) ->
 * flatten -> Linear(C, O) of homo_estimator/Deep_homography/Oneline_DLTv1/models/homo_model_builder.py:161-165 (x = fc(avgpool(
 * backbone(...)))) and hdn/models/model_builder_e2e_unconstrained_v2.py:190-194.  x [B,C,HW] (nhwc = 0) or [B,HW,C] (nhwc = 1)
 * fp32, W [O,C] row-major, bias [O] or NULL, O <= 16.  The mean is the fp32 sum in position order times 1 / HW (ATen's reduction
 * may associate differently: last-bit differences).
 */
int hdn_avgpool_fc_f32(const float* x, const float* w, const float* bias, float* out, int B, int C, int HW, int O, int nhwc, int in_domain, void* stream);

/*
 * Everything of a MultiBAN / MultiCircBAN forward behind the correlations, at the tracker's B = 1, as one launch:
 *   hid[g] = relu(W1[g] . feats[g] + b1[g])             g = branch * n_levels + level; the first 1x1 convolution + BatchNorm (folded by the host) +
 *                                                       ReLU of DepthwiseXCorr.head, hdn/models/head/ban.py:60-66
 *   out[br] = bf[br] + sum_l Wf[br][:, l H : (l + 1) H] . hid[br * n_levels + l]
 *                                                       the second 1x1 convolution, loc_scale and the (softmax-)weighted sum over the levels,
 *                                                       MultiBAN.forward ban.py:113-127 / MultiCircBAN.forward ban_lp.py:77-92 (linear: folded into Wf, bf)
 * feats [2 n_levels, hidden, pixels] (the stacked correlation outputs, cls groups first), b1 [2 n_levels, hidden], wf [2, n_out, n_levels * hidden],
 * bf [2, n_out], out [2, n_out, pixels], all fp32 contiguous; hidden = 128 or 256, n_out <= 8, n_levels <= 4 (and the staged operands must fit the LDS: HDN_E_LIMIT otherwise).  w1_packed: W1 [2 n_levels, hidden, hidden]
 * as two fp16 pieces (v = p0 + 2^-11 p1, as for hdn_conv3x3_bias_relu_f32) in MFMA fragment order
 * [group][hidden / 32 row tiles][hidden / 16 k steps][2 pieces][64 lanes][8] with lane = 32 * (k half) + row — written by hdn_pack_head_tail_f32 (opaque since ABI 10; the order is informative); 16-byte aligned.
 * The first product runs on the matrix cores with the error of an fp32 product, the second in fp32 FMAs; the sum over the levels is a fixed-order
 * register accumulation (deterministic).
 */
int hdn_head_tail_f32(const float* feats, const void* w1_packed, const float* b1, const float* wf, const float* bf, float* out, int n_levels, int hidden,
                      int pixels, int n_out, void* stream);

/*
 * The same tail at any batch B, as one launch (added within ABI 10): everything of MultiBAN.forward / MultiCircBAN.forward behind the correlations for
 * the heads of the lock-step trackers - the six `head` Sequentials (hdn/models/head/ban.py:60-66), loc_scale, the softmax of the level weights and the
 * two weighted sums (ban.py:113-127, ban_lp.py:77-92).
 * feats [2 n_levels][B][hidden][pixels] fp32, dense: group g = branch * n_levels + level, cls groups first, each group a contiguous [B, hidden, Ho, Wo] -
 * exactly what hdn_xcorr_depthwise_multi_f32 writes through `outs`.  w1_packed, b1, wf, bf: exactly what hdn_head_tail_f32 takes with
 * n_out = om = max(n_out_cls, n_out_loc): wf [2, om, n_levels * hidden], bf [2, om], the stream of hdn_pack_head_tail_f32.
 * out: ONE buffer of B (n_out_cls + n_out_loc) pixels floats, the cls block [B][n_out_cls][pixels] first, the loc block [B][n_out_loc][pixels] behind it:
 * row o of branch br, image b is at (br B n_out_cls + b n_out[br] + o) pixels, n_out[0] = n_out_cls, n_out[1] = n_out_loc; rows o >= n_out[br] are not
 * written.  Both results are contiguous [B, n_out_cls, Ho, Wo] / [B, n_out_loc, Ho, Wo] views, as the reference's heads return them; with B = 1 and
 * n_out_cls == n_out_loc it is hdn_head_tail_f32's [2, n_out, pixels].  A workgroup owns 32 pixels of ONE image and one branch (grid z = image; images do
 * not share a pixel tile), and every output element is summed in the order of hdn_head_tail_f32: image b of a batch is bit-equal to that entry on the
 * image alone (batch invariance).
 * All arguments are checked before the first HIP call: HDN_E_NULL a null pointer; HDN_E_SHAPE n_levels, B, hidden, pixels, n_out_cls or n_out_loc <= 0;
 * HDN_E_LIMIT n_levels > 4, an out count > 8, hidden not 128 or 256, B > 65535, 2 n_levels B hidden pixels > 2^31 - 1, staged operands beyond the 160 KB of
 * LDS (hdn_head_tail_lds_bytes), w1_packed not 16-byte aligned; HDN_E_ALIAS out's byte range overlapping feats'.  Takes part in the range guard
 * (hdn_set_check_range) over all images.  Asynchronous on `stream`; allocates nothing; deterministic; capturable.
 */
int hdn_head_tail_batch_f32(const float* feats, const void* w1_packed, const float* b1, const float* wf, const float* bf, float* out,
                            int n_levels, int B, int hidden, int pixels, int n_out_cls, int n_out_loc, void* stream);
/* Bytes of LDS a workgroup of hdn_head_tail_f32 / hdn_head_tail_batch_f32 stages for (n_levels, hidden, n_out = max of the two out counts); both entries
 * return HDN_E_LIMIT above 160 KB (163,840).  Negative = HDN_E_* (the limits above).  Host only. */
long long hdn_head_tail_lds_bytes(int n_levels, int hidden, int n_out);

/*
 * conv_search of the correlation heads at B = 1: n (<= 4) same-shaped problems in one launch, each
 *   out[i] [CO, Hi - 2, Wi - 2] = relu(conv3x3 / stride 1 / no padding (x[i] [256, Hi, Wi], W[i]) + bias[i])
 * = DepthwiseXCorr.conv_search (Conv2d 3x3 no bias + BatchNorm, folded by the host, + ReLU; hdn/models/head/ban.py:55-59,75) for the levels of a
 * MultiBAN / MultiCircBAN, the cls and loc branches of a level concatenated along CO (they share their input).  x[i]: fp32, 256 channels, NCHW
 * (nhwc = 0) or channels-last (nhwc = 1) strides; out[i]: contiguous NCHW planes (what hdn_xcorr_depthwise_multi_f32 reads); bias [n, CO]; CO a
 * multiple of 32.  w_packed: the folded weights as two fp16 pieces (v = p0 + 2^-11 p1, as for hdn_conv3x3_bias_relu_f32) in MFMA fragment order
 * [problem][CO / 32][4 chunks of 64 input channels][4 k slices of 16][9 taps][2 pieces][64 lanes][8], lane = 32 * (k half) + output channel,
 * written by hdn_pack_head_conv3x3_f32 (opaque since ABI 10; the order is informative); 16-byte aligned.  The patch of 64 consecutive output pixels (their rows + 2, full width) must fit 224 pixels
 * (HDN_E_LIMIT otherwise: widths up to ~60).  Error class of an fp32 convolution; deterministic.
 */
int hdn_head_conv3x3_f32(const float* const* xs, const void* w_packed, const float* bias, float* const* outs, int n, int CO, int Hi, int Wi, int nhwc,
                         void* stream);

/*
 * The same convolution at any batch B, into one buffer (added within ABI 10): the template branch of the heads,
 *   kernel = self.conv_kernel(kernel)   (hdn/models/head/ban.py:55-59,74; DepthwiseXCorrCirc in ban_lp.py likewise),
 * for all levels and both branches of a MultiBAN / MultiCircBAN in one launch, and conv_search (ban.py:55-59,75) of the lock-step trackers at B > 1.
 * xs[i]: level i's input [B, 256, Hi, Wi] fp32, every image dense NCHW (nhwc = 0) or dense channels-last (nhwc = 1), the images x_batch_stride
 * (>= 256 Hi Wi) elements apart - a batch slice of a larger tensor needs no copy.  w_packed / bias [n, CO]: exactly what hdn_head_conv3x3_f32 takes
 * (hdn_pack_head_conv3x3_f32).  out: one contiguous buffer [n][groups][B][CO / groups][Ho Wo], groups 1 or 2, CO / groups a multiple of 32: output
 * channel co of level i, image b is at (((i groups + co / (CO / groups)) B + b) (CO / groups) + co % (CO / groups)) Ho Wo.  With groups = 2 and the cls
 * and loc weights of a level concatenated along CO, each branch of each level is a contiguous [B, hidden, Ho, Wo] - what hdn_xcorr_depthwise_multi_f32
 * reads; with B = 1 it is the layout of hdn_head_conv3x3_f32 with adjacent outs.  Every output element is summed in the order of hdn_head_conv3x3_f32:
 * image b of a batch is bit-equal to that entry on the image alone (batch invariance).
 * All arguments are checked before the first HIP call: HDN_E_NULL a null pointer; HDN_E_SHAPE n, B or CO <= 0, Hi or Wi < 3, groups not 1 or 2;
 * HDN_E_LIMIT n > 4, CO / groups no multiple of 32, the 224-pixel patch limit above, n B > 65535, w_packed not 16-byte aligned, x_batch_stride
 * < 256 Hi Wi; HDN_E_ALIAS out overlapping an input.  Takes part in the range guard (hdn_set_check_range) on every image.  Asynchronous on `stream`;
 * allocates nothing; deterministic; capturable.
 */
int hdn_head_conv3x3_batch_f32(const float* const* xs, const void* w_packed, const float* bias, float* out, int n, int B, int groups, int CO, int Hi,
                               int Wi, int nhwc, long long x_batch_stride, void* stream);

/*
 * Whole residual-block convolutions of that trunk on the matrix cores, channels-last fp32 in and out:
 *   hdn_conv3x3_bias_relu_f32:  out = relu(conv3x3/s1/p1(x, W) + bias[c] (+ residual)),  x / residual / out [B,S,S,C], C -> C channels,
 *       (S, C) = (32, 64), (16, 128), (8, 256), (4, 512): conv1 / conv2 + bn + relu (+ `out += residual`) of BasicBlock.forward;
 *   hdn_conv3x3s2_ds_f32:       out = relu(conv3x3/s2/p1(x, W1) + bias[c]) and out_ds = conv1x1/s2(x, Wd) from the SAME staged input,
 *       x [B,2S,2S,CI] -> out / out_ds [B,S,S,2 CI], (S, CI) = (16, 64), (8, 128), (4, 256): conv1 + bn1 + relu and the `downsample`
 *       branch of the first block of layer2..4 (out_ds carries no bias: the caller adds the folded downsample shift to the bias of
 *       the block's second convolution, whose residual out_ds is).
 * Any other shape returns HDN_E_LIMIT (the caller keeps MIOpen for it).  fp32 accuracy from the 16-bit matrix pipe (ABI 5): activations
 * and weights are split into two fp16 pieces each, v = p0 + 2^-11 p1 with p0 = fp16(v), p1 = fp16((v - p0) * 2^11) (22 significand
 * bits), and three piece products are accumulated in fp32 (x0 w0 in one accumulator set, x0 w1 + x1 w0 in a second one that is
 * added with the factor 2^-11; conv3x3.hip); against float64 the result has the error of an fp32 convolution.  Range (ABI 9): weights
 * |w| < 65,504 (fp16; the packer checks them), activations |x| < 65,520 x 256 = 1.67e7 — the kernels split an activation as x 2^-8 and
 * scale the sums back by 2^8 (exact), csrc/mfma_split.h; the trunk's activations are O(10).
 * wpacked: the stream hdn_pack_conv3x3_f32 / hdn_pack_conv3x3s2_ds_f32 wrote from the BatchNorm-folded weights (opaque since ABI 10).  Its
 *   current order, for readers of conv3x3.hip only:
 *   [CO / BN][CI / (16 KS)][3 kernel rows][T taps][KS k steps][2 pieces][2 k halves][BN][8] fp16, input channel = chunk * 16 KS +
 *   step * 16 + half * 8 + j, (BN, KS) = hdn_conv3x3_pack_info(S, CI, stride); T = 3, or 4 for the stride-2 form, whose 4th tap holds
 *   the 1x1 weights in the middle kernel row (zeros in the other two); 16-byte aligned.
 * Workspace: when the output tiles alone do not fill the chip (S = 4 at any batch size, every shape at small B) the K dimension is
 * split over workgroups, the slices' partial sums go to `workspace` and a second launch adds them in slice order (deterministic)
 * with the bias / residual / ReLU.  hdn_conv3x3_workspace_bytes(B, S, CI, stride): bytes needed, 0 = none (workspace may be NULL),
 * negative = HDN_E_*.
 * Replaces homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:78-94 and the downsample branch built at :162-169
 * (eval mode only).
 */
/*
 * Activation domain (ABI 10).  `act_domain` of the trunk's convolution entry points: 0 = activations (x, residual, out, out_ds, slices) are in real units, the
 * kernels split them as x 2^-8 and scale the sums back (one packed multiply per staged pair: +3.8 % on the full head); 1 = they are ALREADY x_real 2^-8 in
 * memory, in and out — no multiply anywhere, `bias` must be handed over as bias 2^-8 (exact).  hdn_amd.trunk runs the whole fused trunk in domain 1: it is
 * entered at hdn_trunk_stem_mfma_f32 (`out_domain` = 1: real input, scaled output) and left at hdn_avgpool_fc_f32 (`in_domain` = 1: multiplies the pooled
 * means by 2^8), so the multiply is paid once per trunk and the range of ABI 9 (|x_real| < 1.67e7) holds at the speed of ABI 8.  ReLU, max-pool, residual
 * addition and hdn_bias_relu_f32 / hdn_conv3x3_finish_f32 are the same in either domain (they are positively homogeneous / linear with the scaled bias).
 *
 * Range guard of the two-fp16-piece kernels (ABI 6): hdn_conv3x3_bias_relu_f32, hdn_conv3x3s2_ds_f32, hdn_conv3x3_v2_f32,
 * hdn_conv3x3_chain_f32 (activation inputs), hdn_trunk_stem_mfma_f32, hdn_head_conv3x3_f32, hdn_head_conv3x3_batch_f32, hdn_head_tail_f32, hdn_head_tail_batch_f32, hdn_conv1x1_f32, hdn_conv3x3s2_f32 and hdn_conv3x3d_f32 are finite and fp32-accurate
 * for |x| < 1.67e7 on their fp32 INPUTS by default (since ABI 9; 65,504 before).  Beyond that the first fp16 piece is inf and the result NaN,
 * where the reference's fp32 convolution stays finite up to 3.4e38.  With HDN_CHECK_RANGE=1 in the environment, or after hdn_set_check_range(1)
 * (returns the previous setting), each of those entry points first reduces max |x| over its input and returns HDN_E_LIMIT when it is
 * >= 16,773,120 or NaN, launching nothing.  The check
 * costs a reduction launch and a stream synchronisation per call: a debug switch, off by default, skipped inside stream captures.
 */
int hdn_set_check_range(int on);

/*
 * Measurement hook (ABI 10): the NEXT 31x31 (x) 61x61 launch the calling thread makes through hdn_xcorr_depthwise_f32 / _multi_f32 carries these two
 * hipEvent_t (either may be NULL) as hipExtLaunchKernelGGL's start / stop events: they take the dispatch's own timestamps, so hipEventElapsedTime(start,
 * stop) is the kernel's duration on its stream with no marker packets around it (a hipEventRecord pair costs the stream ~4 us on each side of the kernel).
 * One-shot: cleared by the launch, and by the end of the calling thread's next hdn_xcorr_depthwise* call whatever that call launched (another shape, the direct
 * variant, an argument error): the events never outlive the call they were armed for.  bench.py brackets the roofline kernel of every timed step this way.
 */
int hdn_xcorr_north_launch_events(void* start_event, void* stop_event);

/*
 * Weight packers (ABI 10; csrc/pack.hip; HOST pointers in and out, no device work).  The matrix-core entry points below and above take their
 * weights as an opaque stream: hand the packer the fp32 weights in the reference's own order ([CO][CI][kh][kw] row major, i.e. what a
 * state_dict holds, BatchNorm folded in by the caller), upload the bytes it wrote (16-byte aligned) and pass them as `wpacked` / `wfrag` /
 * `w_packed` / `w1_packed`.  The ORDER inside a stream is the kernel's business and may change between library builds (the layout notes further
 * down describe the current one for readers of the kernels, they are not part of the contract); pack and run with the same library.
 * Every stream holds two fp16 pieces per (padded) weight, v = p0 + 2^-11 p1; a weight with |w| >= 65,504 or NaN -> HDN_E_LIMIT.
 * (The one packer that runs on the device, hdn_pack_conv3x3d_dev_f32 further down, cannot raise inside a capture: it COUNTS such weights instead.)
 * hdn_pack_*_bytes: size of the stream (negative = HDN_E_SHAPE for a shape no kernel serves); the packers check `out_bytes` against it.
 *   hdn_pack_conv3x3_f32       w [C][C][3][3]                          -> hdn_conv3x3_bias_relu_f32 / hdn_conv3x3_chain_f32, C = 64 / 128 / 256 / 512
 *   hdn_pack_conv3x3s2_ds_f32  w [2CI][CI][3][3], w_ds [2CI][CI]       -> hdn_conv3x3s2_ds_f32 (backbone/resnet.py:78-94 conv1 and :162-169 downsample)
 *   hdn_pack_conv3x3_v2_f32    w [C][C][3][3]                          -> hdn_conv3x3_v2_f32
 *   hdn_pack_conv3x3s2_v2_f32  w [2CI][CI][3][3], w_ds [2CI][CI]       -> hdn_conv3x3s2_v2_f32
 *   hdn_pack_stem_mfma_f32     w [64][2][7][7]                         -> hdn_trunk_stem_mfma_f32 (backbone/resnet.py:141-147)
 *   hdn_pack_head_conv3x3_f32  ws[n] -> [CO][256][3][3]                -> hdn_head_conv3x3_f32 (hdn/models/head/ban.py:55-59)
 *   hdn_pack_head_tail_f32     w1 [G][H][H]                            -> hdn_head_tail_f32 (ban.py:60-66)
 *   hdn_pack_conv1x1_f32       w [CO][CI]                              -> hdn_conv1x1_f32 (backbone/resnet.py:97-133, 162-176), CO, CI multiples of 32
 *   hdn_pack_conv3x3s2_f32     w [C][C][3][3]                          -> hdn_conv3x3s2_f32 (backbone/resnet.py:97-133 conv2 at stride 2), C = 128 / 256 / 512
 *   hdn_pack_conv3x3d_f32      w [CO][CI][3][3]                        -> hdn_conv3x3d_f32 (hdn/models/backbone/resnet_atrous.py:62-110, 152-183), CO, CI multiples of 32;
 *                                                                         also hdn_conv3x3v_f32 (resnet_atrous.py:70-81, 162-174)
 *   hdn_pack_simi_stem_f32     w [64][3][7][7]                         -> hdn_simi_stem_f32 (resnet_atrous.py:117-121); declared beside it further down
 */
long long hdn_pack_conv3x3_bytes(int C);
int hdn_pack_conv3x3_f32(const float* w, int C, void* out, long long out_bytes);
long long hdn_pack_conv3x3s2_ds_bytes(int CI);
int hdn_pack_conv3x3s2_ds_f32(const float* w, const float* w_ds, int CI, void* out, long long out_bytes);
long long hdn_pack_conv3x3_v2_bytes(int C);
int hdn_pack_conv3x3_v2_f32(const float* w, int C, void* out, long long out_bytes);
long long hdn_pack_conv3x3s2_v2_bytes(int CI);
int hdn_pack_conv3x3s2_v2_f32(const float* w, const float* w_ds, int CI, void* out, long long out_bytes);
long long hdn_pack_stem_mfma_bytes(void);
int hdn_pack_stem_mfma_f32(const float* w, void* out, long long out_bytes);
long long hdn_pack_head_conv3x3_bytes(int n, int CO);
int hdn_pack_head_conv3x3_f32(const float* const* ws, int n, int CO, void* out, long long out_bytes);
long long hdn_pack_head_tail_bytes(int G, int H);
int hdn_pack_head_tail_f32(const float* w1, int G, int H, void* out, long long out_bytes);
long long hdn_pack_conv1x1_bytes(int CO, int CI);
int hdn_pack_conv1x1_f32(const float* w, int CO, int CI, void* out, long long out_bytes);
long long hdn_pack_conv3x3s2_bytes(int C);
int hdn_pack_conv3x3s2_f32(const float* w, int C, void* out, long long out_bytes);
long long hdn_pack_conv3x3d_bytes(int CO, int CI);                                              /* resnet_atrous.py:62-110, 152-183 */
int hdn_pack_conv3x3d_f32(const float* w, int CO, int CI, void* out, long long out_bytes);      /* resnet_atrous.py:62-110, 152-183 */

int hdn_conv3x3_pack_info(int S, int CI, int stride, int* block_n, int* k_steps);
long long hdn_conv3x3_workspace_bytes(int B, int S, int CI, int stride);
int hdn_conv3x3_bias_relu_f32(const float* x, const void* wpacked, const float* bias, const float* residual, float* out, float* workspace,
                              long long workspace_bytes, int B, int S, int C, int act_domain, void* stream);
int hdn_conv3x3s2_ds_f32(const float* x, const void* wpacked, const float* bias, float* out, float* out_ds, float* workspace,
                         long long workspace_bytes, int B, int S, int CI, int act_domain, void* stream);

/*
 * The stride-1 convolutions above in the form for batches that fill the chip (ABI 6; conv3x3.hip, conv3x3_v2_kernel): same arithmetic (two
 * fp16 pieces, three products, hi / lo accumulators), same shapes (S, C), same result up to the order of the fp32 partial sums; every
 * consumer wave owns a 64 x 64 output tile, the four consumers of a workgroup are WM pixel tiles x WK slices of K, and the weights
 * stream L2 -> registers in fragment order (they never touch the LDS).  hdn_amd.trunk uses it from B = 24 pairs on (below that the
 * chained form is faster).
 * wpacked: the stream hdn_pack_conv3x3_v2_f32 wrote (opaque since ABI 10); current order, informative:
 *   [C / (32 NT)][C / (16 KS)][WK k slices][9 taps x KS / WK k steps][NT n tiles][2 pieces][64 lanes = k half x 32 + n][8] fp16, input channel = chunk * 16 KS + (j * WK + slice) * 16 + half * 8 + e for the j-th k step of a
 *   slice, output channel = block * 32 NT + tile * 32 + n; (WK, KS, NT) = hdn_conv3x3_v2_pack_info(S, C); 16-byte aligned.
 * Workspace as above (K split over workgroups when the tiles do not fill the chip: S = 4 at B = 64): hdn_conv3x3_v2_workspace_bytes.
 * Replaces homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:78-94 (eval mode only).
 */
int hdn_conv3x3_v2_pack_info(int S, int C, int* k_slices, int* k_steps, int* n_tiles);
long long hdn_conv3x3_v2_workspace_bytes(int B, int S, int C);
int hdn_conv3x3_v2_f32(const float* x, const void* wpacked, const float* bias, const float* residual, float* out, float* workspace,
                       long long workspace_bytes, int B, int S, int C, int act_domain, void* stream);

/*
 * hdn_conv3x3s2_ds_f32's large-batch form (round 5, conv3x3s2.hip; hdn_amd.trunk dispatches from B = 24): the same two outputs,
 *   out = relu(conv3x3/s2/p1(x, w) + bias),  out_ds = conv1x1/s2(x, w_ds) (raw),  x [B,2S,2S,CI] -> out, out_ds [B,S,S,2 CI] (channels-last),
 * (S, CI) = (16, 64), (8, 128), (4, 256) (else HDN_E_LIMIT), no workspace.  Same arithmetic as above (two fp16 pieces, three products, hi / lo
 * fp32 accumulators; summation order: chunks of 32 input channels, inside a chunk the 9 taps, the two 16-channel k steps added last).
 * wpacked: the stream hdn_pack_conv3x3s2_v2_f32 wrote (opaque since ABI 10); current order, informative:
 * [2 CI / 64][CI / 32][2 k steps][10 steps][2 n tiles][2 pieces][k half g][n][8] fp16 - element e of lane (g, n) = piece of
 * w[co = 64 block + 32 tile + n][ci = 32 chunk + 16 k step + 8 g + e][tap t = 3 ky + kx] for step t < 9, of w_ds[co][ci] for step 9
 * ; 16-byte aligned.  Replaces conv1 + bn1 + relu and downsample(x) of a BasicBlock with stride 2,
 * backbone/resnet.py:78-94.
 */
int hdn_conv3x3s2_v2_f32(const float* x, const void* wpacked, const float* bias, float* out, float* out_ds, int B, int S, int CI, int act_domain, void* stream);

/*
 * 1x1 convolution of the ResNet-50 (Bottleneck) homography trunk with its epilogue fused (conv1x1.hip; added in ABI 10):
 *   out[B,So,So,CO] = [relu]( conv1x1/stride(x, w) + bias[co] [+ residual[B,So,So,CO]] ),   x [B,S,S,CI], So = (S - 1) / stride + 1, channels-last,
 * stride 1 or 2 (2: even rows and columns, the downsample branch of a stage's first block), relu 0 / 1, CI and CO multiples of 32, any B >= 1
 * (else HDN_E_SHAPE; more than 2^31 - 1 elements in x or out, or CO > 65,536: HDN_E_LIMIT).  `residual` may be NULL; `out` may overlap neither `x`
 * nor `residual` (HDN_E_ALIAS).  x, out, residual and wpacked 16-byte aligned (HDN_E_LIMIT).  act_domain as above ("Activation domain"): 1 = x,
 * residual and out are x_real 2^-8 in memory and `bias` is bias 2^-8.  fp32 carried as two fp16 pieces, three products, hi / lo fp32 accumulators: the
 * error of an fp32 convolution; deterministic.  Takes part in the range guard (hdn_set_check_range) on `x`.  No workspace.
 * wpacked: the stream hdn_pack_conv1x1_f32 wrote from w [CO][CI] (BatchNorm folded in by the caller).
 * Replaces conv1 + bn1 + relu, conv3 + bn3 + the residual addition + relu and the downsample branch of
 * homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:97-133 (Bottleneck), 162-176 (_make_layer's downsample), eval mode only.
 */
int hdn_conv1x1_f32(const float* x, const void* wpacked, const float* bias, const float* residual, float* out, int B, int S, int CI, int CO, int stride,
                    int relu, int act_domain, void* stream);
/* The launch form hdn_conv1x1_f32 picks for a problem (conv1x1.hip, Cfg<NT, WM, WN, KW>: 32-channel output tiles per wave, pixel tiles x
 * output-channel groups x K slices of the four waves of a workgroup), as NT | WM << 8 | WN << 16 | KW << 24, or HDN_E_SHAPE / HDN_E_LIMIT as the
 * entry point answers for these arguments.  Asked of the rule the launch itself goes through; host only, nothing is launched.  For tests (which
 * prove with it that they run every form) and profiles; the forms themselves are no part of the ABI. */
int hdn_conv1x1_form(int B, int S, int CI, int CO, int stride);

/*
 * Stride-2 3x3 convolution of a Bottleneck, bias and ReLU fused (conv3x3s2.hip; added in ABI 10): conv2 + bn2 + relu of the first block of layer2 / 3 / 4
 * of the ResNet-50 homography trunk,
 *   out[B,S,S,C] = relu( conv3x3 / stride 2 / padding 1 (x[B,2S,2S,C], w[C][C][3][3]) + bias[c] ),   channels-last fp32,
 * (S, C) = (16, 128), (8, 256), (4, 512), any B >= 1 (B <= 0 or act_domain outside {0, 1}: HDN_E_SHAPE; another (S, C), more than 2^31 - 1 elements in x,
 * a pointer that is not 16-byte aligned or a workspace that is too small: HDN_E_LIMIT).  `out` and `workspace` may not overlap `x` (HDN_E_ALIAS).
 * act_domain as above ("Activation domain").  fp32 carried as two fp16 pieces, three products, hi / lo fp32 accumulators: the error of an fp32
 * convolution.  Deterministic: inside a workgroup the sum runs over chunks of 32 input channels, the nine taps of a chunk, the two 16-channel k steps of a
 * tap; where the output tiles alone do not fill the chip (small B, and S = 8 / 4 at any B) K is split over workgroups - by chunks, then by kernel row -
 * the slices' partial sums go to `workspace` and a second launch adds them in slice order with the bias and the ReLU.  No atomics.
 * hdn_conv3x3s2_workspace_bytes(B, S, C): bytes needed, 0 = none (workspace may be NULL then), negative = HDN_E_*.
 * Takes part in the range guard (hdn_set_check_range) on `x`.  Asynchronous on `stream`; allocates nothing.
 * wpacked: the stream hdn_pack_conv3x3s2_f32 wrote from the BatchNorm-folded w (opaque).
 * Replaces conv2 + bn2 + relu of homo_estimator/Deep_homography/Oneline_DLTv1/backbone/resnet.py:97-133 where the block's stride is 2 (eval mode only).
 */
long long hdn_conv3x3s2_workspace_bytes(int B, int S, int C);
int hdn_conv3x3s2_f32(const float* x, const void* wpacked, const float* bias, float* out, float* workspace, long long workspace_bytes, int B, int S, int C,
                      int act_domain, void* stream);

/*
 * Dilated 3x3 convolution of the similarity branch's atrous ResNet-50, bias and ReLU fused (conv3x3d.hip; added in ABI 10):
 *   out[B,S,S,CO] = [relu]( conv3x3 / stride 1 / dilation d / zero padding d (x[B,S,S,CI], w[CO][CI][3][3]) [+ bias[co]] ),   channels-last fp32,
 * d = 1 / 2 / 4, CI and CO multiples of 32, any B >= 1 and S >= 1 (S <= d: only the centre tap is in bounds), relu and act_domain 0 / 1 (else
 * HDN_E_SHAPE); more than 2^31 - 1 elements in x or out, a pointer that is not 16-byte aligned or a workspace that is too small: HDN_E_LIMIT.  `bias` may
 * be NULL (zero: a downsample branch, whose shift rides in the block's last bias).  `out` may overlap neither `x` nor `ws`, `ws` not `x` (HDN_E_ALIAS).
 * act_domain as above ("Activation domain").  fp32 carried as two fp16 pieces, three products, hi / lo fp32 accumulators: the error of an fp32
 * convolution.  Deterministic: K runs tap-major (tap = 3 ky + kx, inside a tap chunks of 32 input channels, the two 16-channel k steps of a chunk); where
 * the output tiles do not fill the chip K is split over workgroups into slices of whole (tap, chunk) steps, the slices' partial sums go to `ws` and a second
 * launch adds them in slice order with the bias and the ReLU.  No atomics.
 * hdn_conv3x3d_workspace_bytes: bytes needed, 0 = none (ws may be NULL then), negative = HDN_E_*.
 * hdn_conv3x3d_form: the launch form for a problem, MT | NT << 4 | WM << 8 | WN << 12 | (K slices) << 16 (conv3x3d.hip, Cfg<MT, NT, WM, WN>: 32 x 32 tiles per
 * wave, waves per workgroup), or HDN_E_* as the entry point answers; host only, nothing is launched; for tests and profiles, no part of the ABI.
 * Takes part in the range guard (hdn_set_check_range) on `x`.  Asynchronous on `stream`; allocates nothing.
 * wpacked: the stream hdn_pack_conv3x3d_f32 wrote from the BatchNorm-folded w (opaque; the same stream serves every dilation).
 * Replaces conv2 + bn2 + relu of a Bottleneck and the 3x3 downsample branches of hdn/models/backbone/resnet_atrous.py:62-110, 152-183 (eval mode only).
 */
long long hdn_conv3x3d_workspace_bytes(int B, int S, int CI, int CO, int dilation);             /* resnet_atrous.py:62-110, 152-183 */
int hdn_conv3x3d_form(int B, int S, int CI, int CO, int dilation);                              /* resnet_atrous.py:62-110, 152-183 */
int hdn_conv3x3d_f32(const float* x, const void* wpacked, const float* bias, float* out, void* ws, long long ws_bytes, int B, int S, int CI, int CO,
                     int dilation, int relu, int act_domain, void* stream);                     /* resnet_atrous.py:62-110, 152-183 */

/*
 * The same convolution without padding ("valid"), stride 1 or 2 (conv3x3d.hip, the kernel above with another pixel map; an addition to ABI 10):
 *   out[B,So,So,CO] = [relu]( conv3x3 / stride s / padding 0 / dilation 1 (x[B,S,S,CI], w[CO][CI][3][3]) [+ bias[co]] ),   So = (S - 3) / s + 1,
 * channels-last fp32 in and out; output pixel (oy, ox) reads input pixels (s oy + ky, s ox + kx), so with an even S at stride 2 the last input row and
 * column are never read.  s = 1 / 2, S >= 3, CI and CO multiples of 32, any B >= 1, relu and act_domain 0 / 1 (else HDN_E_SHAPE); more than 2^31 - 1
 * elements in x or out, a pointer that is not 16-byte aligned or a workspace that is too small: HDN_E_LIMIT.  `bias` may be NULL (zero: the 3x3 skip of
 * layer2's first block, whose shift rides in the block's last bias).  `out` may overlap neither `x` nor `ws`, `ws` not `x` (HDN_E_ALIAS); NULL x,
 * wpacked, out, or ws where one is needed: HDN_E_NULL.  act_domain as above ("Activation domain").  fp32 carried as two fp16 pieces, three products,
 * hi / lo fp32 accumulators: the error of an fp32 convolution.  Deterministic, exactly as hdn_conv3x3d_f32: tap-major K, forms A / B / C over M = B So^2
 * pixels by the same rule, K split into at most 16 slices of whole steps into `ws` [z][M][CO] with a finish pass in slice order.  No atomics.
 * hdn_conv3x3v_workspace_bytes / hdn_conv3x3v_form: as the dilated kernel's queries, with `stride` in place of `dilation`; host only.
 * Takes part in the range guard (hdn_set_check_range) on `x`.  Asynchronous on `stream`; allocates nothing.
 * wpacked: the stream hdn_pack_conv3x3d_f32 wrote from the BatchNorm-folded w (the dilated kernel's stream; there is no second packer).
 * Replaces conv2 + bn2 + relu (`padding = 2 - stride`) and the strided 3x3 downsample branch of layer2's first block,
 * hdn/models/backbone/resnet_atrous.py:70-81, 162-174 (eval mode only).
 */
long long hdn_conv3x3v_workspace_bytes(int B, int S, int CI, int CO, int stride);               /* resnet_atrous.py:70-81, 162-174 */
int hdn_conv3x3v_form(int B, int S, int CI, int CO, int stride);                                /* resnet_atrous.py:70-81, 162-174 */
int hdn_conv3x3v_f32(const float* x, const void* wpacked, const float* bias, float* out, void* ws, long long ws_bytes, int B, int S, int CI, int CO,
                     int stride, int relu, int act_domain, void* stream);                       /* resnet_atrous.py:70-81, 162-174 */

/*
 * Training the valid stride-1 convolution above — the heads' Conv2d(CI, CO, 3, bias=False) in front of the correlations, hdn/models/head/ban.py:55-64,
 * ban_lp.py:17-26 (conv3x3_train.hip, conv3x3d.hip; additions to ABI 10).  Everything below is asynchronous on `stream`, allocates nothing, reads
 * nothing back and can be captured into a graph.  The forward is hdn_conv3x3v_f32(stride 1, relu 0, bias NULL) on the mode-0 stream.
 *
 * hdn_pack_conv3x3d_dev_f32: hdn_pack_conv3x3d_f32 on the DEVICE.  w: device pointer to plain [CO][CI][3][3] fp32; out: device buffer of
 *   hdn_pack_conv3x3d_bytes(CO, CI) bytes, 16-byte aligned (else HDN_E_LIMIT), not overlapping w (HDN_E_ALIAS).  mode 0: byte for byte the stream the host
 *   packer writes from w; mode 1: the stream the host packer would write for w'[ci][co][ky][kx] = w[co][ci][2 - ky][2 - kx] (CO and CI swap roles:
 *   the operand of hdn_conv3x3v_dgrad_f32); another mode, CO or CI no positive multiple of 32, a wrong out_bytes: HDN_E_SHAPE; NULL w or out: HDN_E_NULL.
 *   RANGE.  The host packers return HDN_E_LIMIT for a weight with |w| >= 65,504 or NaN.  A device packer cannot raise inside a capture: it converts as
 *   v_cvt_f16_f32 converts (inf / NaN pieces, which propagate into every output they enter) and ADDS the number of such weights to *bad_count, an int
 *   on the device that the caller zeroes and reads outside a capture (integer atomic adds: the count does not depend on their order); may be NULL.
 *
 * hdn_grad_scale_f32: one pass over g[n] that writes ONE int to the device, the exponent e with amax 2^e in [2^14, 2^15), amax = max |g|:
 *   e = 141 - (the 8-bit exponent field of amax), so scaling g by a power of two shifts e and changes nothing else; e = 0 when amax is 0, inf or NaN (a
 *   NaN anywhere in g counts as amax); a subnormal amax counts as the smallest normal number (e = 140).  The maximum is taken over bit patterns with
 *   integer operations — the same in any order, no float atomics.  g 16-byte aligned (HDN_E_LIMIT), n >= 1 (HDN_E_SHAPE), exp_out not inside g (HDN_E_ALIAS).
 *   With this e every element v of g is carried by its two fp16 pieces within max(2^-22 |v|, 2^-50 amax).
 *
 * hdn_conv3x3v_dgrad_f32: gx[B,S,S,CI] = the FULL correlation (padding 2) of dy[B,So,So,CO], So = S - 2, with the mode-1 stream `wpacked_t` — the third
 *   pixel map of conv3x3d.hip's kernel: output side So + 2, tap (ky, kx) of output pixel (y, x) reads dy at (y + ky - 2, x + kx - 2) when that is inside
 *   the image.  dy is split as dy 2^e with e = *exp (device pointer, what hdn_grad_scale_f32 wrote for dy), the join multiplies by 2^-e: both exact.
 *   Forms A / B / C over M = B S^2 pixels, N = CI, K = 9 CO in tap-major steps, K split and finish pass exactly as hdn_conv3x3v_f32; the summation order
 *   depends on (B, S, CI, CO) only.  S >= 3, B >= 1, CI and CO positive multiples of 32 (HDN_E_SHAPE); more than 2^31 - 1 elements in dy or gx, a
 *   pointer that is not 16-byte aligned, a workspace too small: HDN_E_LIMIT; gx overlapping dy, exp or ws, ws overlapping dy: HDN_E_ALIAS; NULL dy,
 *   wpacked_t, exp, gx, or ws where one is needed: HDN_E_NULL.  No range guard: a gradient is scaled by its own amax.
 *
 * hdn_conv3x3v_wgrad_f32: gw[co][ci][ky][kx] = sum over (b, oy, ox) of dy[b,oy,ox,co] x[b,oy+ky,ox+kx,ci], plain [CO][CI][3][3] fp32 (what weight.grad
 *   is), x[B,S,S,CI] and dy[B,So,So,CO] channels-last.  Both operands are split in the kernel (x as activations, 2^-8, inside the range guard on x; dy by
 *   *exp), three piece products into hi / lo accumulators.  K is the pixel axis: it walks in units of (8 consecutive images, one output row), a unit in
 *   segments of 8 output pixels whose dy tile and 3 x 10 x halo are staged once for all nine taps; workgroups of W = 4 / 2 / 1 waves (the largest W with
 *   32 W dividing CO) own 32 W x 32 (co, ci) x 9 taps; K is split into at most 16 slices of whole units that write partial sums to `ws` [z][CO][CI][3][3]
 *   and a finish pass adds them in slice order.  Deterministic, no atomics; the summation order depends on (B, S, CI, CO) only.  Checks as dgrad's, with
 *   x in place of wpacked_t and gw in place of gx.
 *
 * *_workspace_bytes: bytes needed, 0 = none (ws may be NULL then), negative = HDN_E_*.  *_form: the launch form, for tests and profiles (no part of the
 *   ABI): dgrad as hdn_conv3x3v_form; wgrad W | (K slices) << 16.  Host only.
 */
int hdn_pack_conv3x3d_dev_f32(const float* w, int CO, int CI, int mode, void* out, long long out_bytes, int* bad_count, void* stream);  /* ban.py:55-64 */
int hdn_grad_scale_f32(const float* g, long long n, int* exp_out, void* stream);                                                        /* ban.py:55-64 */
long long hdn_conv3x3v_dgrad_workspace_bytes(int B, int S, int CI, int CO);                                                             /* ban.py:55-64 */
int hdn_conv3x3v_dgrad_form(int B, int S, int CI, int CO);                                                                              /* ban.py:55-64 */
int hdn_conv3x3v_dgrad_f32(const float* dy, const void* wpacked_t, const int* exp, float* gx, void* ws, long long ws_bytes, int B, int S, int CI, int CO,
                           void* stream);                                                                                               /* ban.py:55-64 */
long long hdn_conv3x3v_wgrad_workspace_bytes(int B, int S, int CI, int CO);                                                             /* ban.py:55-64 */
int hdn_conv3x3v_wgrad_form(int B, int S, int CI, int CO);                                                                              /* ban.py:55-64 */
int hdn_conv3x3v_wgrad_f32(const float* x, const float* dy, const int* exp, float* gw, void* ws, long long ws_bytes, int B, int S, int CI, int CO,
                           void* stream);                                                                                               /* ban.py:55-64 */

/*
 * BatchNorm2d on batch statistics, optionally followed by ReLU, forward and backward — the pair between a head branch's 3x3 convolution and its
 * correlation, hdn/models/head/ban.py:55-64, ban_lp.py:17-26 (bn_train.hip; additions to ABI 10).  One BatchNorm over N = B P values per channel, P the
 * pixel count of one image; c is the pre-normalisation map, channels-last, [N][C] row-major:
 *   mean = sum c / N                 var = sum (c - mean)^2 / N   (biased)
 *   invstd = 1 / sqrt(var + eps)     alpha = gamma invstd
 *   z = (c - mean) alpha + beta      y = relu ? max(z, 0) : z     (subtract first, then one fma; a NaN z stays a NaN in y)
 *   backward, dz = dy [z > 0] (relu) or dy, the mask recomputed from c by the same statement of z:
 *   S1 = sum dz    S2 = sum dz x^,  x^ = (c - mean) invstd    dbeta = S1    dgamma = S2    dc = alpha (dz - S1 / N - x^ S2 / N)
 * Sums over pixels are float64 from the product on, rounded to fp32 once; fixed order, no atomics: two calls give the same bits, and the order
 * depends on (B, P, C) and the launch form only (the form on (B, P, C) and the measurement switch below).
 * Layouts: c and dc channels-last, 16-byte aligned.  y / dy by flag: 0 channels-last (16-byte aligned), 1 NCHW planes y[(b C + ch) P + p] (4-byte
 * aligned).  stats: mean[C], invstd[C], written by the forward, read by the backward.  running_mean / running_var: NULL (track_running_stats=False) or
 * updated in place, r = (1 - momentum) r + momentum s with s = mean or var N / (N - 1), in float64 from the float64 statistics, rounded once.
 * Backward: a NULL gradient output is neither computed nor written; with dc NULL the apply pass is skipped; all three NULL: HDN_E_SHAPE.
 * Checks, in this order: a required pointer NULL (ws where the form needs one): HDN_E_NULL; B, P or C not positive, C no multiple of 32, N < 2, a flag
 * outside 0 / 1, eps <= 0, momentum outside [0, 1]: HDN_E_SHAPE; C > 2048, N C > 2^31 - 1, c / dc / ws (or a channels-last y / dy) not 16-byte aligned,
 * ws too small: HDN_E_LIMIT; an output's byte range (y, stats, the running buffers, dc, dgamma, dbeta, ws) overlapping an input's or another
 * output's: HDN_E_ALIAS.  Asynchronous on `stream`, allocates nothing, reads nothing back: can be captured into a graph.
 * hdn_bn_relu_train_workspace_bytes: bytes needed by either direction, 0 = none (ws may be NULL), negative = HDN_E_*.  hdn_bn_relu_train_form: the launch
 * form (0: one launch, a workgroup per 32 channels through statistics and normalisation; 1: partial sums, finish, apply), for tests and profiles, no
 * part of the ABI.  Both host only.
 * Measurement switch: the environment variable HDN_BN_TRAIN_FUSED_ROWS (a positive integer), read by the query, the form function and both entry
 * points at every call, replaces the row count up to which form 0 is used (tools/head_bn_train_bench.py forces either form with it).  It is no
 * tuning knob: leave it unset.  Whoever changes it between a workspace query and its launch gets HDN_E_LIMIT or NULL checks as for any wrong
 * workspace; between two calls, another launch form and with it another (still fixed) summation order.
 */
long long hdn_bn_relu_train_workspace_bytes(int B, int P, int C);                                                                      /* ban.py:55-64 */
int hdn_bn_relu_train_form(int B, int P, int C);                                                                                        /* ban.py:55-64 */
int hdn_bn_relu_train_fwd_f32(const float* c, const float* gamma, const float* beta, float* y, float* stats, float* running_mean_or_null,
                              float* running_var_or_null, double momentum, double eps, void* ws, long long ws_bytes, int B, int P, int C, int relu,
                              int y_layout, void* stream);                                                                              /* ban.py:55-64 */
int hdn_bn_relu_train_bwd_f32(const float* dy, const float* c, const float* gamma, const float* beta, const float* stats, float* dc_or_null,
                              float* dgamma_or_null, float* dbeta_or_null, void* ws, long long ws_bytes, int B, int P, int C, int relu, int dy_layout,
                              void* stream);                                                                                            /* ban.py:55-64 */

/*
 * First stage of the similarity branch's ResNet-50 in one launch (simi_stem.hip; an addition to ABI 10):
 *   out[B,Sp,Sp,64] = maxpool3x3/s2/p1( relu( conv7x7 / s2 / p0 (x[B,3,S,S], w[64][3][7][7]) + bias[co] ) ),  Sc = (S - 7) / 2 + 1,  Sp = (Sc - 1) / 2 + 1,
 * x NCHW fp32, out channels-last fp32 (255 -> 125 -> 63, 127 -> 61 -> 31).  Square inputs with 7 <= S <= 255: S < 7, B <= 0 or act_domain != 0 (the
 * HIP backbone runs in real units): HDN_E_SHAPE; S > 255, more than 2^31 - 1 elements in x, wpacked or out not 16-byte aligned: HDN_E_LIMIT; `out`
 * overlapping `x`: HDN_E_ALIAS; a NULL pointer (bias included): HDN_E_NULL.  The Sc x Sc x 64 convolution map stays in the workgroup (registers / LDS);
 * the pool needs no -inf: behind the ReLU everything is >= 0 and every window holds a real element.
 * fp32 carried as two fp16 pieces (pixels split as x 2^-8), three products, hi / lo fp32 accumulators: the error of an fp32 convolution.
 * Deterministic: a conv output is the sum over k steps 0 .. 10 (k = 16 step + 8 g + j <-> ci * 7 + ky = 2 step + g, kx = j) into zeroed accumulators,
 * joined, + bias; the order depends neither on B nor on the workgroup (image, pooled row, channel half) that computes it, so an image gives the same bits
 * at any batch size.  Takes part in the range guard (hdn_set_check_range) on `x`.  Asynchronous on `stream`; allocates nothing; no workspace.
 * wpacked: the stream hdn_pack_simi_stem_f32 wrote from the BatchNorm-folded w, 45,056 bytes, 16-byte aligned.  Current order, informative:
 * [11 k steps][2 n tiles][2 pieces][64 lanes = (k half g, n)][8] fp16: element j is piece pc (p0 = fp16(w), p1 = fp16((w - p0) * 2048)) of
 * w[co = 32 tile + n][ci][ky][kx = j], ci * 7 + ky = 2 * k step + g; 0 at j = 7 and at 2 * k step + g = 21.
 * Replaces conv1 / bn1 / relu / maxpool of hdn/models/backbone/resnet_atrous.py:117-121, 186-189 (eval mode only; a network that returns the stem's
 * own output, `0 in used_layers`, keeps the unfused stem).
 */
long long hdn_pack_simi_stem_bytes(void);                                                       /* resnet_atrous.py:117-121 */
int hdn_pack_simi_stem_f32(const float* w, void* out, long long out_bytes);                     /* resnet_atrous.py:117-121 */
int hdn_simi_stem_f32(const float* x, const void* wpacked, const float* bias, float* out, int B, int S, int act_domain, void* stream);   /* resnet_atrous.py:117-121, 186-189 */

/* The compile-time exponent of the activation scale (csrc/mfma_split.h, HDN_ACT_SCALE_LOG2; 8): callers that hand over pre-scaled biases in
 * act_domain = 1 check it against the value they scale with (hdn_amd.trunk.ACT_SCALE_LOG2). */
int hdn_act_scale_log2(void);

/*
 * The same convolutions chained (ABI 5, the tracker's B = 1, where every launch is a dependent step of ~5 us and the launches that only
 * add K slices up were half of the trunk's): a convolution writes its raw K-slice sums and the NEXT convolution finishes them while it
 * stages its input, so a BasicBlock is two launches instead of four.
 *   hdn_conv3x3_chain_slices(B, S, CI, stride): z >= 1, the number of slices hdn_conv3x3_chain_f32 writes for this problem.
 *   hdn_conv3x3_chain_f32: out_slices[z][B,S,S,CO] = the K slices of conv3x3/stride/p1(X, W) without bias (stride 2: CO = 2 CI and
 *     out_ds_slices[z][B,S,S,CO] = the slices of the 1x1 / stride-2 downsample branch), where the input X [B, S stride, S stride, CI] is
 *       x_slices == 0: the activation x itself (x_bias / x_res / x_out NULL), or
 *       x_slices  > 0: relu(sum of x[0 .. x_slices) in slice order + x_bias[c] (+ the residual)), x = the slices a previous call wrote;
 *                      x_res: the residual as res_slices >= 1 arrays like X, added up in slice order (1: an activation; more: the
 *                      out_ds_slices of the block's first convolution), NULL with res_slices == 0 for none;
 *                      x_out (optional): X is also written here, once (the next block's residual).
 *     The arithmetic and its order are those of hdn_conv3x3_bias_relu_f32's reduction launch: the chain is bit-identical to the
 *     unchained calls.
 *   hdn_conv3x3_finish_f32: out[B,S,S,C] = relu(sum of slices[0 .. n_slices) + bias[c] (+ residual as above)): the end of a chain.
 * Same shapes, packing and value range as above; pointers 16-byte aligned; out_slices / x_out must not alias an input.
 */
int hdn_conv3x3_chain_slices(int B, int S, int CI, int stride);
int hdn_conv3x3_chain_f32(const float* x, int x_slices, const float* x_bias, const float* x_res, int res_slices, float* x_out, const void* wpacked,
                          float* out_slices, float* out_ds_slices, int B, int S, int CI, int stride, int act_domain, void* stream);
int hdn_conv3x3_finish_f32(const float* slices, int n_slices, const float* bias, const float* res, int res_slices, float* out, int B, int S, int C,
                           void* stream);

/*
 * Multi-GPU: template/search pairs are independent, so ranks own disjoint contiguous blocks of pairs
 * and the path's ONLY exchange is one all-gather of the predicted corner offsets, on RCCL over xGMI.
 *   local[Bl,8] (this rank's offsets) -> all[world*Bl,8] on every rank, in rank order; Bl must be equal on all
 *   ranks (pad ragged shards: hdn_amd.dist does); in place iff local == all + rank*Bl*8.
 * rccl_comm is an ncclComm_t (from hdn_rccl_comm_create below, or any communicator of the process's RCCL);
 * asynchronous on `stream` like every other entry point.
 * The reference has no inference-time collective (its multi-GPU evaluation is manual video ranges per
 * CUDA_VISIBLE_DEVICES, tools/test.py:49,91-103); this replaces the host-side concatenation a batched caller of
 * HomoModelBuilder.forward (homo_model_builder.py:161-165: x = fc(...)) would do.
 */
int hdn_allgather_offsets(const float* local, float* all, int Bl, void* rccl_comm, void* stream);

/* Communicator plumbing for hosts without torch.distributed: rank 0 fills a 128-byte id, ships it to the other ranks
 * by any means (file, socket, MPI, torch's store), every rank creates its communicator on its current device.
 * RCCL is loaded on first use (dlopen "librccl.so.1", or $HDN_RCCL_LIB); hdn_rccl_available() reports whether it was. */
#define HDN_RCCL_UNIQUE_ID_BYTES 128
int hdn_rccl_available(void);
int hdn_rccl_unique_id(void* id128);
int hdn_rccl_comm_create(void** comm_out, int world, int rank, const void* id128);
int hdn_rccl_comm_count(void* comm, int* count);   /* ncclCommCount: the ranks RCCL itself sees (ABI 6) */
int hdn_rccl_comm_destroy(void* comm);

/*
 * Measurement aid (bench.py `roofline.measured_copy_GBps`; SURVEY.md section 8d asks for a measured device-copy bandwidth beside the
 * nominal 8 TB/s): dst[0..n) = src[0..n), 16 bytes per lane, nontemporal on both sides, 8,192 workgroups.  n % 4 == 0, 16-byte aligned
 * pointers, no overlap.  Asynchronous on `stream`; moves 2 * 4 * n bytes.
 */
int hdn_ubench_copy_f32(const float* src, float* dst, long long n, void* stream);

/*
 * The same exchange as ONE kernel per rank and one xGMI hop, for a fully connected node (for 2 KB per rank a
 * direct one-shot gather beats a ring): every rank owns a window of uncached device memory that its peers map through
 * hipIpc handles; a call stores the local slice straight into every peer's window, raises a flag there, waits for the peers'
 * flags in its own window and copies the slices out.  No RCCL, no host thread in the data path, no host state per call
 * (the call counter lives in the window), so the launch can sit inside a hipGraph.
 *   hdn_gather_create   window on the CURRENT device: world <= 16 ranks, slot_bytes (multiple of 16) = the largest local slice
 *   hdn_gather_handle   this rank's 64-byte hipIpcMemHandle_t; ship all of them to all ranks (any means), in rank order
 *   hdn_gather_connect  maps the peers' windows (handles[world][64]; the own entry is ignored); collective, once
 *   hdn_gather_offsets_oneshot  local[Bl,8] -> all[world*Bl,8], same contract as hdn_allgather_offsets (Bl equal on all ranks,
 *                       Bl*32 <= slot_bytes, 16-byte aligned pointers, no overlap); asynchronous on `stream`.  A peer that does
 *                       not show up within 2 s makes the kernel give up: that peer's rows of `all` are NaN, hdn_gather_status()
 *                       is non-zero from then on (sticky; read it at the next synchronisation point) and every later call on
 *                       the context returns HDN_E_PEER — the two-parity protocol cannot survive a wait that ended without its flag.
 *   hdn_gather_status   0, or the sticky error bits (1 = a wait timed out); a host read of pinned memory, no synchronisation
 *   hdn_gather_destroy  synchronises the own device, unmaps and frees.  The peers must have stopped calling and their launches
 *                       must have completed (device synchronisation + a group barrier on every rank first).
 *   hdn_gather_peer_access / hdn_device_pci_bus_id   before creating the windows: can `device` reach the device a peer reported
 *                       by PCI bus id (1 / 0; HDN_E_SHAPE = not visible to this process)?  hdn_amd.dist.OneShotGather falls back
 *                       to RCCL with a warning unless every pair of ranks answers 1.
 * Every rank must make the same sequence of calls.  Validated with two processes sharing one device (tests/test_gpu_dist.py);
 * across devices it needs peer access over xGMI (hipIpcMemLazyEnablePeerAccess) and has not been run.
 */
#define HDN_IPC_HANDLE_BYTES 64
int hdn_gather_create(void** ctx_out, int world, int rank, long long slot_bytes);
int hdn_gather_handle(void* ctx, void* handle64);
int hdn_gather_connect(void* ctx, const void* handles);
int hdn_gather_offsets_oneshot(void* ctx, const float* local, float* all, int Bl, void* stream);
int hdn_gather_status(void* ctx);
int hdn_gather_destroy(void* ctx);
int hdn_gather_peer_access(int device, const char* peer_pci_bus_id);
int hdn_device_pci_bus_id(int device, char* out, int len);

#ifdef __cplusplus
}
#endif
#endif /* HDN_HIP_H */

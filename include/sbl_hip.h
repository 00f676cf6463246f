/* libsbl_hip.so — C ABI of the MI355X-native (gfx950) SBL lip-reading hot path.
 *
 * The reference (VIPL SBL_For_Multilingual_Lip_Reading) has no FFI: its boundary is the
 * Python class surface of SBL_Multilingual_Lip_reading/transformer/ ("SBL/..." below).
 * Each entry point here replaces the torch ops one reference call site issues; the Python
 * mirror (sbl_for_multilingual_lip_reading_amd/transformer/) binds them through ctypes
 * (see INTEGRATION.md for the stub a maintainer adds to the reference).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless marked host.
 *   - the CALLER allocates every output and workspace; nothing is allocated inside.
 *   - every call only enqueues work on `stream` (hipStream_t passed as void*): no sync, no
 *     host read-back, so any sequence of calls can be captured into a hipGraph.
 *   - return 0 on success, otherwise a hipError_t value or SBL_ERR_INVALID (bad shape /
 *     alignment, checked on the host BEFORE any launch); text via sbl_last_error()
 *     (thread-local).  Safe from several host threads on distinct streams/devices (nn.DataParallel's
 *     threading model, SBL/train.py:115).  The only mutable state is a handful of process-wide settings, all
 *     read when a launch is enqueued, so one thread's change reaches every thread's later launches: the
 *     matrix-product precision, the two routing switches of sbl_set_tuning and the profile stamps.
 *   - activations of the visual trunk are NHWC ("channels last"): (image, h, w, c), image =
 *     n*T + t — the reference's transpose/contiguous/view (SBL/transformer/video_frontend.py:113-115)
 *     is folded into the layout.  Transformer tensors are row-major (B, L, 512).
 *   - tensors are fp32 in memory everywhere (the reference's dtype).  The arithmetic of the matrix products of the
 *     tile engine is a process-wide setting, sbl_set_matmul_precision() below: exact fp32 MFMA
 *     (v_mfma_f32_32x32x2_f32, the library default) or split-bf16 MFMA with fp32 accumulation.  The setting is read
 *     when a launch is ENQUEUED: a captured hipGraph keeps the mode it was captured under, whatever is set later.
 */
#ifndef SBL_HIP_H
#define SBL_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SBL_ERR_INVALID (-22)
#define SBL_ABI_VERSION 1

typedef void* sbl_stream_t; /* hipStream_t */

const char* sbl_last_error(void);
int sbl_abi_version(void);

/* Bench instrumentation (debug; process-wide): between begin/end every GEMM / convolution launch gets a slot
 * stamps[2*slot] = min start, stamps[2*slot+1] = max end of its workgroups, in 100 MHz s_memrealtime ticks
 * (caller pre-fills starts with ~0 and ends with 0).  The slot pointer is baked into the launch, so stamps are
 * taken inside hipGraph replays too.  sbl_profile_last_slot/kernel report the launch just enqueued by this thread
 * (slot -1 = not instrumented; kernel 1 skinny GEMM, 2 tiled 64x64, 3 tiled 128x128, 4/5/6 conv fwd/dgrad/wgrad,
 * 7 merged decoder/encoder weight gradients); sbl_profile_used = slots handed out so far by ALL threads (autograd
 * runs backward on its own thread, so a caller brackets a call with it to learn which slots the call used). */
int sbl_profile_begin(uint64_t* stamps, int capacity);
int sbl_profile_end(void);
int sbl_profile_used(void);
int sbl_profile_last_slot(void);
int sbl_profile_last_kernel(void);
/* The launch leaf the last trunk convolution - or sbl_gemm2_rows_f32 call, family 9, described there - enqueued by this
 * thread took (debug; 0 before the first one):
 *   (family << 24) | (tile << 20) | (TR << 10) | G
 *   family  1 per-tap gather, one plain launch         2 per-tap gather, tail split (two launches)
 *           3 position-major forward / input gradient  4 patch-resident forward / input gradient
 *           5 stride-2 parity classes (one launch)     6 patch-resident weight gradient
 *           7 position-major weight gradient           8 plain implicit-GEMM weight gradient
 *   tile    1 = 64x64, 2 = 128x64, 3 = 128x128; 0 for the patch-resident kernels (families 4 and 6), which report the tile
 *           geometry they chose instead: TR rows of one image (G == 1) or G whole images (TR == H); TR = G = 0 elsewhere. */
int sbl_profile_last_route(void);

/* Precision of the matrix products of the tile engine (dense GEMMs and trunk convolutions), process-wide, default 0:
 *   0  exact fp32 MFMA (v_mfma_f32_32x32x2_f32), bitwise an fmaf chain — the reference's arithmetic;
 *   6  every operand split exactly into three bf16 planes on the way into LDS, six bf16 MFMA products per fp32
 *      product (all plane pairs of weight >= 2^-16), fp32 accumulation: fp32-grade results (dropped terms <= 2^-26
 *      per product) at 6 x 32 instead of 8 x 64 MFMA cycles per 32x32x16 block;
 *   3  two planes, three products (~2^-17 per product);   1  plain bf16 inputs with fp32 accumulation — BASELINE
 *      config 5 "mixed bf16" (fp32 master weights, fp32 accumulate).
 * Inputs and outputs stay fp32 in memory in every mode.  Returns SBL_ERR_INVALID for any other value.
 * Dense products small enough for the register-only skinny kernel (skinny_gemm.h; sbl_profile_last_kernel() == 1) are
 * multiplied in exact fp32 in EVERY mode: the setting reaches the tiled kernels only.
 * The value is read at enqueue time and baked into captured hipGraphs (re-capture after changing it).  Mode 6's
 * "exact split" holds for |x| >= 2^-110 or x == 0; residual planes of smaller magnitudes underflow bf16's range. */
int sbl_set_matmul_precision(int terms);
int sbl_get_matmul_precision(void);
/* Routing switches (process-wide, read at enqueue time like the precision).  Each chooses between two shipped kernel
 * families for the 3x3 / stride-1 trunk convolutions in the split-bf16 modes; the suite uses them to run the second
 * family on the large maps.  Any other knob, or a value a knob does not take, returns SBL_ERR_INVALID.
 * knob 5: 2 (default) patch-resident forward / input-gradient kernel on every map whose tile sbl_conv_patch_tile accepts; 0
 *         the per-tap gather / position-major kernels.  The tile comes from an LDS budget per bf16 plane, so the maps depend
 *         on the mode: 22x22 and 28x28 (rows of one image) and 11x11 (2 images per tile) in bf16x6, bf16x3 and bf16; 6x6 (7
 *         images), 7x7 (5), 4x4 (16) and 4x5 / 5x4 (12) in bf16x3 and bf16 only; 3x3 (28 images) in bf16 only;
 * knob 9: patch-resident weight gradient for maps of at least `value` pixels (default 30: the 22x22, 11x11 and 6x6
 *         layers; 0 = the implicit-GEMM weight gradients everywhere). */
int sbl_set_tuning(int knob, int value);

/* ---------------------------------------------------------------- dense GEMM / Linear
 * C[M,N] (+)= opA(A)[M,K] * opB(B)[K,N], row-major; opA(A)[m,k] = transA ? A[k*lda+m] : A[m*lda+k],
 * opB(B)[k,n] = transB ? B[n*ldb+k] : B[k*ldb+n].  Epilogue: +bias[n], ReLU, or multiply by
 * (relu_mask[m*ldm+n] > 0) (ReLU backward fused into the producing GEMM).
 * accumulate: 0 = overwrite, 1 = C += (in place: gradients accumulate straight into the flat .grad buffer).
 * a_colsum (transA=1 only, may be NULL): float[M] += sum_k opA(A)[m,k], float atomics — the bias gradient
 *   db = sum_rows dY rides on the weight-gradient GEMM dW = dY^T X.
 * ws / ws_bytes (may be NULL/0): split-K workspace = int[4096] tile counters (zero on first hand-over, left
 *   zero by every call) followed by fp32 partial slabs.  With it, small-M problems split K across workgroups
 *   and the last-arriving workgroup of each tile reduces the slabs and runs the epilogue inside the same
 *   launch; without it split-K falls back to float atomics on C (plain epilogue only).  One workspace per
 *   stream: concurrent calls must not share it.
 * Replaces nn.Linear forward/backward: SBL/transformer/attention.py:16-18,27,41-43,57;
 * module.py:42-43,49; encoder.py:27,54; decoder.py:59-60,166-167. */
int sbl_gemm_f32(int transA, int transB, int M, int N, int K, const float* A, long lda, const float* B, long ldb,
                 float* C, long ldc, const float* bias, int relu, const float* relu_mask, long ldm, int accumulate,
                 float* a_colsum, void* ws, long ws_bytes, sbl_stream_t stream);
/* Two products of one shape in ONE launch: C_d[M,N] = A_d[M,K] * B_d[N,K]^T (+ bias_d) (ReLU), d = 0, 1 - the nn.Linear
 * forward of layer_stack_l2r[i] and layer_stack_r2l[i], which SBL/transformer/decoder.py:121-156 runs back to back on
 * same-shape inputs.  Kernel boundaries cost ~5 us and small launches on two streams do not overlap on this GPU, so
 * the two decoder directions share launches.  Same kernels and workspace convention as sbl_gemm_f32. */
int sbl_gemm2_f32(int M, int N, int K, const float* A0, const float* A1, long lda, const float* B0, const float* B1,
                  long ldb, float* C0, float* C1, long ldc, const float* bias0, const float* bias1, int relu, void* ws,
                  long ws_bytes, sbl_stream_t stream);
/* The same call for the decoder forward, whose small stages (one or two decoding steps, M = 32...128 rows per direction)
 * leave a 32x32 tiling with fewer workgroups than the GPU has CUs.  A launch that is row-starved,
 * 2 * ceil(M/32) * ceil(N/32) < 256 and M <= 128, with K % 16 == 0, 16-byte aligned A and B and lda % 4 == ldb % 4 == 0 runs on 16x16
 * output tiles (one workgroup each, its waves split K; exact fp32 in every precision mode like the skinny kernel, no
 * workspace; sbl_profile_last_kernel() == 1).  Every other call is sbl_gemm2_f32 with the same arguments, bit for bit.
 * sbl_profile_last_route() afterwards: family 9, tile 4 and (NW, U) in the TR / G fields for the 16x16 kernel, tile 0
 * for a forwarded call. */
int sbl_gemm2_rows_f32(int M, int N, int K, const float* A0, const float* A1, long lda, const float* B0, const float* B1,
                       long ldb, float* C0, float* C1, long ldc, const float* bias0, const float* bias1, int relu, void* ws,
                       long ws_bytes, sbl_stream_t stream);
/* Deferred weight gradient of one decoder weight over all stages of a step:
 * C[M,N] += sum_s A_s^T B_s with A_s (seg_rows[s] x M, row stride lda) = dY of stage s and B_s (seg_rows[s] x N) = its
 * input; a_colsum[m] += column sums of the A_s (bias gradient).  A_ptrs / B_ptrs / seg_rows are HOST arrays of nseg
 * <= 16 entries (device pointers inside).  C and a_colsum are accumulated with float atomics (split-K). */
int sbl_wgrad_seg_f32(int nseg, const float* const* A_ptrs, long lda, const float* const* B_ptrs, long ldb,
                      const int* seg_rows, int M, int N, float* C, long ldc, float* a_colsum, sbl_stream_t stream);
/* The same for MANY weights in one launch (all deferred decoder weights of a step): every 128x128 tile of every
 * C_p (+)= sum_s A_{p,s}^T B_{p,s} is owned by one workgroup over the whole K = sum(seg_rows) (no split-K, no
 * atomics on C: deterministic).  All problems share nseg / seg_rows (multiples of 16 rows); A_ptrs / B_ptrs are HOST
 * arrays of nprob*nseg device pointers (problem-major); lda/ldb/M/N/C/ldc/colsum HOST arrays of nprob entries
 * (colsum[p] may be NULL).  table: device scratch of sbl_wgrad_group_table_bytes(nprob) bytes (problem descriptors,
 * written by the call on `stream`). */
long sbl_wgrad_group_table_bytes(int nprob);
int sbl_wgrad_group_f32(int nprob, int nseg, const int* seg_rows, const float* const* A_ptrs, const long* lda,
                        const float* const* B_ptrs, const long* ldb, const int* M, const int* N, float* const* C,
                        const long* ldc, float* const* colsum, void* table, long table_bytes, sbl_stream_t stream);
/* out[n] (+)= sum_m X[m*ldx + n]   (bias gradients) */
int sbl_colsum_f32(const float* X, long ldx, float* out, int M, int N, int accumulate, sbl_stream_t stream);

/* ---------------------------------------------------------------- stem (frontend3D)
 * Conv3d(1,64,(5,7,7),s(1,2,2),p(2,3,3),bias=False) -> BatchNorm3d(64) -> ReLU ->
 * MaxPool3d((1,3,3),s(1,2,2),p(0,1,1)): SBL/transformer/video_frontend.py:99-104.
 * x: (N,T,H,W) fp32 (C=1).  conv_out: (N*T,Ho,Wo,64), Ho=H/2, Wo=W/2.  pooled: (N*T,Ho/2,Wo/2,64).
 * stats: double[128] = per-channel (sum, sumsq) of conv_out; zeroed by the call. */
int sbl_stem_conv_fwd(const float* x, const float* w /*[64][245]*/, float* conv_out, double* stats, int N, int T, int H,
                      int W, sbl_stream_t stream);
int sbl_stem_bn_relu_pool_fwd(const float* conv_out, const float* mean, const float* invstd, const float* gamma,
                              const float* beta, float* pooled, uint8_t* argmax, int NT, int Ho, int Wo,
                              sbl_stream_t stream);
/* backward pass 1: sums = double[128] (sum g, sum g*xhat), g = grad wrt BN output after pool/ReLU adjoints */
int sbl_stem_bwd_reduce(const float* conv_out, const float* dpooled, const uint8_t* argmax, const float* mean,
                        const float* invstd, const float* gamma, const float* beta, double* sums, int NT, int Ho,
                        int Wo, sbl_stream_t stream);
/* backward pass 2: dconv recomputed on the fly and contracted with the input patches:
 * dw[64][245] (zeroed by the call), dgamma[64], dbeta[64].  No input gradient (x is data). */
int sbl_stem_wgrad(const float* x, const float* conv_out, const float* dpooled, const uint8_t* argmax,
                   const float* mean, const float* invstd, const float* gamma, const float* beta, const double* sums,
                   float* dw, float* dgamma, float* dbeta, int N, int T, int H, int W, sbl_stream_t stream);

/* The same two kernels fed by the loader's uint8 frames: the device input pipeline of sbl_preprocess_clips (below) folded
 * into the stem's patch staging, so the fp32 clip (N,Tout,Hc,Wc) never exists - not in HBM, not saved for backward.  The
 * staged value of clip coordinate (n, tt, ih, iw) is lut256[in[n, src_frame[n,tt], y1[n]+ih, x1[n] + (flip[n] ? Wc-1-iw : iw)]]
 * (the table entry itself: no arithmetic on the byte), and 0 where src_frame[n,tt] < 0, in the convolution's padding, and
 * wherever the resolved coordinate leaves the (Tin,Hin,Win) frames - a bad crop origin or frame index reads as zero, never
 * out of bounds.  in, lut256, y1, x1, flip, src_frame: exactly sbl_preprocess_clips' arguments; (Tout,Hc,Wc) take the place
 * of sbl_stem_conv_fwd's (T,H,W) and obey its rules (Hc, Wc multiples of 4, >= 8), Hc <= Hin, Wc <= Win, N*Tin*Hin*Win < 2^31.
 * conv_out / dw are bit-identical to sbl_preprocess_clips + sbl_stem_conv_fwd / sbl_stem_wgrad up to the order of the float
 * atomics (stats, dw), in every sbl_set_matmul_precision mode.  Replaces SBL/data_gen.py:104-108,122-125,276-296 and
 * cvtransforms.py:7-48 (the loader's float pipeline) in front of SBL/transformer/video_frontend.py:99-104. */
int sbl_stem_conv_fwd_u8(const uint8_t* in, const float* lut256, const int* y1, const int* x1, const int* flip,
                         const int* src_frame, const float* w /*[64][245]*/, float* conv_out, double* stats, int N, int Tin,
                         int Hin, int Win, int Tout, int Hc, int Wc, sbl_stream_t stream);
int sbl_stem_wgrad_u8(const uint8_t* in, const float* lut256, const int* y1, const int* x1, const int* flip,
                      const int* src_frame, const float* conv_out, const float* dpooled, const uint8_t* argmax,
                      const float* mean, const float* invstd, const float* gamma, const float* beta, const double* sums,
                      float* dw, float* dgamma, float* dbeta, int N, int Tin, int Hin, int Win, int Tout, int Hc, int Wc,
                      sbl_stream_t stream);

/* ---------------------------------------------------------------- BatchNorm (train / eval)
 * nn.BatchNorm{2,3}d defaults: SBL/transformer/video_frontend.py:21,24,71,101. */
int sbl_bn_finalize(const double* stats /*[2C]*/, long count, float* running_mean, float* running_var,
                    float momentum, float eps, float* save_mean, float* save_invstd, int C,
                    int64_t* num_batches_tracked /* += 1, or NULL */, sbl_stream_t stream);
int sbl_bn_eval_stats(const float* running_mean, const float* running_var, float eps, float* mean, float* invstd,
                      int C, sbl_stream_t stream);
/* y = [relu]( gamma*(x-mean)*invstd + beta [+ res] ), NHWC rows x C */
int sbl_bn_apply_fwd(const float* x, const float* res, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, float* y, long rows, int C, int relu, sbl_stream_t stream);
/* Training form: sbl_bn_finalize folded into the apply launch - mean / invstd are derived from the convolution epilogue's
 * (sum, sumsq) statistics inside the kernel (same double arithmetic), save_mean / save_invstd, the running statistics and
 * num_batches_tracked are written by the same launch.  C/4 must divide 256. */
int sbl_bn_apply_fwd_stats(const float* x, const float* res, const double* stats, long count, float* running_mean,
                           float* running_var, float momentum, float eps, const float* gamma, const float* beta, float* y,
                           float* save_mean, float* save_invstd, int64_t* num_batches_tracked, long rows, int C, int relu,
                           sbl_stream_t stream);
/* sums = double[2C] (sum g, sum g*xhat), g = dy * (y>0 if relu); overwritten by the call.
 * ws: NULL or the calling stream's sbl_gemm_f32 workspace (>= 16 KiB of int counters that are zero between launches,
 * then fp32 scratch): block partials + a last-arriver reduction replace 2C contended double atomics per block.
 * C/4 must divide 256 and C <= 512 (the last-arriver reduction has 256 lanes for the 2C/4 partial columns). */
int sbl_bn_bwd_reduce(const float* dy, const float* y, const float* x, const float* mean, const float* invstd,
                      double* sums, long rows, int C, int relu, void* ws, long ws_bytes, sbl_stream_t stream);
/* dx = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)); dres = g (if non-null); dgamma, dbeta from sums
 * (accumulate != 0: += into the persistent gradient buffers) */
int sbl_bn_bwd_apply(const float* dy, const float* y, const float* x, const float* mean, const float* invstd,
                     const float* gamma, const double* sums, float* dx, float* dres, float* dgamma, float* dbeta,
                     long rows, int C, int relu, int accumulate, sbl_stream_t stream);

/* ---------------------------------------------------------------- ResNet-18 trunk convolutions
 * conv3x3 / 1x1-stride-2, bias-free, NHWC implicit GEMM: SBL/transformer/video_frontend.py:10-12,69-70.
 * Weights are used in OHWI order [Cout][KH][KW][Cin]; pack/unpack convert from/to the
 * reference's OIHW parameter layout (state-dict shapes stay the reference's). */
int sbl_conv_weight_pack(const float* w_oihw, float* w_ohwi, float* w_dgrad /*[Cin][KH][KW][Cout] or NULL*/, int Cout,
                         int Cin, int KH, int KW, double* zero /* nzero doubles set to 0 by the same launch (the BN
                         statistics of the convolution that follows), or NULL */, int nzero, sbl_stream_t stream);
/* accumulate != 0: dw_oihw += (the persistent flat gradient buffer of a data-parallel replica) */
int sbl_conv_wgrad_unpack(const float* dw_ohwi, float* dw_oihw, int Cout, int Cin, int KH, int KW, int accumulate,
                          sbl_stream_t stream);
/* stats: NULL or double[2*Cout] (sum, sumsq of y) accumulated by the epilogue; zeroed by the call unless stats_zeroed.
 * ws / ws_bytes (may be NULL/0): the calling stream's sbl_gemm_f32 workspace.  With it, a launch whose tile count
 * is not a multiple of the 256 CUs runs its last partial round of tiles split along K (in-launch slab reduction). */
int sbl_conv2d_fwd(const float* x, const float* w_ohwi, float* y, double* stats, int stats_zeroed, int NIMG, int H, int W, int Cin,
                   int Cout, int KH, int KW, int stride, int pad, void* ws, long ws_bytes, sbl_stream_t stream);
int sbl_conv2d_dgrad(const float* dy, const float* w_dgrad, float* dx, int NIMG, int H, int W, int Cin, int Cout,
                     int KH, int KW, int stride, int pad, void* ws, long ws_bytes, sbl_stream_t stream);
/* The same, and in its epilogue the reduction pass of the BatchNorm backward that consumes dx: dx is the gradient of
 * act = relu(bn(pre)) (video_frontend.py:31-33: conv1 -> bn1 -> relu feeds conv2), so
 * sums[c] = sum_pixels g, sums[Cin + c] = sum_pixels g * (pre - mean[c]) * invstd[c] with g = dx * (act > 0) - what
 * sbl_bn_bwd_reduce(dx, act, pre, ...) would compute in a separate pass over the three tensors.  Stride 1 only. */
int sbl_conv2d_dgrad_bnstats(const float* dy, const float* w_dgrad, float* dx, int NIMG, int H, int W, int Cin, int Cout,
                             int KH, int KW, int stride, int pad, void* ws, long ws_bytes, const float* act,
                             const float* pre, const float* mean, const float* invstd, double* sums,
                             int sums_zeroed /* sums already hold zeros (a pooled memset): skip the call's own */,
                             sbl_stream_t stream);
/* The general form (any stride; every fused operand may be NULL) - what BasicBlock's backward needs so that no separate
 * pass touches dx (video_frontend.py:28-41):
 *   addend  the residual branch's gradient, added before the store and the sums.  Stride 1: laid out like dx (identity
 *           shortcut).  Stride 2: the COMPACT (NIMG, ceil(H/2), ceil(W/2), Cin) gradient of the 1x1 / stride-2 downsample
 *           branch (sbl_conv1x1s2_dgrad_compact), which lives on the even/even pixels only.
 *   act, pre, mean, invstd  as in sbl_conv2d_dgrad_bnstats: the BatchNorm whose output gradient dx (with the addend) is -
 *           the previous block's bn2; sums[0..2Cin).
 *   pre2, mean2, invstd2    a second BatchNorm fed through the same act (that block's downsample branch):
 *           sums[2Cin..4Cin) = (sum g, sum g * (pre2 - mean2) * invstd2).  sums: double[2*Cin] or double[4*Cin]. */
int sbl_conv2d_dgrad_fused(const float* dy, const float* w_dgrad, float* dx, int NIMG, int H, int W, int Cin, int Cout,
                           int KH, int KW, int stride, int pad, void* ws, long ws_bytes, const float* addend,
                           const float* act, const float* pre, const float* mean, const float* invstd, const float* pre2,
                           const float* mean2, const float* invstd2, double* sums, int sums_zeroed, sbl_stream_t stream);
/* Input gradient of the 1x1 / stride-2 downsample convolution on its own support: dx_compact (NIMG, ceil(H/2), ceil(W/2),
 * Cin) = dy (NIMG, ceil(H/2), ceil(W/2), Cout) * w; the other three quarters of the full-size gradient are zeros that
 * nobody needs to write (sbl_conv2d_dgrad_fused adds the compact form to conv1's gradient). */
int sbl_conv1x1s2_dgrad_compact(const float* dy, const float* w_dgrad, float* dx_compact, int NIMG, int H, int W, int Cin,
                                int Cout, void* ws, long ws_bytes, sbl_stream_t stream);
/* dw_ohwi zeroed by the call (unless dw_zeroed: the caller hands over zeros), then split-K float atomics */
int sbl_conv2d_wgrad(const float* x, const float* dy, float* dw_ohwi, int NIMG, int H, int W, int Cin, int Cout,
                     int KH, int KW, int stride, int pad, int dw_zeroed, sbl_stream_t stream);
/* AdaptiveAvgPool2d(1): (NIMG,HW,C) -> (NIMG,C): video_frontend.py:53,87-88 */
int sbl_avgpool_fwd(const float* x, float* y, int NIMG, int HW, int C, sbl_stream_t stream);
int sbl_avgpool_bwd(const float* dy, float* dx, int NIMG, int HW, int C, sbl_stream_t stream);

/* ---------------------------------------------------------------- dropout (fused Philox-style masks)
 * y = x * keep / (1-p); the mask is a function of (*seed, offset, element index) and is
 * regenerated in backward.  F.dropout(p=0.5) video_frontend.py:122; nn.Dropout(0.1) x80. */
int sbl_dropout(const float* x, float* y, long n, float p, const uint64_t* seed, uint64_t offset,
                sbl_stream_t stream);
int sbl_seed_bump(uint64_t* seed, sbl_stream_t stream);

/* ---------------------------------------------------------------- LayerNorm with fused residual
 * y = LN(x + res) * gamma + beta (eps 1e-5), rows of D=512: attention.py:58, module.py:51, encoder.py:54. */
/* With drop_p > 0 the sub-layer's dropout is fused: y = LN(dropout(x) + res) (attention.py:57-58,
 * module.py:50-51); the mask is a function of (*seed, offset, element index). */
int sbl_add_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* y,
                          float* mean, float* rstd, int M, int D, float eps, float drop_p, const uint64_t* seed,
                          uint64_t offset, sbl_stream_t stream);
/* sbl_add_layernorm2_fwd followed by the SBL cross-direction fusion (SBL/transformer/module.py:50-51 then decoder.py:127-143)
 * in one launch: xn0 = A + flip(B), xn1 = 2B + flip(A), A / B = the two directions' LayerNorm(dropout(x_d) + res_d) rows of a
 * ragged stage (B sequences per segment of length seg_L[s]; flip along each sequence's own prefix).  A / B are not stored. */
int sbl_add_layernorm2_fusion_fwd(const float* x0, const float* x1, const float* res0, const float* res1, const float* gamma0,
                                  const float* gamma1, const float* beta0, const float* beta1, float* xn0, float* xn1, float* mean0,
                                  float* mean1, float* rstd0, float* rstd1, int B, const int* seg_L, int nseg, int D, float eps,
                                  float drop_p, const uint64_t* seed, uint64_t offset0, uint64_t offset1, sbl_stream_t stream);
/* The same for two same-shape problems (the two decoder directions) in one launch. */
int sbl_add_layernorm2_fwd(const float* x0, const float* x1, const float* res0, const float* res1, const float* gamma0,
                           const float* gamma1, const float* beta0, const float* beta1, float* y0, float* y1, float* mean0,
                           float* mean1, float* rstd0, float* rstd1, int M, int D, float eps, float drop_p,
                           const uint64_t* seed, uint64_t offset0, uint64_t offset1, sbl_stream_t stream);
/* dz = gradient of the LayerNorm input (= dres); dx_drop (may be NULL) = gradient of the pre-dropout x;
 * dgamma/dbeta accumulated with float atomics (caller zeroes, or passes the .grad buffers to accumulate) */
int sbl_add_layernorm_bwd(const float* dy, const float* x, const float* res, const float* gamma, const float* mean,
                          const float* rstd, float* dz, float* dx_drop, float* dgamma, float* dbeta, int M, int D,
                          float drop_p, const uint64_t* seed, uint64_t offset, sbl_stream_t stream);
/* y = x + pe[l] (l = row % L) : encoder.py:53-55 positional add */
int sbl_add_pe(const float* x, const float* pe, float* y, int B, int L, int D, sbl_stream_t stream);

/* y[m,:] = x[m,:] * s[m]: the `*= non_pad_mask` of encoder.py:86,89 / decoder.py:399,403,406 (ragged lengths) */
int sbl_rowscale(const float* x, const float* s, float* y, long M, int D, sbl_stream_t stream);

/* ---------------------------------------------------------------- scaled dot-product attention
 * One workgroup per (batch, head): S = Q K^T * scale, mask, softmax over keys, [dropout], O = P V.
 * q/k/v/o are (B, L, H*64) row-major views with row strides ldq/ldk/ldv/ldo (heads are the
 * contiguous 64-wide column blocks: attention.py:41-47); p_out is (H*B, Lq, Lk) head-major like
 * the reference's returned attn.  mask_kind: 0 none, 1 causal (key > query masked:
 * utils.py:116-124), 2 explicit uint8 (B,Lq,Lk), nonzero = masked.  Lq, Lk <= 64, d = 64.
 * A query row whose keys are all masked gets p = 0 and o = 0 (the reference's softmax of such a row is NaN); in backward
 * its dq row is 0 and it adds nothing to dk / dv.
 * Replaces attention.py:72-83. */
int sbl_attention_fwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* o, long ldo,
                      float* p_out, int mask_kind, const uint8_t* mask, int B, int H, int Lq, int Lk, float scale,
                      float drop_p, const uint64_t* seed, uint64_t offset, sbl_stream_t stream);
int sbl_attention_bwd(const float* dout, long lddo, const float* q, long ldq, const float* k, long ldk, const float* v,
                      long ldv, const float* p, float* dq, long lddq, float* dk, long lddk, float* dv, long lddv,
                      int B, int H, int Lq, int Lk, float scale, float drop_p, const uint64_t* seed, uint64_t offset,
                      sbl_stream_t stream);

/* Ragged ("segmented") forms.  A run of decoder steps whose input tokens are all known (teacher-forced) has no
 * step-to-step dependency (decoder.py:176-186 feeds back the argmax only when the coin says so), so the run is
 * processed as ONE batch: segment s = the step with prefix length seg_L[s]; its B*seg_L[s] rows follow segment
 * s-1's rows, in (b, l) order.  seg_L is a HOST array of nseg <= 16 lengths.  Lk_fixed == 0: self-attention inside
 * each segment; Lk_fixed > 0: all segments attend to the same (B, Lk_fixed) key/value rows (cross-attention); in
 * backward the segments' dk/dv contributions are summed inside the call (dq, dk, dv are always overwritten).
 * p_out holds the segments' (H*B, L, Lk) probability blocks back to back. */
int sbl_attention_seg_fwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* o,
                          long ldo, float* p_out, int mask_kind, const uint8_t* mask, int B, int H, const int* seg_L,
                          int nseg, int Lk_fixed, float scale, float drop_p, const uint64_t* seed, uint64_t offset,
                          sbl_stream_t stream);
/* sbl_attention_seg_fwd for two same-shape problems (the two decoder directions) in one launch; mask_kind 0 or 1. */
int sbl_attention_seg2_fwd(const float* q0, const float* q1, long ldq, const float* k0, const float* k1, long ldk,
                           const float* v0, const float* v1, long ldv, float* o0, float* o1, long ldo, float* p_out0,
                           float* p_out1, int mask_kind, int B, int H, const int* seg_L, int nseg, int Lk_fixed, float scale,
                           float drop_p, const uint64_t* seed, uint64_t offset0, uint64_t offset1, sbl_stream_t stream);
int sbl_attention_seg_bwd(const float* dout, long lddo, const float* q, long ldq, const float* k, long ldk, const float* v,
                          long ldv, const float* p, float* dq, long lddq, float* dk, long lddk, float* dv, long lddv,
                          int B, int H, const int* seg_L, int nseg, int Lk_fixed, float scale, float drop_p,
                          const uint64_t* seed, uint64_t offset, sbl_stream_t stream);
/* Grouped cross-attention forward, inference only (the beam search of the SBL decoder, sbl_pair_beam_tail): as
 * sbl_attention_seg_fwd with Lk_fixed >= 1 and no mask, but sequence b of the B reads the key / value rows of entry
 * b / kv_group - k / v hold B / kv_group entries of Lk_fixed rows, the W slots of a clip share the clip's hoisted K/V - and no
 * probabilities are written.  B must be a multiple of kv_group.  Per sequence the kernels, the size dispatch and the
 * arithmetic are those of sbl_attention_seg_fwd on K/V repeated kv_group-fold (bit-identical output); the dropout mask
 * index is the element's place in the probability layout of that call. */
int sbl_attention_seg_grouped_fwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* o,
                                  long ldo, int B, int H, const int* seg_L, int nseg, int Lk_fixed, int kv_group, float scale,
                                  float drop_p, const uint64_t* seed, uint64_t offset, sbl_stream_t stream);
/* Attention with a key count per entry, inference only (ragged clips: the padded frames behind a clip's end are no keys).
 * Lk_fixed >= 1: sbl_attention_seg_grouped_fwd, where kv_len is a DEVICE array of B / kv_group counts and sequence b sees key j
 * iff j < min(max(kv_len[b / kv_group], 0), Lk_fixed).  Lk_fixed == 0: self-attention of ONE segment (nseg == 1, kv_group == 1,
 * the encoder): kv_len has B counts and every query row of sequence b sees the keys j < kv_len[b] of its own rows, clamped the
 * same way; there is no causal mode.  A sequence without a visible key gets o = 0.  Key / value rows at or behind the count are
 * never loaded, so whatever they hold (NaN included) cannot reach o.  No probabilities are written and there is no backward.  The
 * dropout mask index of probability (i, j) is the one of the call without counts (the layout of Lk_fixed, or L, keys).  The
 * kernels are chosen from the host-known shapes as sbl_attention_seg_grouped_fwd chooses them (self-attention: by seg_L[0]);
 * kv_len is never read on the host, so a captured graph follows counts that are overwritten in place.  On the one-wavefront
 * kernels (L <= 16 and Lk <= 32; one segment of 17..32 rows) sequence b's output is bit-identical to that of
 * sbl_attention_seg_grouped_fwd on K/V cut to its count. */
int sbl_attention_seg_len_fwd(const float* q, long ldq, const float* k, long ldk, const float* v, long ldv, float* o,
                              long ldo, int B, int H, const int* seg_L, int nseg, int Lk_fixed, int kv_group,
                              const int32_t* kv_len, float scale, float drop_p, const uint64_t* seed, uint64_t offset,
                              sbl_stream_t stream);
/* Stage head of the SBL decoder for BOTH directions in one launch: out_d = dropout(emb[tok_d] + pe[:L]) for every segment
 * of the stage (SBL/transformer/decoder.py:116-120); mask = f(seed, offset_d, element index inside the stage's rows), the
 * indexing of sbl_dropout, which regenerates it in backward.  drop_p == 0: plain embedding + PE. */
int sbl_embed_pe_drop2_fwd(const int64_t* tok0, const int64_t* tok1, long ldt, const float* emb, const float* pe, float* out0,
                           float* out1, int B, const int* seg_L, int nseg, int D, int V, float drop_p, const uint64_t* seed,
                           uint64_t offset0, uint64_t offset1, sbl_stream_t stream);
/* Stage tail of the SBL decoder in one launch (SBL/transformer/decoder.py:160-186): the last cross-direction fusion at the
 * last position of every sequence (A'[L-1] = A[L-1] + B[0], B'[L-1] = 2 B[L-1] + A[0]) -> last_d (nseg*B, 512), the two
 * bias-free Linear(512, V) heads -> pred_d (nseg*B, ldp), and - write_tok != 0 - ys_d[b, step + 1] = argmax of the stage's
 * final segment (first maximal index).  yf_d: the last layer's outputs of the stage's rows; D must be 512, V <= 64. */
int sbl_decoder_tail_fwd(const float* yf0, const float* yf1, const float* w0, const float* w1, float* last0, float* last1,
                         float* pred0, float* pred1, long ldp, int64_t* ys0, int64_t* ys1, long ldy, int step, int write_tok,
                         int B, const int* seg_L, int nseg, int D, int V, sbl_stream_t stream);
int sbl_embed_pe_seg_fwd(const int64_t* tok, long ldt, const float* emb, const float* pe, float* out, int B,
                         const int* seg_L, int nseg, int D, int V, sbl_stream_t stream);
int sbl_embed_seg_bwd(const int64_t* tok, long ldt, const float* dy, float* demb, int B, const int* seg_L, int nseg, int D,
                      int V, sbl_stream_t stream);
int sbl_fusion_seg_fwd(const float* a, const float* b, float* a2, float* b2, int B, const int* seg_L, int nseg, int D,
                       sbl_stream_t stream);
int sbl_fusion_seg_bwd(const float* da2, const float* db2, float* da, float* db, int B, const int* seg_L, int nseg, int D,
                       sbl_stream_t stream);
/* out[s*B + b, :] = x[last row of sequence (s, b)]: the rows the output heads read (decoder.py:166-167);
 * bwd zero-fills dx (all rows) and scatters the nseg*B gradient rows back */
int sbl_gather_last_fwd(const float* x, float* out, int B, const int* seg_L, int nseg, int D, sbl_stream_t stream);
int sbl_gather_last_bwd(const float* dy, float* dx, int B, const int* seg_L, int nseg, int D, sbl_stream_t stream);

/* ---------------------------------------------------------------- last decoder layer on its "ends" rows
 * Of the last layer's output the step reads two rows per sequence: pred = prj(dec_output[:, -1]) after the last fusion
 * (SBL/transformer/decoder.py:160-167), i.e. A'[L-1] = A[L-1] + B[0] and B'[L-1] = 2 B[L-1] + A[0].  Everything of that layer
 * behind the self-attention core (attention.py:53-58 onwards, module.py:47-51) therefore runs on a compact batch: segment s
 * (prefix length L = seg_L[s]) holds B sequences of Lc = min(2, L) rows in (b, k) order, k = 0 -> position 0, k = Lc-1 ->
 * position L-1; compact row (s, b, k) stands for full row (sum_{t<s} B*seg_L[t]) + b*L + k*(L-1).  seg_L is always the list
 * of FULL prefix lengths.  Dropout decisions are those of the full-layout kernels for the same element. */
/* dst_t (compact rows, D) = the end rows of src_t (full rows, D) for up to four tensors in one launch (trailing ones NULL). */
int sbl_ends_gather4(const float* src0, const float* src1, const float* src2, const float* src3, float* dst0, float* dst1,
                     float* dst2, float* dst3, int B, const int* seg_L, int nseg, int D, sbl_stream_t stream);
/* dst_t (full rows, D) = src_t (compact rows) at the end rows and zero elsewhere (every row is written: no zero fill needed);
 * one or two tensors (src1 / dst1 NULL). */
int sbl_ends_scatter2(const float* src0, const float* src1, float* dst0, float* dst1, int B, const int* seg_L, int nseg, int D,
                      sbl_stream_t stream);
/* Adjoint of the stage tail's fusion (decoder.py:160-167) into the compact layout: dy_d(s, b, last) = kf_d * dlast_d[s*B + b]
 * (kf = 1 for l2r, 2 for r2l), dy_d(s, b, first) = dlast_{1-d}[s*B + b], the L = 1 row gets both; a NULL dlast is zero. */
int sbl_ends_tail_bwd(const float* dlast0, const float* dlast1, float* dy0, float* dy1, int B, const int* seg_L, int nseg, int D,
                      sbl_stream_t stream);
/* sbl_add_layernorm2_fwd / sbl_add_layernorm_bwd (module.py:50-51, attention.py:57-58) on the compact rows. */
int sbl_add_layernorm2_ends_fwd(const float* x0, const float* x1, const float* res0, const float* res1, const float* gamma0,
                                const float* gamma1, const float* beta0, const float* beta1, float* y0, float* y1, float* mean0,
                                float* mean1, float* rstd0, float* rstd1, int B, const int* seg_L, int nseg, int D, float eps,
                                float drop_p, const uint64_t* seed, uint64_t offset0, uint64_t offset1, sbl_stream_t stream);
int sbl_add_layernorm_ends_bwd(const float* dy, const float* x, const float* res, const float* gamma, const float* mean,
                               const float* rstd, float* dz, float* dx_drop, float* dgamma, float* dbeta, int B, const int* seg_L,
                               int nseg, int D, float drop_p, const uint64_t* seed, uint64_t offset, sbl_stream_t stream);
/* Cross-attention (attention.py:63-83 with the encoder's keys, Lk_fixed <= 32 rows per sequence) of the compact queries, both
 * directions in one launch / one direction's adjoint; p holds the compact (H*B, Lc, Lk) probability blocks back to back. */
int sbl_attention_ends2_fwd(const float* q0, const float* q1, long ldq, const float* k0, const float* k1, long ldk, const float* v0,
                            const float* v1, long ldv, float* o0, float* o1, long ldo, float* p_out0, float* p_out1, int B, int H,
                            const int* seg_L, int nseg, int Lk_fixed, float scale, float drop_p, const uint64_t* seed,
                            uint64_t offset0, uint64_t offset1, sbl_stream_t stream);
int sbl_attention_ends_bwd(const float* dout, long lddo, const float* q, long ldq, const float* k, long ldk, const float* v,
                           long ldv, const float* p, float* dq, long lddq, float* dk, long lddk, float* dv, long lddv, int B, int H,
                           const int* seg_L, int nseg, int Lk_fixed, float scale, float drop_p, const uint64_t* seed, uint64_t offset,
                           sbl_stream_t stream);

/* ---------------------------------------------------------------- SBL decoder pieces
 * Decoder.preprocess (decoder.py:62-77): strip IGNORE_ID, <sos> + ids (input form) / ids (label form), both padded with <eos>
   to maxlen; int64 (N,To) -> two int64 (N,maxlen).  padded1 != NULL: a second target set (the r2l direction) in the same launch. */
int sbl_decoder_preprocess(const int64_t* padded0, const int64_t* padded1, int64_t* ys_in0, int64_t* ys_out0, int64_t* ys_in1,
                           int64_t* ys_out1, int N, int To, int maxlen, int64_t sos, int64_t eos, int64_t ignore,
                           sbl_stream_t stream);
/* ys[b, step+1] = use_argmax ? argmax_c pred[b,c] : gold[b, step]: decoder.py:173-186.
 * use_argmax: host int, or if coins_dev != NULL coins_dev[step] (device int32, for graph replay). */
int sbl_argmax_select(const float* pred, long ldp, const int64_t* gold, long ldg, int64_t* ys, long ldy, int step,
                      int use_argmax, const int32_t* coins_dev, int B, int V, sbl_stream_t stream);

/* ---------------------------------------------------------------- label-smoothed cross entropy
 * SBL/transformer/loss.py:27-52.  out[0]=sum of row losses, out[1]=#valid rows, out[2]=#correct
 * (zeroed by the call).  bwd: dpred = gscale[0] / out[1] * (softmax - q) on valid rows. */
int sbl_smoothed_ce_fwd(const float* pred, const int64_t* gold, float* out3, int R, int C, float eps, int ignore_id,
                        sbl_stream_t stream);
int sbl_smoothed_ce_bwd(const float* pred, const int64_t* gold, const float* out3, const float* gscale, float* dpred,
                        int R, int C, float eps, int ignore_id, sbl_stream_t stream);

/* ---------------------------------------------------------------- validation scoring (WER / PER of greedy decodes)
 * SBL/train.py:251-276 with per_compute / wer_compute (:28-42), both directions of a batch in one launch, counters kept on
 * the device.  Per direction and sample, with ys the (Ly,) row of recognize (Ly = 17, column 0 is sos) and gold the (To,)
 * target row, To <= 15:
 *   g = the entries of gold not in {sos, eos, ignore}, in order; c = len(g)                              (train.py:252-253)
 *   p = the entries of ys[:c+1] not in {sos, eos, ignore}, in order (an eos is stripped where it stands)  (train.py:254)
 *   dist = Levenshtein distance of p and g over ids, unit costs (editdistance.eval); PER of the sample = dist / c
 *   word_err = 0 if p and g spell the same string, else 1 (the reference joins the names without a separator, so its
 *   wer_compute is 0 or 1 per sample).  names == NULL: the spelling of an id is the id.  Else names[id], id < n_names, is
 *   one 64-bit word: bits 56..58 the length L <= 7, the low L bytes the characters, first character most significant,
 *   all other bits 0 (the caller packs and checks it); a kept id outside [0, n_names) spells the empty string.
 * Deviations from the reference: (a) every sample counts once (train.py:262-263 extends the WER lists inside the sample
 * loop, so sample j of a batch of B enters the reference's WER mean B - j times); (b) a sample with c = 0 (a division by
 * zero there) is counted in n_empty and left out of every other counter; (c) rows n >= valid_rows[0] (device int32, NULL =
 * all N rows: the short last batch of a replayed graph) are ignored.
 * acc: uint64 (2, SBL_SCORE_COUNTERS), direction-major, ADDED to (the caller zeroes it once per epoch): n_scored, n_empty,
 * n_word_err, sum of dist, sum of c, then dist_by_len[16] and count_by_len[16] (sum of dist / number of scored samples per
 * gold length c).  mean(dist / c) = sum_c dist_by_len[c] / c / n_scored, formed in fp64 by the reader.  All state is
 * integer: the result does not depend on the order of the atomics and sums exactly across calls, replays and ranks.
 * per_sample: NULL, or int32 (2, 3, N) = per direction dist, c, word_err of every row (-1 on ignored rows).  N == 0 is a
 * successful no-op. */
#define SBL_SCORE_N_SCORED 0
#define SBL_SCORE_N_EMPTY 1
#define SBL_SCORE_N_WORD_ERR 2
#define SBL_SCORE_SUM_DIST 3
#define SBL_SCORE_SUM_LEN 4
#define SBL_SCORE_DIST_BY_LEN 5
#define SBL_SCORE_COUNT_BY_LEN 21
#define SBL_SCORE_COUNTERS 37
int sbl_seq_score(const int64_t* ys_l2r, const int64_t* ys_r2l, int Ly, const int64_t* gold_l2r, const int64_t* gold_r2l,
                  int To, int N, int64_t sos, int64_t eos, int64_t ignore, const uint64_t* names, int n_names,
                  const int32_t* valid_rows, int32_t* per_sample, uint64_t* acc, sbl_stream_t stream);
/* The same scoring for ONE direction: the single-direction seq2seq model, LRW/train.py:245-260 (predictions cut at
 * len(gold) + 1 and stripped of sos / eos / -1, :247-249).  ys (N, Ly) is the row of Seq2SeqTransformer.recognize, acc uint64
 * (SBL_SCORE_COUNTERS), per_sample NULL or int32 (3, N).  Same definition, deviations and counters as sbl_seq_score. */
int sbl_seq_score1(const int64_t* ys, int Ly, const int64_t* gold, int To, int N, int64_t sos, int64_t eos, int64_t ignore,
                   const uint64_t* names, int n_names, const int32_t* valid_rows, int32_t* per_sample, uint64_t* acc,
                   sbl_stream_t stream);

/* ---------------------------------------------------------------- single-direction seq2seq decoder (LRW/transformer/decoder.py)
 * out[b,l,:] = emb[tok[b*ldt + pos0 + l]] * scale + pe[pos0 + l], l < L: decoder.py:111-112 (teacher-forced, pos0 = 0, L = 14)
 * and :154-156 (greedy).  scale is x_logit_scale: d_model^-0.5 when the embedding is tied to the output projection, else 1. */
int sbl_embed_scale_pe_fwd(const int64_t* tok, long ldt, const float* emb, const float* pe, float* out, int B, int L, int D,
                           int V, float scale, int pos0, sbl_stream_t stream);
/* demb[tok[b*ldt + l]] += scale * dy[b,l,:] (float atomics; demb is accumulated into) */
int sbl_embed_scale_bwd(const int64_t* tok, long ldt, const float* dy, float* demb, int B, int L, int D, int V, float scale,
                        sbl_stream_t stream);
/* One greedy step of attention with a K/V cache: replaces the prefix recompute of decoder.py:146-164 (every step there runs
 * attention.py:32-60 over the whole prefix; the decoder is causal, so row i needs only the new query and the keys 0..i).
 * One wavefront per (clip, head), d = 64.  q (B, H*64) rows of stride ldq: the step's query.  k_cache / v_cache:
 * (B, Lcap, H*64) with row stride ldc and batch stride Lcap*ldc (independent of the current length), Lcap <= 64.
 * append = 1 (self-attention): the step's new rows k_new / v_new (B, H*64), stride ldn, are stored at cache row n_prev and the
 * query attends to rows 0..n_prev.  append = 0 (cross-attention over the hoisted encoder K/V): rows 0..n_prev-1, nothing is
 * written.  n_prev is the step index, a launch argument.  o (B, H*64), stride ldo = softmax(q K^T * scale) V, fp32. */
int sbl_decode_attn_step(const float* q, long ldq, const float* k_new, const float* v_new, long ldn, float* k_cache,
                         float* v_cache, long ldc, int Lcap, float* o, long ldo, int B, int H, int n_prev, int append,
                         float scale, sbl_stream_t stream);
/* Tail of a greedy step in one launch (decoder.py:166-171, then :154-156 of the next step): logits = y w^T (bias-free
 * Linear(512, V), V <= 64; plain fp32 FMA in every sbl_set_matmul_precision mode), ys[b, step+1] = arg-max (lowest index on
 * ties), and - x_next != NULL - x_next[b,:] = emb[that token] * emb_scale + pe[step+1], the next step's input row.  logits:
 * NULL or (B, V) with row stride ldl.  D must be 512; pe has pe_rows rows. */
int sbl_decode_tail(const float* y, long ldy, const float* w, float* logits, long ldl, int64_t* ys, long ldys, int step,
                    const float* emb, const float* pe, int pe_rows, float emb_scale, float* x_next, int B, int V, int D,
                    sbl_stream_t stream);

/* ---------------------------------------------------------------- beam search of the single-direction decoder
 * LRW1000/transformer/decoder.py:131-245, batched: clip n owns the W = beam_size slots n*W .. n*W + W-1 and every launch
 * runs all S = N * W slots; a slot without a live hypothesis carries the score -inf.  Ties, which the reference leaves to
 * torch.topk: the lower parent slot first, then the lower token id.  A candidate of score -inf is never kept.
 *
 * sbl_decode_attn_step for beam slots (replaces the per-hypothesis prefix recompute of LRW1000/transformer/decoder.py:170-184).
 * append = 1 (self-attention): anc (S, lda) int32 is the ancestry table - key j < n_prev of slot b is row j of cache slot
 * anc[b][j] (values are clamped to 0 .. S-1), for the score and the value pass; the new rows k_new / v_new are stored at row
 * n_prev of slot b's OWN cache and used from registers.  k_cache / v_cache: (S, Lcap, H*64).  No cache row is ever copied.
 * append = 0 (cross-attention): anc is unused (NULL); slot b reads rows 0 .. n_prev-1 of the hoisted cache of clip b / W, so
 * k_cache / v_cache hold S / W clips.  Strides, Lcap <= 64, scale and o as in sbl_decode_attn_step. */
int sbl_beam_attn_step(const float* q, long ldq, const float* k_new, const float* v_new, long ldn, float* k_cache,
                       float* v_cache, long ldc, int Lcap, const int32_t* anc, long lda, float* o, long ldo, int S, int W, int H,
                       int n_prev, int append, float scale, sbl_stream_t stream);
/* Tail of beam step `step` in one launch, one workgroup per clip (LRW1000/transformer/decoder.py:186-229): logits = y w^T
 * (fp32 FMA, V <= 64, 1 <= W <= min(16, V)); local = log_softmax(logits) + log_prior[last_tok[slot]] (log_prior: NULL or
 * (V, V) fp32, already logged, -inf allowed: decoder.py:163-166,191); candidates = score[slot] + local, fp32; the best W of
 * the clip's W * V candidates are kept in order.  At step maxlen-1 every kept hypothesis ends (decoder.py:213-218: an <eos> is
 * appended at no score, also behind an <eos>); before that the ones whose token is eos end (decoder.py:222-227).  Written:
 *   hist_tok / hist_par / hist_score / hist_flag (N, maxlen, W) at [n][step][rank]: token, parent rank at the previous step,
 *     accumulated score, flag (0 nothing kept, 1 live, 2 ended);
 *   end_score / end_ref (N, W*maxlen), end_count (N): the ended list in kept order, ref = step * W + rank (step 0 resets the
 *     count, so nothing has to be zeroed between calls);
 *   score / last_tok (S), in place: rank r moves to slot n*W + r; score = -inf unless live;
 *   anc_new (S, lda >= maxlen): anc_new[r][0..step-1] = anc_old[parent][0..step-1], anc_new[r][step] = the parent's slot
 *     (anc_old and anc_new must differ: the kernel reads the parents' rows);
 *   x_next (S, 512), when not NULL: emb[token] * emb_scale + pe[step+1], the next step's input rows. */
int sbl_beam_tail(const float* y, long ldy, const float* w, const float* log_prior, float* score, int32_t* last_tok,
                  const int32_t* anc_old, int32_t* anc_new, long lda, int32_t* hist_tok, int32_t* hist_par, float* hist_score,
                  int32_t* hist_flag, float* end_score, int32_t* end_ref, int32_t* end_count, int step, int maxlen, int eos,
                  const float* emb, const float* pe, int pe_rows, float emb_scale, float* x_next, int N, int W, int V, int D,
                  sbl_stream_t stream);
/* The nbest <= 16 best ended hypotheses of every clip, a stable descending sort by score (LRW1000/transformer/decoder.py:240-245;
 * no length normalisation), traced back through the history: yseq (N, nbest, maxlen+2) int64 = <sos>, the tokens, eos-filled
 * behind the end; lengths (N, nbest) int32 (maxlen+2 for a hypothesis that ended at the last step); scores (N, nbest) fp32;
 * n_hyps (N) int32 = min(ended, nbest).  Ranks beyond n_hyps: length 0, score -inf, an all-eos row. */
int sbl_beam_finish(const float* end_score, const int32_t* end_ref, const int32_t* end_count, const int32_t* hist_tok,
                    const int32_t* hist_par, int64_t* yseq, int32_t* lengths, float* scores, int32_t* n_hyps, int N, int W,
                    int maxlen, int nbest, int sos, int eos, sbl_stream_t stream);

/* ---------------------------------------------------------------- ragged clips in the single-direction decodes
 * Clip n of a padded batch decodes as the reference decodes it ALONE, cut to its first l_n frames: LRW/transformer/decoder.py
 * :138-176 (greedy, maxlen = encoder_outputs.size(1) = l_n there) and LRW1000/transformer/decoder.py:131-245 (beam search,
 * maxlen = l_n with decode_max_len == 0, :139-141; the forced end of :213-218 then comes at step l_n - 1).  All counts are
 * device arrays that no entry reads on the host, so a captured graph follows an array that is overwritten in place.
 *
 * sbl_decode_attn_step / sbl_beam_attn_step with a key count per K/V entry, cross-attention only (append must be 0):
 * kv_len holds B counts (decode) or S / W counts (beam, one per clip); row b sees key j iff
 * j < min(max(kv_len[clip], 0), n_prev).  Cache rows at or behind the count are never loaded, in the score pass and in the
 * value pass, so whatever they hold cannot reach o; a row without a visible key gets o = 0.  Row b's output is bit-identical
 * to the entry without counts called with n_prev = its count on the same K / V.  anc / lda of sbl_beam_attn_step_len are
 * kept for the argument list's sake and unused, as in sbl_beam_attn_step with append = 0 (pass NULL, 0).  Refused before
 * any launch: kv_len == NULL,
 * append != 0, and everything the entries without counts refuse. */
int sbl_decode_attn_step_len(const float* q, long ldq, const float* k_new, const float* v_new, long ldn, float* k_cache,
                             float* v_cache, long ldc, int Lcap, float* o, long ldo, int B, int H, int n_prev, int append,
                             float scale, const int32_t* kv_len, sbl_stream_t stream);
int sbl_beam_attn_step_len(const float* q, long ldq, const float* k_new, const float* v_new, long ldn, float* k_cache,
                           float* v_cache, long ldc, int Lcap, const int32_t* anc, long lda, float* o, long ldo, int S, int W,
                           int H, int n_prev, int append, float scale, const int32_t* kv_len, sbl_stream_t stream);
/* sbl_beam_tail with a last step per clip: clip_steps (N) int32; every kept hypothesis of clip n ends (with the appended
 * <eos> at no score) at step clamp(clip_steps[n], 1, maxlen) - 1 instead of maxlen - 1.  From the next step on the clip has no
 * live hypothesis: its slots carry -inf, nothing is kept, the history flags are 0 and the ended list stays as it is.  With
 * clip_steps[n] == maxlen for every clip all outputs equal sbl_beam_tail's bit for bit.  (The lexicon tail has no such form:
 * its step count is the longest word's.) */
int sbl_beam_tail_len(const float* y, long ldy, const float* w, const float* log_prior, float* score, int32_t* last_tok,
                      const int32_t* anc_old, int32_t* anc_new, long lda, int32_t* hist_tok, int32_t* hist_par,
                      float* hist_score, int32_t* hist_flag, float* end_score, int32_t* end_ref, int32_t* end_count, int step,
                      int maxlen, int eos, const float* emb, const float* pe, int pe_rows, float emb_scale, float* x_next, int N,
                      int W, int V, int D, const int32_t* clip_steps, sbl_stream_t stream);
/* sbl_beam_finish after sbl_beam_tail_len, with the same array: a hypothesis that ended at step s has length s + 3 when
 * s == clamp(clip_steps[n], 1, maxlen) - 1 (the appended <eos>) and s + 2 otherwise.  yseq keeps its maxlen + 2 columns. */
int sbl_beam_finish_len(const float* end_score, const int32_t* end_ref, const int32_t* end_count, const int32_t* hist_tok,
                        const int32_t* hist_par, int64_t* yseq, int32_t* lengths, float* scores, int32_t* n_hyps, int N, int W,
                        int maxlen, int nbest, int sos, int eos, const int32_t* clip_steps, sbl_stream_t stream);

/* ---------------------------------------------------------------- beam search of the bidirectional SBL decoder
 * The reference's recognize_beam (SBL/transformer/decoder.py:301-385) is greedy; this is the search its beam_size / nbest
 * arguments name.  A hypothesis is a PAIR of an l2r and an r2l prefix that are fused with each other as row b of the two
 * directions is in the greedy decode; clip n owns the W slots n*W .. n*W + W-1, a dead slot carries the total score -inf, and
 * nothing ends early (16 positions are always decoded, <eos> is fed and predicted behind the end).
 *
 * Tail of step `step` in one launch, one workgroup per clip: y_l / y_r (S = N*W, ldy) are the rows the two heads read,
 * w_l / w_r the (V, 512) bias-free heads (plain fp32 FMA in every sbl_set_matmul_precision mode; V <= 64, 1 <= W <= min(16, V)).
 * lpL / lpR = log_softmax of the logits.  Candidates of a live slot s: every (a, b) in V x V, total = score[s] + (lpL[s][a] +
 * lpR[s][b]) added in fp32 in that order, per-direction scores score_dir[s][0] + lpL[s][a] and score_dir[s][1] + lpR[s][b].  The
 * best W candidates of the clip are kept in descending total and the candidate of rank r moves to slot r.  Exact ties: the
 * lower parent slot, then the lower rank of a in its slot's l2r ordering (log-prob descending, token id ascending), then the
 * lower rank of b.  A candidate of total -inf is never kept; a rank without one gets the scores -inf, eos tokens and its own
 * rank as parent.  Written:
 *   score (S) and score_dir (S, 2), in place;
 *   ys_new_d[rank] = ys_old_d[parent][0 .. step] || token || eos ..., (S, ldys >= maxlen+1) int64 (ys_old and ys_new must
 *     differ: the kernel reads the parents' rows);
 *   hist_tok_l / hist_tok_r / hist_par / hist_score (N, maxlen, W) at [n][step][rank]: the two tokens, the parent's rank at
 *     the previous step, the total score. */
int sbl_pair_beam_tail(const float* y_l, const float* y_r, long ldy, const float* w_l, const float* w_r, float* score,
                       float* score_dir, const int64_t* ys_old_l, const int64_t* ys_old_r, int64_t* ys_new_l, int64_t* ys_new_r,
                       long ldys, int32_t* hist_tok_l, int32_t* hist_tok_r, int32_t* hist_par, float* hist_score, int step,
                       int maxlen, int eos, int N, int W, int V, int D, sbl_stream_t stream);

/* ---------------------------------------------------------------- closed-vocabulary word decode (lexicon shortlist, rescoring)
 * LRW and LRW1000 are closed-vocabulary word benchmarks.  The reference scores "the joined phoneme string equals the gold
 * string" (wer_compute, SBL/train.py:28-38, as the test loop uses it, SBL/test.py:185-218): a hypothesis one substitution away
 * from a vocabulary word is a miss.  These two launches replace that comparison and extend it: the hypotheses are mapped onto
 * the lexicon, and the model chooses between the close words.
 *
 * Lexicon: Wn >= 1 words; word w is a token row of length c_w in 1..15 with ids in [0, V), none equal to sos or eos;
 *   duplicate rows are distinct entries.  Packed as `lex` (Wn, 16) uint8: bytes 0..14 the tokens (0 behind the end), byte 15
 *   c_w; 16-byte aligned.  The caller validates the words when it packs them.
 * Hypothesis h < H of clip n: the rows ys_l2r[n*ld_n + h*ld_h ..] and ys_r2l[...] of Ly = 17 entries, as recognize and
 *   beam_search return them.  From each row: entries 1..16, cut before the first eos, without the entries equal to sos or
 *   ignore -> p_l and p_r, of length 0..16.
 * Distance: D(n, h, w) = lev(p_l, w) + lev(p_r, reversed(w)), unit costs, 0..32.
 * Shortlist: the key of word w for clip n is the lexicographic minimum over h of (D(n,h,w), h); the shortlist is the K words
 *   with the smallest (D, h, w), in that order, 1 <= K <= min(Wn, 16).  All integer: no float, no atomics.
 * Written: cand / cand_dist / cand_hyp (N, K) int32 = w, D, h per rank; the candidates' token tables cand_ys_l2r (N*K, 17)
 *   int64 = sos, w, eos fill and cand_ys_r2l = sos, reversed(w), eos fill; n_pos (N*K) int32 = c_w + 1, the trained positions
 *   (the tokens and the one eos that preprocess puts in ys_out).  N == 0 is a successful no-op. */
int sbl_lexicon_shortlist(const int64_t* ys_l2r, const int64_t* ys_r2l, long ld_n, long ld_h, int Ly, const uint8_t* lex, int Wn,
                          int N, int H, int K, int64_t sos, int64_t eos, int64_t ignore, int32_t* cand, int32_t* cand_dist,
                          int32_t* cand_hyp, int64_t* cand_ys_l2r, int64_t* cand_ys_r2l, int32_t* n_pos, sbl_stream_t stream);
/* Pair score of S slots in groups of G <= 16 (G = K after a shortlist, G = W when a beam is rescored), one workgroup per group.
 * y_l / y_r (16*S, ldy): row i*S + s is what the head reads at the last position of prefix length i+1 of slot s - the
 * segment-major rows of sbl_gather_last_fwd for the 16 segments of lengths 1..16.  w_l / w_r: the (V, 512) bias-free heads,
 * plain fp32 FMA in every sbl_set_matmul_precision mode, V <= 64: the arithmetic of sbl_pair_beam_tail.  ys_l2r / ys_r2l
 * (S, ldys >= 17) int64 token tables; n_pos (S) int32, clamped to 0..16, NULL = 16 everywhere.
 * With lpL_i / lpR_i the two heads' log-softmax at step i, taken at tokens ys_l2r[s][i+1] / ys_r2l[s][i+1] (-inf for a token
 * outside [0, V)):  logp (S, 16, 2) = (lpL_i, lpR_i) for i < n_pos[s], else 0;  score_dir (S, 2) = their sums in ascending i,
 * fp32;  score (S): starts at 0, then score += (lpL_i + lpR_i) in ascending i - the order of sbl_pair_beam_tail, so with
 * n_pos = 16 it is the beam search's total.  No length penalty, no prior.  best (S/G) int32: the rank in the group with the
 * largest score, the lower rank on an exact tie.  S == 0 is a successful no-op. */
int sbl_pair_score_tail(const float* y_l, const float* y_r, long ldy, const float* w_l, const float* w_r, const int64_t* ys_l2r,
                        const int64_t* ys_r2l, long ldys, const int32_t* n_pos, float* logp, float* score_dir, float* score,
                        int32_t* best, int S, int G, int V, int D, sbl_stream_t stream);

/* ---------------------------------------------------------------- lexicon-constrained beam search (single-direction decoder)
 * Every layer of the single-direction decoder is causal, so ONE KV-cached beam search restricted to the prefixes of the word
 * list ranks the lexicon by the model's own score: every hypothesis is a word, the n-best are distinct words, and the search
 * runs Cmax + 1 steps (Cmax = the longest word, <= 15) instead of Ti.
 *
 * Trie of a lexicon (above): node 0 is the empty prefix and there is one node per distinct non-empty prefix of any word,
 *   numbered breadth-first with siblings in ascending token id, so the children of a node are consecutive;
 *   P <= 1 + sum of c_w nodes.  Three tables of P entries:
 *   mask int64: bit v is set iff prefix(p) + [v] is a node; bit eos is set iff prefix(p) is a word (words hold neither sos nor
 *     eos, so the eos bit is unambiguous);
 *   first int32: the node of the lowest-token child;  child(p, v) = first[p] + popcount(mask[p] & ~bit(eos) & (bit(v) - 1)),
 *     clamped to 0 .. P-1;
 *   word int32: the lowest word index whose tokens are prefix(p), or -1 if there is none (duplicate rows of the lexicon share
 *     a node; the lowest index answers for them).
 * Constrained search: the search of sbl_beam_tail word for word - the same candidate arithmetic in fp32, tie order, history,
 *   ended list and ancestry rows - except that every slot carries a node q (the root at the start), candidate (slot, v)
 *   exists only where bit v of mask[q] is set, and the kept rank's node is child(q_parent, v) for v != eos and q_parent for
 *   v == eos (0 at a rank where nothing is kept).  The candidate's value is score + log_softmax(logits)[v]
 *   (+ log_prior[last_tok][v]); the log-softmax runs over all V classes and is NOT renormalised over the allowed ones, so an
 *   ended hypothesis carries log P(w, eos | clip) of the teacher-forced model (plus priors).  The last-step rule of
 *   sbl_beam_tail is untouched: the host sets maxlen = Cmax + 1, and with a real lexicon only eos candidates exist there.
 *   Node values read from memory are clamped to 0 .. P-1, as anc is: a bad table never reads out of bounds.
 *
 * sbl_beam_tail with the constraint: the arguments of sbl_beam_tail, then trie_mask / trie_first (P) and node (S) int32,
 * updated in place like last_tok.  With the one-node table P = 1, mask = all V bits, first = 0 it equals sbl_beam_tail bit
 * for bit in every output.  One 8-byte mask load per slot, a bit test per lane, a popcount for the child. */
int sbl_beam_tail_lex(const float* y, long ldy, const float* w, const float* log_prior, float* score, int32_t* last_tok,
                      const int32_t* anc_old, int32_t* anc_new, long lda, int32_t* hist_tok, int32_t* hist_par, float* hist_score,
                      int32_t* hist_flag, float* end_score, int32_t* end_ref, int32_t* end_count, int step, int maxlen, int eos,
                      const float* emb, const float* pe, int pe_rows, float emb_scale, float* x_next, int N, int W, int V, int D,
                      const int64_t* trie_mask, const int32_t* trie_first, int P, int32_t* node, sbl_stream_t stream);
/* Exact lookup of R token rows in the trie, one thread per row.  ys (R, ldys >= Ly) int64; from each row, by the hypothesis
 * rule of sbl_lexicon_shortlist: entries 1 .. Ly-1, cut before the first eos, without the entries equal to sos or ignore.
 * The tokens are walked from the root.  node (R) int32 = the node reached, -1 if a token has no child (or is outside 0..63);
 * word (R) int32 = trie_word[node], -1 if the walk failed or the end node is not a word (an empty row: -1).  It gives the
 * n-best of the constrained search their word indices and greedy rows an exact-match lookup.  R == 0 is a successful no-op. */
int sbl_lexicon_lookup(const int64_t* ys, long ldys, int Ly, int R, const int64_t* trie_mask, const int32_t* trie_first,
                       const int32_t* trie_word, int P, int64_t sos, int64_t eos, int64_t ignore, int32_t* word, int32_t* node,
                       sbl_stream_t stream);

/* ---------------------------------------------------------------- lexicon-constrained pair beam search (SBL decoder)
 * The same constraint for the pair search of sbl_pair_beam_tail, through ONE trie over PAIRS of tokens: a hypothesis pair is
 * one lexicon word w, its l2r row spelling w and its r2l row reversed(w).  The n-best are distinct words, a word's total is
 * the sum sbl_pair_score_tail forms over its c_w + 1 trained positions, and the search runs Cmax + 1 steps.
 *
 * Pair trie of a lexicon: a state is what both directions have emitted after t steps of one word of c tokens,
 *   (w[:t], w[c-t:]) - the prefix, and the suffix that the r2l row has spelled backwards.  Node 0 is the empty state; one node
 *   per distinct state of any word at any depth 0..c_w (words of different length share equal states); one TERMINAL node per
 *   distinct word, the child of its depth-c_w state under the key (eos, eos).  The key of an edge is a * 64 + b < 4096, a the
 *   l2r and b the r2l token of the step: (w[t], w[c-1-t]) for t < c, (eos, eos) at t = c.  Nodes are numbered breadth-first
 *   with the children of a node in ascending key, so the child reached through CSR entry e is node e + 1.
 *   P <= 2 + sum of (c_w + 1) nodes, E = P - 1 edges.  Three int32 tables:
 *   begin (P + 1): CSR offsets into key; a terminal node has an empty range;
 *   key (E): the edge keys, ascending inside a node;
 *   word (P): at a terminal node the lowest word index that spells it (duplicate rows share a node), -1 elsewhere.
 *
 * Tail of step `step`: the arguments, launch shape, logits and per-row log-softmax of sbl_pair_beam_tail (one body), then the
 * tables, node_old / node_new (S) int32 - double-buffered like the prefixes, a rank reads its parent's node; the search starts
 * with every node 0 - and hist_node (N, maxlen, W).  Candidates of a live slot s at node q = node_old[s]:
 *   word[q] >= 0 (the pair has ended): exactly one, tokens (eos, eos), total score[s] and score_dir[s] UNCHANGED (no add: the
 *     values are carried bit for bit), node q;
 *   otherwise one per entry e in begin[q] .. begin[q+1], a = key[e] >> 6, b = key[e] & 63: total = score[s] + (lpL[s][a] +
 *     lpR[s][b]) added in fp32 in that order, score_dir[s][0] + lpL[s][a] and score_dir[s][1] + lpR[s][b], node e + 1.
 *   The log-softmax runs over all V classes and is NOT renormalised over the allowed tokens.
 * The clip's best W candidates are kept in descending total; exact ties go to the lower slot, then the lower entry e (the
 * lower key) - simpler than the rank order of sbl_pair_beam_tail, whose candidates are a product of two sorted lists.  A
 * candidate of total -inf or NaN is never kept; a rank without a candidate gets the scores -inf, eos tokens, its own rank as
 * parent and node 0.  Any candidate count is handled (the root may have min(Wn, V*V) children).
 * A bad table never reads out of bounds: nodes read from memory are clamped to 0 .. P-1, begin values to 0 .. E (an empty or
 * inverted range: no candidates), a key with a token >= V is a -inf candidate, and the node written is min(e + 1, P - 1).
 * Written: score, score_dir, ys_new_* and the four histories as sbl_pair_beam_tail writes them, hist_node, node_new. */
int sbl_pair_beam_tail_lex(const float* y_l, const float* y_r, long ldy, const float* w_l, const float* w_r, float* score,
                           float* score_dir, const int64_t* ys_old_l, const int64_t* ys_old_r, int64_t* ys_new_l,
                           int64_t* ys_new_r, long ldys, int32_t* hist_tok_l, int32_t* hist_tok_r, int32_t* hist_par,
                           float* hist_score, int step, int maxlen, int eos, int N, int W, int V, int D, const int32_t* trie_begin,
                           const int32_t* trie_key, const int32_t* trie_word, int P, int E, const int32_t* node_old,
                           int32_t* node_new, int32_t* hist_node, sbl_stream_t stream);

/* ---------------------------------------------------------------- stage-1 classification heads (CLS pre-training)
 * CLS/transformer/transformer.py:31-35 as oracle.sbl_oracle.cls_forward restates it (the shipped forward's mean(dim=2)
 * raises): enc (N,T,D) row-major, D = 512; fc_1500 = W1 (C1,D) + b1, fc_2 = W2 (C2,D) + b2, C2 <= 16.
 * Plain fp32 FMA in every sbl_set_matmul_precision mode; deterministic (no atomics, every sum in a fixed order).
 * fwd (2 launches): pooled (N,D) = mean over t of enc (kept for bwd), pooled_t (D,N) scratch, logits1 (N,C1) =
 * pooled W1^T + b1, logits2 (N,C2) = enc[:, lang_index] W2^T + b2 (the reference reads row 30 of its 31-frame clips). */
int sbl_cls_head_fwd(const float* enc, const float* w1, const float* b1, const float* w2, const float* b2, float* pooled,
                     float* pooled_t, float* logits1, float* logits2, int N, int T, int D, int C1, int C2, int lang_index,
                     sbl_stream_t stream);
/* loss = CE(logits1, tgt1) + lang_weight * CE(logits2, tgt2): CLS/train.py:127-130 (nn.CrossEntropyLoss, each a mean over the
 * rows whose target != ignore_id).  stats6 = {loss sum, valid rows, correct} of head 1, then of head 2 (argmax ties go to the
 * lowest index; CLS/train.py:115-121).  One launch, written by the call (nothing to zero).  bwd (one launch): dlogits =
 * gscale[0] / valid * (softmax - onehot) for head 1, times lang_weight for head 2, 0 on ignored rows. */
int sbl_cls_loss_fwd(const float* logits1, const float* logits2, const int64_t* tgt1, const int64_t* tgt2, int N, int C1,
                     int C2, float lang_weight, int ignore_id, float* loss, float* stats6, sbl_stream_t stream);
int sbl_cls_loss_bwd(const float* logits1, const float* logits2, const int64_t* tgt1, const int64_t* tgt2, const float* stats6,
                     const float* gscale, float* dlogits1, float* dlogits2, int N, int C1, int C2, float lang_weight,
                     int ignore_id, sbl_stream_t stream);
/* head bwd (one launch): dW1 = dlogits1^T pooled, db1 = sum_n dlogits1, dW2 = dlogits2^T enc[:, lang_index], db2 = sum_n
 * dlogits2; d_enc[n,t] = dlogits1[n] W1 / T, + dlogits2[n] W2 on t == lang_index.  accumulate = 1: the four parameter
 * gradients are added to (persistent flat gradient buffers); d_enc is always written.  Any of the five outputs may be NULL
 * (not computed). */
int sbl_cls_head_bwd(const float* enc, const float* pooled, const float* dlogits1, const float* dlogits2, const float* w1,
                     const float* w2, float* d_enc, float* dw1, float* db1, float* dw2, float* db2, int N, int T, int D,
                     int C1, int C2, int lang_index, int accumulate, sbl_stream_t stream);

/* ---------------------------------------------------------------- device input pipeline
 * uint8 grayscale frames (N,Tin,Hin,Win) -> fp32 clips (N,Tout,Hc,Wc): out = lut256[in[n, src_frame[n,t], y1[n]+y,
 * x1[n] + (flip[n] ? Wc-1-x : x)]], zero where src_frame < 0.  lut256[v] = float32((v/255. - mean)/std) computed in
 * double by the caller: bit-identical to SBL/data_gen.py:122-125 + cvtransforms.py:44-48 (ColorNormalize), :22-33 /
 * :7-19 (Random/CenterCrop), :36-41 (HorizontalFlip), data_gen.py:104-108 (FrameRemoval as a source-frame map) and
 * :290-296 (zero padding to 30 frames).  y1/x1/flip: device int32[N]; src_frame: device int32[N*Tout]. */
int sbl_preprocess_clips(const uint8_t* in, float* out, const float* lut256, const int* y1, const int* x1, const int* flip,
                         const int* src_frame, int N, int Tin, int Hin, int Win, int Tout, int Hc, int Wc,
                         sbl_stream_t stream);

/* ---------------------------------------------------------------- fused Adam
 * torch.optim.Adam(betas=(0.9,0.98), eps=1e-9) over a flat fp32 buffer, grad pre-scaled by
 * grad_scale (1/world_size): SBL/train.py:75, SBL/transformer/optimizer.py:18-27. */
int sbl_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                  int step, float grad_scale, sbl_stream_t stream);

/* ---------------------------------------------------------------- device-side optimizer step
 * Global-norm / element clip, non-finite skip, Noam schedule and Adam with every per-step scalar in DEVICE memory, so
 * that zero_grad + forward + backward + update replay as one hipGraph (sbl_adam_step takes lr and step from the host).
 * The optimizer state is a caller-owned, 8-byte aligned double[SBL_OPT_STATE_SLOTS]; doubles hold the counters exactly:
 *   [SBL_OPT_STEP]          t, the number of APPLIED steps (Adam's bias-correction exponent, the Noam step)
 *   [SBL_OPT_SKIPPED]       number of skipped steps
 *   [SBL_OPT_GRAD_NORM]     L2 norm of the last clamped, scaled gradient (inf / NaN when it held a non-finite element)
 *   [SBL_OPT_CLIP_COEF]     last global-norm clip coefficient, min(1, max_norm / (norm + 1e-6)); 1 when max_norm <= 0
 *   [SBL_OPT_LR]            current rate: written by sbl_opt_finalize under a Noam schedule, else by the host
 *   [SBL_OPT_STEP_SIZE]     lr / (1 - beta1^t)
 *   [SBL_OPT_INV_SQRT_BC2]  1 / sqrt(1 - beta2^t)
 *   [SBL_OPT_SKIP]          1 when the last sbl_opt_finalize decided to skip the update, else 0
 * One step = sbl_grad_sumsq per trainable range (increasing workspace offsets), one sbl_opt_finalize, sbl_adam_step_dev
 * per range, all on one stream.  A launch of n elements uses min(SBL_OPT_MAX_BLOCKS, ceil(ceil(n / 4)
 * / 256)) blocks (one partial sum each).  No float or double atomics anywhere: every sum is taken in an order that is a
 * function of (n, number of partials) alone, so two runs give the same bits and data-parallel replicas that hold the same
 * summed gradient derive the same coefficient. */
#define SBL_OPT_STATE_SLOTS 8
#define SBL_OPT_STEP 0
#define SBL_OPT_SKIPPED 1
#define SBL_OPT_GRAD_NORM 2
#define SBL_OPT_CLIP_COEF 3
#define SBL_OPT_LR 4
#define SBL_OPT_STEP_SIZE 5
#define SBL_OPT_INV_SQRT_BC2 6
#define SBL_OPT_SKIP 7
#define SBL_OPT_MAX_BLOCKS 2048
/* partials[offset + b] = sum over block b's elements of clamp(g[i] * grad_scale, +-clip_value)^2, accumulated in double.
 * The clamp is torch.clamp's (SBL/utils.py:10-19 clip_gradient): NaN stays NaN, +-inf becomes +-clip_value; clip_value
 * <= 0: off.  Any n >= 1; 16-byte loads when g is 16-byte aligned.  capacity: doubles in `partials`. */
int sbl_grad_sumsq(const float* g, long n, float grad_scale, float clip_value, double* partials, long capacity, long offset,
                   sbl_stream_t stream);
/* One block: sum = partials[0 .. nparts) in a fixed order, norm = sqrt(sum), coef as above (the rule of
 * torch.nn.utils.clip_grad_norm_; max_norm <= 0: off).  If sum is finite, or skip_nonfinite == 0: t += 1, with noam_k > 0
 * lr = noam_k * 512^-0.5 * min(t^-0.5, t * noam_warmup^-1.5) (SBL/transformer/optimizer.py:18-27), else lr is the slot as
 * the host left it, and both bias-correction slots are recomputed from t; the skip flag is cleared.  Otherwise the skip
 * flag is set, the skipped counter goes +1, and t, lr and the correction slots are untouched.  The sum of squares of
 * finite floats cannot overflow a double, so a non-finite sum means exactly "some clamped element was inf or NaN". */
int sbl_opt_finalize(double* state, const double* partials, long nparts, double max_norm, int skip_nonfinite, double noam_k,
                     double noam_warmup, float beta1, float beta2, sbl_stream_t stream);
/* Adam over one range with g' = clamp(g * grad_scale, +-clip_value) * state[SBL_OPT_CLIP_COEF], the step size and second
 * bias factor from the state buffer, and sbl_adam_step's arithmetic otherwise.  With state[SBL_OPT_SKIP] set nothing is
 * written: p, m, v keep their bits. */
int sbl_adam_step_dev(float* p, const float* g, float* m, float* v, long n, const double* state, float beta1, float beta2,
                      float eps, float grad_scale, float clip_value, sbl_stream_t stream);
/* sbl_adam_step_dev with an exponential moving average of the weights in the same launch: p, m, v are updated by that
 * kernel's arithmetic (bit-identical to it), then e += w * (p_new - e) in fp32 (the difference rounded, product and sum one
 * fused multiply-add) with w = (float)(1 - d_t) and d_t in double from t = state[SBL_OPT_STEP], the count AFTER
 * sbl_opt_finalize's increment: d_t = min(ema_decay, (1 + t) / (10 + t)) when ema_warmup != 0, else ema_decay.  Every
 * thread derives w itself: no extra launch, no state slot.  Order in a step: sbl_grad_sumsq, sbl_opt_finalize, then this
 * in place of sbl_adam_step_dev.  With state[SBL_OPT_SKIP] set nothing is written: p, m, v, e keep their bits.  ema_decay
 * must lie in (0, 1); 16-byte accesses when all five buffers are 16-byte aligned. */
int sbl_adam_ema_step_dev(float* p, const float* g, float* m, float* v, float* e, long n, const double* state, float beta1,
                          float beta2, float eps, float grad_scale, float clip_value, double ema_decay, int ema_warmup,
                          sbl_stream_t stream);
/* a[i] <-> b[i] for i in [0, n), in place and exact (each element is read from both buffers and written to both by one
 * thread); the launch geometry of the kernels above.  The two ranges must not overlap.  It reads no state: the caller
 * decides when an exchange is due (FusedAdam.swap_ema: live weights <-> their average, then the weight re-pack). */
int sbl_swap_f32(float* a, float* b, long n, sbl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif

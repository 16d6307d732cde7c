/* convasr_hip.h -- C ABI of libconvasr_hip.so: the MI355X (gfx950) implementation of convasr's one hot path.
 *
 * The reference (vadimkantorov/convasr) has no FFI on this path: its boundary is the Python nn.Module surface of
 * models.py, whose arithmetic is delegated to torch.nn.functional (ATen/cuDNN/cuFFT).  Each entry point below names
 * the reference call site(s) (file:line in /root/reference) whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory; nothing here allocates, frees or synchronises;
 *   - every function enqueues on `stream` (a hipStream_t passed as void*) and returns 0, or a negative
 *     CONVASR_E* code with a message retrievable through convasr_last_error() (thread-local);
 *   - activations are "channels-last": element (b, c, t) of a logical (B, C, T) tensor lives at
 *     ((b * T + t) * C + c); dtype is CONVASR_F32, CONVASR_BF16 or CONVASR_F16 (the two 16-bit storage types run the same
 *     kernels, instantiated on v_mfma_*_bf16 / v_mfma_*_f16; every sum is accumulated in fp32).  convasr_convert_layout() moves data between
 *     this layout and arbitrary (B, C, T) strides (e.g. torch-contiguous NCW);
 *   - conv weights are consumed in a packed layout [tap][cout_pad][cin] produced by convasr_pack_conv_weight()
 *     from the reference's (Cout, Cin, K) fp32 parameters;
 *   - lengths are passed the way the reference passes them: `xlen` = fraction of the time axis per utterance
 *     (float, models.py:611-614); valid frames of a T-long axis are t < ceil(xlen[b] * T).
 */
#ifndef CONVASR_HIP_H
#define CONVASR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CONVASR_ABI_VERSION 11

enum { CONVASR_F32 = 0, CONVASR_BF16 = 1, CONVASR_I16 = 2, CONVASR_F16 = 3 };
enum { CONVASR_ACT_NONE = 0, CONVASR_ACT_RELU = 1, CONVASR_ACT_HARDTANH = 2, CONVASR_ACT_LEAKY_RELU = 3 };
enum { CONVASR_OK = 0, CONVASR_EINVAL = -1, CONVASR_ELAUNCH = -2, CONVASR_EUNSUPPORTED = -3 };

int convasr_abi_version(void);
const char* convasr_last_error(void);

/* ---- layout / dtype plumbing -------------------------------------------------------------------------------- */

/* dst[b,c,t] = (dst_dtype) src[b,c,t] for arbitrary element strides on both sides. */
int convasr_convert_layout(const void* src, int src_dtype, int64_t src_sb, int64_t src_sc, int64_t src_st,
                           void* dst, int dst_dtype, int64_t dst_sb, int64_t dst_sc, int64_t dst_st,
                           int B, int C, int T, void* stream);

/* ---- frontend: models.py:565-597 (LogFilterBankFrontend.forward), models.py:684-686 (normalize_signal) -------- */

/* absmax[b] = max_t |signal[b,t]|  (models.py:685).  signal dtype F32 or I16. */
int convasr_signal_absmax(const void* signal, int signal_dtype, int B, int T, float* absmax, void* stream);

/* Fused normalise -> pre-emphasis -> mask -> reflect/zero pad -> STFT(nfft, hop, window centred in nfft) -> power ->
 * mel (nmel x (nfft/2+1), + bias) -> log.  out is channels-last (B, F, nmel) fp32 with F = 1 + T / hop.
 * absmax may be NULL (normalize_signal=False); xlen may be NULL (no mask).  nfft = 128, 256, 512 or 1024 (models.py:516: the power
 * of two above the window -- 512 at 16 kHz x 0.02 s, 256 at train.py's default 8 kHz x 0.02 s), win_length <= nfft, nmel <= 128 (one or two channels per lane);
 * anything else returns CONVASR_EUNSUPPORTED. */
int convasr_logmel_fwd(const void* signal, int signal_dtype, const float* absmax, const float* xlen,
                       const float* window, int win_length, const float* mel_weight, const float* mel_bias,
                       float* out, int B, int T, int nfft, int hop, int nmel, float preemphasis, void* stream);

/* ---- MaskedInstanceNorm1d.forward: models.py:694-719 ---------------------------------------------------------- */

/* x: (B, C, T), y: (B, C, T_out >= T) with the given element strides; frames T .. T_out - 1 of y are written as zeros (the even-length
 * input the stride-2 fold below wants).  xlen NULL -> legacy un-masked branch (models.py:704-710). */
int convasr_instnorm_fwd(const void* x, int x_dtype, int64_t x_sb, int64_t x_sc, int64_t x_st,
                         void* y, int y_dtype, int64_t y_sb, int64_t y_sc, int64_t y_st,
                         const float* xlen, int B, int C, int T, int T_out, float eps, void* stream);

/* nn.InstanceNorm1d(track_running_stats = True).forward as MaskedInstanceNorm1d reaches it (models.py:711, JasperNetSmallTrainableInstanceNorm
 * 1394-1404; un-masked, no affine).  training != 0: y = (x - mean) / sqrt(biased var + eps) per (utterance, channel), and
 * running = (1 - momentum) running + momentum * batch mean of the instance means / UNBIASED variances (num_batches_tracked += 1 when given:
 * torch's InstanceNorm never counts, so the host mirror passes NULL);
 * stats_workspace: 2 B C floats.  training == 0: y = (x - running_mean) / sqrt(running_var + eps), nothing written back. */
int convasr_instnorm_running_fwd(const void* x, int x_dtype, int64_t x_sb, int64_t x_sc, int64_t x_st,
                                 void* y, int y_dtype, int64_t y_sb, int64_t y_sc, int64_t y_st,
                                 int B, int C, int T, int T_out, float eps, float* running_mean, float* running_var,
                                 int64_t* num_batches_tracked, float momentum, int training, float* stats_workspace, void* stream);

/* ---- compute_output_lengths: models.py:611-614 ------------------------------------------------------------------ */

/* out[b] = ceil(xlen[b] * T) in fp32 arithmetic, as (lengths_fraction * T).ceil().long() evaluates it (xlen NULL: T). */
int convasr_output_lengths(const float* xlen, int B, int T, int64_t* out, void* stream);

/* ---- Conv1d: models.py:47-77 (ConvSamePadding -> nn.Conv1d), models.py:23-44 (Decoder 1x1) --------------------- */

/* cout_pad(cout): rows of the packed weight (multiple of the kernel's N tile). */
int convasr_conv_cout_pad(int cout);

/* Memory layout of an fp32 conv parameter / its gradient, logical shape (Cout, Cin, K):
 *   CONVASR_W_REFERENCE  element (co, ci, k) at (co*Cin + ci)*K + k  -- torch-contiguous, what the reference's state dict holds;
 *   CONVASR_W_KMAJOR     element (co, ci, k) at (k*Cout + co)*Cin + ci -- tap-major, the element order of the packed compute
 *                        copies and of the weight-gradient slabs: the layout the MI355X training arena keeps masters and
 *                        gradients in (a torch view of shape (Cout, Cin, K) with strides (Cin, 1, Cout*Cin)), so that the packed
 *                        forward weights are a cast of the master and the split-K combine is a streaming sum. */
#define CONVASR_W_REFERENCE 0
#define CONVASR_W_KMAJOR 1

/* (Cout, Cin, K) fp32 parameter (in layout w_layout) -> packed compute-dtype copies:
 *   packed_fwd  [K][cout_pad(Cout)][Cin]  : packed_fwd[k][co][ci]   = w[co][ci][k]        (required)
 *   packed_dgrad[K][cout_pad(Cin)][Cout]  : packed_dgrad[k][ci][co] = w[co][ci][K-1-k]    (optional; input gradient = conv
 *                                           with flipped taps; derived from packed_fwd by a tiled transpose)
 * Only rows < Cout (resp. < Cin) are written: the caller zero-fills the buffers once so the padded rows read as zeros.
 * w == NULL: packed_fwd is already current (e.g. written by convasr_sgd_step's bf16 mirror) and only packed_dgrad is rebuilt. */
int convasr_pack_conv_weight(const float* w, void* packed_fwd, void* packed_dgrad, int dtype, int Cout, int Cin, int K, int w_layout, void* stream);

/* y[b,t,co] = epilogue( sum_{k,ci} x[b, t*stride + k*dil - pad, ci] * wp[k][co][ci] ), zero outside [0, Tin).
 * epilogue: acc -> (+ bias[co] if bias) -> (stats of that value over the tile's valid (b,t) if stats) -> (* scale[co] + shift[co]
 * if scale) -> activation -> (zero frames t >= ceil(xlen[b]*Tout) if xlen) -> store as y_dtype.
 * stats (may be NULL): per-m-tile partial sums, [rows][2][Cout] doubles (sum then sum of squares), rows written = *stats_rows
 * (<= convasr_conv_stats_max_rows(B, Tout), the size to allocate).  No atomics: convasr_bn_finalize / convasr_reduce_rows add the
 * rows in a fixed order, so batch statistics are bit-identical from run to run.
 * Used for forward (mode FWD weights) and for dgrad (mode DGRAD weights, stride must be 1, pad' = dil*(K-1) - pad).
 * Tout is at most (Tin + 2 pad - dil (K-1) - 1) / stride + 1 (F.conv1d's output length); a smaller Tout computes the first Tout frames only. */
int convasr_conv1d_fwd(const void* x, const void* wp, void* y, int x_dtype, int y_dtype,
                       int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int dil, int pad,
                       const float* bias, double* stats, const float* scale, const float* shift,
                       int act, float act_lo, float act_hi, const float* xlen, int* stats_rows, void* stream);
int convasr_conv_stats_max_rows(int B, int Tout);

/* Which kernel convasr_conv1d_fwd would launch for this geometry and these optional operands (has_* / act: what conv1d_fwd would be given)
 * under the current convasr_debug_set_conv_v2 state: 0 = the call would be refused (out[0] = the error code, convasr_last_error() the
 * message), 1 = the register-staged kernel, 2 = the LDS-DMA kernel, 3 = the one-tap kernel.  out[CONVASR_CONV_ROUTE_INTS] = error code,
 * B and Tout as the kernel is given them (a one-tap batch may be flattened to 1 x B T), tile rows, m tiles per utterance (one-tap: m
 * tiles), n tiles, total tiles, full tiles, narrow parts and tail128 (LDS-DMA only: tiles from `full tiles` on run as 2 or 4 column
 * pieces; 1 = the last m tile of an utterance is a 128-row tile, 2 = every tile is), x_rows, XI and ALIGNED_X (register-staged only),
 * LDS stages (one-tap only), dynamic LDS bytes, partial statistics rows.  It is the decision code of the launch itself, not a copy;
 * it launches nothing and needs no GPU: the tests ask it which shapes reach which instantiation. */
#define CONVASR_CONV_ROUTE_INTS 16
int convasr_conv1d_fwd_route(int x_dtype, int y_dtype, int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int dil, int pad,
                             int has_scale_shift, int act, int has_xlen, int has_stats, int* out);

/* Split-K form of convasr_conv1d_fwd for launches of a few tiles -- online inference, transcribe.py:140 / benchmark_online.py:125 (B = 1 x 6 s is
 * 4-16 workgroups per layer on 256 CUs, each reducing all of Cin x K alone): the reduction is cut over the 64-channel input blocks, workgroup
 * (tile, split) stores an fp32 partial tile into `workspace`, a second streaming kernel adds the partials in split order (deterministic) and
 * runs the same epilogue (bias, scale / shift, activation, length mask, rounding to y_dtype).  stride 1, no statistics; 16-bit input (the LDS-DMA
 * kernel, 64-channel blocks) or fp32 in and out (the exact-fp32 kernel, 32-channel slabs; the partials are added in fp64).
 *   convasr_conv1d_fwd_splitk_plan: the number of splits for this geometry (1: not worth it -- from a quarter of the CUs' worth of tiles up -- or
 *     outside the envelope: call convasr_conv1d_fwd) and the workspace bytes (splits x B x Tout x Cout fp32);
 *   convasr_conv1d_fwd_splitk: `splits` must be the plan's answer (>= 2).  The plan does not see the dilation: a 16-bit geometry whose halo
 *     the LDS-DMA kernel cannot hold at 256-row tiles ((K - 1) dil > 64) runs as the unsplit convasr_conv1d_fwd, same epilogue. */
int convasr_conv1d_fwd_splitk_plan(int x_dtype, int B, int Cin, int Cout, int Tout, int K, int64_t* workspace_bytes);
int convasr_conv1d_fwd_splitk(const void* x, const void* wp, void* y, int x_dtype, int y_dtype,
                              int B, int Cin, int Cout, int Tin, int Tout, int K, int dil, int pad,
                              const float* bias, const float* scale, const float* shift, int act, float act_lo, float act_hi,
                              const float* xlen, int splits, void* workspace, void* stream);

/* Stride-2 fold (the prologue conv of every model, models.py:312: ConvBn1d(kernel_size_prologue = 11, stride = 2) on the 64 mel
 * channels).  A stride-2, dilation-1 conv over an EVEN number of frames Tin equals the stride-1 conv with K' taps and padding P'
 * over the same memory read as (Tin / 2) frames of 2 Cin channels (frames 2r, 2r+1 side by side -- a view, no copy):
 *   P' = ceil(pad / 2), s0 = 2 P' - pad, K' = (K - 1 + s0) / 2 + 1,   w'[co][p Cin + ci][j] = w[co][ci][2 j + p - s0] (0 outside [0, K)),
 * called as convasr_conv1d_fwd(x, packed', y, ..., Cin = 2 Cin, Tin = Tin / 2, Tout = the stride-2 conv's own Tout, K', 1, 1, P') and
 * convasr_conv1d_wgrad the same way.  K = 11, pad = 5, Cin = 64 gives K' = 6, P' = 3, 128 channels: inside the envelope of the
 * LDS-DMA kernels, which a stride-2 / 64-channel problem is not.
 *   convasr_fold2_geometry      K, pad -> K', P'
 *   convasr_fold2_pack_weight   fp32 (Cout, Cin, K) parameter in layout w_layout -> packed forward operand [K'][cout_pad(Cout)][2 Cin]
 *   convasr_fold2_unfold_wgrad  fp32 gradient of the folded conv, tap-major [K'][Cout][2 Cin] (convasr_conv1d_wgrad with
 *                               CONVASR_W_KMAJOR) -> dw (+)= the parameter's gradient in layout dw_layout */
int convasr_fold2_geometry(int K, int pad, int* K_folded, int* pad_folded);
int convasr_fold2_pack_weight(const float* w, int w_layout, void* packed_fwd, int dtype, int Cout, int Cin, int K, int pad, void* stream);
int convasr_fold2_unfold_wgrad(const float* dw_folded, float* dw, int dw_layout, int Cout, int Cin, int K, int pad, int accumulate, void* stream);

/* A/B and test hook: bit 0 = 0 routes bf16 / fp16 launches through the general register-staged kernels instead of the LDS-DMA kernels;
 * bits 8 and up are diagnostic switches documented where they are read (e.g. 8192 << 8: no one-tap kernel, 32768 << 8: the workgroup
 * form of convasr_ctc_alignment for every target length).  Returns the previous setting of bit 0; the switches are cleared by the next call. */
int convasr_debug_set_conv_v2(int enable);

/* Bytes of fp32 workspace convasr_conv1d_wgrad needs (split-K partial slabs). */
int64_t convasr_conv1d_wgrad_workspace_bytes(int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int dil);

/* dw[co][ci][k] (+)= sum_{b,t} dy[b,t,co] * x[b, t*stride + k*dil - pad, ci]; dw is the fp32 (Cout, Cin, K) gradient in layout
 * dw_layout (CONVASR_W_REFERENCE: the reference's parameter layout; CONVASR_W_KMAJOR: the training arena's).
 * accumulate != 0 adds to dw.  dbias (Cout fp32, may be NULL) = sum dy. */
int convasr_conv1d_wgrad(const void* x, const void* dy, float* dw, float* dbias, void* workspace, int dtype,
                         int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int dil, int pad,
                         int accumulate, int dw_layout, void* stream);

/* Which kernel convasr_conv1d_wgrad (x_ld = dy_ld = 0) or convasr_conv1d_wgrad_ld (frames x_ld / dy_ld elements apart) would launch for this
 * geometry under the current convasr_debug_set_conv_v2 state: 0 = the call would be refused, 1 = the general kernel, 2 = the LDS-DMA kernel.
 * out[5] = splits, chunks_per_split, chunks_per_b, tap_groups, x_rows of the plan that launch would use (untouched when 0 is returned).
 * Launches nothing and needs no GPU: the tests ask it which shapes reach which edge of the kernels. */
int convasr_conv1d_wgrad_plan(int dtype, int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int dil, int x_ld, int dy_ld, int* out);

/* ---- grouped Conv1d: models.py:50-64 (ConvSamePadding(separable = True): nn.Conv1d(Cin, Cout, K, groups = G) -> ReLU -> 1x1 conv), ---------
 * ---- JasperNetSeparable (models.py:1372-1374, G = 128).  The 1x1 half is convasr_conv1d_*; this is the grouped half. ------------------ */

/* y[b,t,co] = act(bias[co] + sum_k sum_{j < Cin/G} x[b, t stride + k - pad, (co / (Cout/G)) Cin/G + j] w[co][j][k]); relu != 0: act = ReLU.
 * x, y channels-last (B, T, C) of `dtype` (F32 / BF16 / F16); w the fp32 (Cout, Cin / G, K) parameter with element strides
 * (w_sco, w_sj, w_sk) -- torch-contiguous or the training arena's tap-major view; at most 8 channels per group on either side. */
int convasr_grouped_conv1d_fwd(const void* x, const float* w, int64_t w_sco, int64_t w_sj, int64_t w_sk, const float* bias, void* y, int dtype,
                               int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int pad, int groups, int relu, void* stream);
/* dx = input gradient (stride 1 only); y_act (may be NULL): the forward's post-ReLU output -- the gradient passes where it is > 0. */
int convasr_grouped_conv1d_dgrad(const void* dy, const void* y_act, const float* w, int64_t w_sco, int64_t w_sj, int64_t w_sk, void* dx, int dtype,
                                 int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int pad, int groups, void* stream);
/* dw (+)= weight gradient (same strides as w), dbias (may be NULL) (+)= sum of the gated dy; per-utterance partial sums go through
 * `workspace` and are added in a fixed order (no atomics). */
int64_t convasr_grouped_conv1d_wgrad_workspace_bytes(int B, int Cin, int Cout, int K, int groups);
int convasr_grouped_conv1d_wgrad(const void* x, const void* dy, const void* y_act, float* dw, int64_t w_sco, int64_t w_sj, int64_t w_sk, float* dbias,
                                 void* workspace, int dtype, int B, int Cin, int Cout, int Tin, int Tout, int K, int stride, int pad, int groups,
                                 int accumulate, void* stream);

/* ---- BatchNorm1d + ResidualActivation + temporal mask: models.py:111-114, 127-139, 357-371, 436-443 ----------- */

/* From the conv epilogue's stats (sum, sumsq over n = B*T values per channel): batch mean / biased var ->
 * scale = gamma * invstd, shift = beta - mean * scale; mean/invstd saved for backward; running stats updated
 * with momentum (running_var with the unbiased estimate), exactly nn.BatchNorm1d training semantics.
 * stats: [stats_rows][2][C] partial sums as the conv epilogue writes them (stats_rows = 1: plain totals), added in a fixed order.
 * num_batches_tracked (may be NULL) is incremented. */
int convasr_bn_finalize(const double* stats, int stats_rows, int64_t n, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, float eps,
                        float* mean, float* invstd, float* scale, float* shift, int C,
                        int64_t* num_batches_tracked, void* stream);
/* out[c] = sum over rows of part[r][c] (fp64, the same fixed order): totals of a partial-sum buffer for callers that want them. */
int convasr_reduce_rows(const double* part, int rows, int width, double* out, void* stream);

/* eval: scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale. */
int convasr_bn_eval_scale_shift(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                                float eps, float* scale, float* shift, int C, void* stream);

/* z = mask_t( dropout( act( y * scale[c] + shift[c] + sum_r (res_r * rscale_r[c] + rshift_r[c]) ) ) ).
 * y, z, res_r channels-last (B, T, C) of `dtype`.  n_res <= 12; rscale_r NULL means the residual is added as is.
 * dropout_p == 0 disables dropout; otherwise a counter-based hash of (seed, offset, element index) decides.
 * step_key (may be NULL; here and in the three backward entry points that re-derive the mask): one device word XORed into the
 * whitened seed when the kernel runs -- the per-step key convasr_step_begin() advances -- so that a training step captured into a
 * HIP graph (whose by-value arguments are frozen) draws fresh masks at every replay, the same ones an eager step draws.
 * gate (may be NULL; B*T*C/8 bytes; activations with derivative 0 or 1 only: none / relu / hardtanh): bit (e & 7) of byte (e >> 3) for
 * element e = (b*T + t)*C + c is set iff the gradient passes the element -- inside the activation's linear range, kept by dropout,
 * frame not masked.  The backward passes below take it back in: g = dz * (1 / (1 - p)) or 0, with no re-derivation of the
 * pre-activation, no hash and no frame arithmetic (bit-identical to the re-derived g). */
int convasr_bn_act_fwd(const void* y, void* z, int dtype, const float* scale, const float* shift,
                       int n_res, const void* const* res, const float* const* rscale, const float* const* rshift,
                       int act, float act_lo, float act_hi, float dropout_p, uint64_t seed, uint64_t offset, const uint64_t* step_key,
                       const float* xlen, int B, int T, int C, uint8_t* gate, void* stream);

/* Backward of the above, pass 1.  g = dz * mask * dropout * act'(pre), pre recomputed from y (and residuals).
 * Writes g (same dtype; g may be NULL when pass 2 recomputes it from dz) and reduces per channel: sums[0..C) += sum g, sums[C..2C) += sum g * xhat with
 * xhat = (y - mean) * invstd, and for each of the first two residuals r with BN: rsums_r likewise w.r.t. (res_r, rmean_r,
 * rinvstd_r).  sums / rsums_r (2*C doubles each) are WRITTEN (block partials go through `workspace`, then an fp64 sum:
 * deterministic, no contended atomics).  workspace: convasr_bn_bwd_workspace_bytes(B, T, C) bytes.
 * Optional outputs for the main BN (need mean / invstd): coef (3*C floats: dy = coef[c]*g + coef[C+c]*y + coef[2C+c], the
 * batch-norm training backward with `gamma` folded in), dgamma = sum g*xhat, dbeta = sum g (added to when accumulate).
 * gate (may be NULL): the one-bit gates convasr_bn_act_fwd stored; then g = gate ? dz / (1 - p) : 0 with no re-derivation (n_res must be
 * 0, g NULL, mean / invstd given): three streams in, two sums out. */
int64_t convasr_bn_bwd_workspace_bytes(int B, int T, int C);
int convasr_bn_act_bwd_reduce(const void* dz, const void* y, void* g, int dtype, const float* scale, const float* shift,
                              const float* mean, const float* invstd,
                              int n_res, const void* const* res, const float* const* rscale, const float* const* rshift,
                              const float* const* rmean, const float* const* rinvstd, double* const* rsums,
                              int act, float act_lo, float act_hi, float dropout_p, uint64_t seed, uint64_t offset, const uint64_t* step_key,
                              const float* xlen, double* sums, void* workspace, const float* gamma, float* coef, float* dgamma, float* dbeta,
                              int accumulate, int B, int T, int C, const uint8_t* gate, void* stream);

/* Backward pass 2 in coefficient form: dy = coef[c]*g + coef[C+c]*y + coef[2C+c].  from_dz != 0: g is recomputed on the fly
 * from dz (activation derivative, dropout, temporal mask; no residuals) so pass 1 need not materialise it; gate (may be NULL): the
 * one-bit gates convasr_bn_act_fwd stored, used instead of the re-derivation (dropout_p still supplies the 1 / (1 - p)). */
int convasr_bn_act_bwd_apply(const void* dz_or_g, const void* y, void* dy, int dtype, const float* coef, int from_dz,
                             const float* scale, const float* shift, int act, float act_lo, float act_hi, float dropout_p,
                             uint64_t seed, uint64_t offset, const uint64_t* step_key, const float* xlen, int B, int T, int C, const uint8_t* gate, void* stream);

/* Backward pass 2: dy = gamma * invstd * (g - sum_g / n - xhat * sum_gxhat / n)  (batch-norm training backward);
 * dgamma = sum_gxhat, dbeta = sum_g (written, or added when accumulate).  In place allowed (dy == g). */
int convasr_bn_bwd_apply(const void* g, const void* y, void* dy, int dtype, const float* gamma, const float* mean,
                         const float* invstd, const double* sums, float* dgamma, float* dbeta, int accumulate,
                         int B, int T, int C, void* stream);

/* ---- head: models.py:316 (log_softmax), 323 (F.ctc_loss), 645-657 (entropy), transcript_generators.py:27 (argmax) */

/* logits/log_probs channels-last (B, T, C) fp32. */
int convasr_log_softmax_fwd(const float* logits, float* log_probs, int64_t rows, int C, void* stream);
/* dlogits = g - exp(lp) * sum_c g */
int convasr_log_softmax_bwd(const float* grad_lp, const float* log_probs, float* dlogits, int64_t rows, int C, void* stream);

int64_t convasr_ctc_workspace_bytes(int B, int T, int S_max);
/* nll[b] = -log p(targets[b,:ylen[b]] | log_probs[b,:olen[b]]) with blank = `blank`, +inf when infeasible
 * (zero_infinity=False).  grad (B,T,C) = d nll / d log_probs as ATen defines it: exp(lp) - posterior for t < olen,
 * 0 for t >= olen (may be NULL: forward only).  targets: (B, S_max) int64, olen/ylen int64 (the reference's dtypes).
 * Envelope: S_max <= 1,023 labels, T <= ~13,000 frames (the per-frame hand-over slots of the two-wave sweeps live in LDS); beyond it
 * the call fails with CONVASR_EUNSUPPORTED / an invalid-argument error and launches nothing. */
int convasr_ctc_loss(const float* log_probs, const int64_t* targets, const int64_t* olen, const int64_t* ylen,
                     float* nll, float* grad, void* workspace, int B, int T, int C, int S_max, int blank, void* stream);
/* 1 when convasr_ctc_loss takes the shape -- S_max within its label limit, T within what its LDS hand-over slots hold, C <= 8192 -- and 0
 * when it refuses it: what a caller asks before it chooses between the call above and convasr_ctc_loss_long (ops.ctc_loss does). */
int convasr_ctc_loss_supported(int B, int T, int C, int S_max);

/* The same loss and gradient (F.ctc_loss at models.py:323 with no limit on target or input length) for whole recordings: arguments,
 * results and edge cases are those of convasr_ctc_loss -- +inf and a zero gradient for an infeasible utterance, 0 / +inf for olen == 0
 * with an empty / non-empty target, a -inf log-prob staged as the finite sentinel, a non-finite loss for a NaN log-prob, a zero gradient
 * at frames >= olen, ragged olen / ylen and empty targets within one batch.  Both lattices are cut into tiles of
 * convasr_ctc_loss_long_states_per_block() states x chunk frames, one wave per tile; launch k of ceil(T / chunk) + ceil((2 S_max + 1) /
 * states_per_block) - 1 plain launches runs the k-th anti-diagonal of the alpha sweep and of the beta sweep (alpha tiles in which no
 * state can be reached yet, s > 2t + 1, are not launched; beta tiles beyond an utterance's own reach end at once), then one launch for
 * the totals and one for the gradient (one wave per frame, a fixed order of additions, no atomics on global memory).  Nothing waits inside
 * a launch.  Arithmetic: fp32 log-sum-exp in base 2, renormalised per block of states by integer log2 offsets at every frame whose
 * absolute index is a multiple of 8; the result does not depend on chunk_frames: 0 = convasr_ctc_loss_long_chunk_frames() (256), or
 * 16 .. 4096 to force the chunk length (tests and tuning).  grad may be NULL (forward only).  workspace: at least
 * convasr_ctc_loss_long_workspace_bytes bytes, 16-byte aligned, uninitialised: two fp32 lattices [B][T][blocks x states_per_block] and
 * their offsets [B][blocks][T] -- ten minutes (30,000 frames, 9,000 labels) take about 4.4 GB.  Envelope: 0 <= S_max <= 131071,
 * 1 <= T <= 2^20, 2 <= C <= 8192, 1 <= B <= 65535, checked before any launch; outside it CONVASR_EUNSUPPORTED (the query returns that
 * negative code, with a message), any other bad argument CONVASR_EINVAL.  Not for stream capture (hundreds of launches over a per-call
 * workspace). */
int convasr_ctc_loss_long_states_per_block(void);
int convasr_ctc_loss_long_chunk_frames(void);
int64_t convasr_ctc_loss_long_workspace_bytes(int B, int T, int C, int S_max);
int convasr_ctc_loss_long(const float* log_probs, const int64_t* targets, const int64_t* olen, const int64_t* ylen, float* nll, float* grad,
                          void* workspace, int64_t workspace_bytes, int B, int T, int C, int S_max, int blank, int chunk_frames, void* stream);
/* CTC over PARTIAL transcripts: a star token -- "any stretch of frames may stand here, or nothing at all" -- in the gaps of the transcript
 * that star_mask allows (csrc/star_ctc.hip).  The rule is this project's own (the W-CTC / Star Temporal Classification family), pinned
 * against no outside implementation.  log_probs, targets, olen, ylen, blank, nll as in convasr_ctc_loss; star_mask (B, S_max + 1) bytes:
 * entry g != 0 allows a star in gap g, which lies before label g (gap ylen[b]: after the last label; entries past ylen[b] are ignored);
 * star_penalty <= 0: natural log, paid per frame spent in a star; star_enter <= 0: natural log, paid once per star that is used.
 *   Units: the labels with a star unit inserted in every allowed gap, n <= 2 S + 1 of them (two stars are never adjacent).  State 2i is
 *   the blank before unit i, state 2i + 1 is unit i, state 2n the last blank.  A blank emits lp[t, blank], a label lp[t, y], a star the
 *   constant star_penalty (it matches every frame, silence included, and takes no gradient).
 *   Arcs into state s from frame t - 1: s; s - 1; s - 2 when s is a unit that differs from unit s - 2 (a star differs from every label);
 *   the arcs s - 1 and s - 2 INTO a star also pay star_enter (its self arc does not); and, a star being optional, when unit s - 2 is a
 *   star: s - 3 (the blank before that star) and s - 4 (the unit before it) when that unit differs from unit s.
 *   Start states: 0 and 1 (state 1 pays star_enter when unit 0 is a star), and 3 when unit 0 is a star.  End states: 2n and 2n - 1, and
 *   2n - 2 and 2n - 3 when the last unit is a star.  nll = -log of the sum over all paths; +inf where there is none.
 *   Equivalently exp(-nll) = sum over the subsets A of the allowed gaps of exp(|A| star_enter) * P_ctc(labels with a star class at the gaps
 *   in A | log_probs with one more column holding star_penalty)  (tests/test_star_ctc_ref.py checks that through F.ctc_loss).
 * grad (B,T,C; may be NULL) in convasr_ctc_loss's convention: occ[b,t] * exp(lp[b,t,c]) - post[b,t,c] for t < olen[b], 0 beyond and for an
 * infeasible utterance; post = the posterior mass of the label and blank states of class c, occ = sum_c post = the share of the paths
 * that is not inside a star at frame t (1 everywhere with an all-zero mask: the plain formula; any multiple of exp(lp) vanishes in
 * log_softmax's backward, so the logits' gradient is the true one).  star_frames (B, S_max + 1) fp32: the expected number of frames
 * every gap's star absorbs (0 for a gap without one): where it is large the transcript lacks speech.
 * One workgroup per utterance, both sweeps in one loop with a workgroup barrier per frame, every loop bounded by T or the state count;
 * fp32 in base 2 with convasr_ctc_loss's finite sentinel, every (blank, unit) pair of states renormalised by an integer offset of its
 * own every convasr_star_ctc_renorm_frames() frames; a wave holds convasr_star_ctc_states_per_wave() states, the lattice rows are that
 * many states rounded up over 4 S_max + 3 (what the tests straddle).  Two plain launches, no memset or copy, no host synchronisation; nll and grad
 * are bit-reproducible, star_frames (fp32 atomics between workgroups) to rounding.  workspace: convasr_star_ctc_workspace_bytes bytes,
 * uninitialised.  Envelope, checked before any launch: S_max <= 255 (convasr_star_ctc_max_states() = 1,023 states with every gap
 * starred), T <= 8192, 2 <= C <= 8192, B <= 65535; outside it CONVASR_EUNSUPPORTED (the workspace query returns that code) -- never a
 * silent plain loss; a positive or NaN penalty, NULL, blank outside [0, C): CONVASR_EINVAL.  What only the device sees is read
 * defensively: olen outside [0, T] or ylen outside [0, S_max] give +inf, a label outside [0, C) is a unit nothing matches. */
int convasr_star_ctc_states_per_wave(void);
int convasr_star_ctc_renorm_frames(void);
int convasr_star_ctc_max_states(void);
int convasr_star_ctc_supported(int B, int T, int C, int S_max);
int64_t convasr_star_ctc_workspace_bytes(int B, int T, int C, int S_max);
int convasr_star_ctc_loss(const float* log_probs, const int64_t* targets, const int64_t* olen, const int64_t* ylen, const uint8_t* star_mask,
                          float star_penalty, float star_enter, float* nll, float* grad, float* star_frames, void* workspace,
                          int B, int T, int C, int S_max, int blank, void* stream);
/* The BEST PATH through the star lattice above, at the size of whole recordings (csrc/star_align.hip): which frame every label of a
 * partial transcript occupies, and which frames the star of every gap absorbed -- the untranscribed audio.  The rule is this project's
 * own and is pinned against no outside aligner; the two costs are untuned.
 *   Units, states, the arc costs c[d][s] (d = 0 .. 4: 0, star_enter or "no arc" = -inf), start costs and end costs are exactly those
 *   of convasr_star_ctc_loss.  A star emits star_penalty at every frame, every other state log_probs[b, t, class]; star_penalty and
 *   star_enter are finite natural-log costs <= 0.  The sum becomes a maximum, in fp32, fl() = one rounding:
 *     v[0][s] = fl(start[s] + em[0][s]);   v[t][s] = fl(em[t][s] + max_d fl(v[t-1][s-d] + c[d][s]));
 *     the back-pointer of (t, s) is the SMALLEST d that attains the maximum;
 *     the path ends in the SMALLEST s that attains max_s (v[Tb-1][s] + end[s]), Tb = input_lengths[b]; only frames < Tb are read.
 *   This is true max-plus Viterbi.  It is NOT convasr_ctc_alignment's recursion (the reference's ctc.alignment), which carries a
 *   log-sum-exp and takes the argmax of its addends; with an all-zero mask the two agree wherever the best path is unambiguous.  As only
 *   max and one rounded addition per step occur, a float32 restatement with the same operations is equal bit for bit
 *   (tests/_star_align_ref.py).  In exact arithmetic the score is the maximum over the subsets A of the allowed gaps of |A| star_enter +
 *   the plain CTC Viterbi score of the labels with a star class at the gaps in A (tests/test_star_align_ref.py checks that).
 * Inputs: log_probs (B, T, C) fp32 contiguous; units (B, N_max) int32: row b's first n_units[b] entries are its units in order -- a class
 * in [0, C), -1 for a label outside it (it emits -inf), -(gap + 2) for the star of gap `gap` (what csrc/star_ctc.hip writes per state); the
 * caller builds the table (ops.star_ctc_alignment: cumsum and scatter on the device), the kernels do not scan a mask.  target_lengths (B,):
 * the labels among the units.  Outputs, all written by the walk kernel (no memset): alignment (B, S_max) int64, the last frame of the path
 * inside every label's state (convasr_ctc_alignment's convention; 0 past target_lengths[b]); star_begin (B, S_max + 1) int64, the first
 * frame the path spends in the star of gap g, -1 where that star is unused or absent; star_frames (B, S_max + 1) int64, how many frames
 * (contiguous by construction); score (B,) fp32.  No path (Tb <= 0, Tb > T, too few frames, n_units outside [0, N_max]): score -inf,
 * alignment 0, star_begin -1, star_frames 0.
 * Scheme: tiles of convasr_star_alignment_states_per_block() states x chunk frames, one wave per tile, one plain launch per
 * anti-diagonal, nothing waits inside a launch; back-pointers take 4 bits per (blank, unit) pair of states.  chunk_frames: 0 =
 * convasr_star_alignment_chunk_frames(), or 16 .. 4096 (tests and tuning; no output depends on it).  workspace: at least
 * convasr_star_alignment_workspace_bytes(B, T, N_max) bytes, 16-byte aligned, uninitialised.  Envelope, checked before any launch:
 * S_max <= 131071, N_max <= 2 * 131071 + 1, T <= 2^20, B <= 65535; outside it CONVASR_EUNSUPPORTED (the workspace query returns -1).
 * Eager only: the launch sequence depends on the shape and the workspace is per call.  parts: 1 = the sweep, 2 = the walk over a
 * workspace that a sweep with the same arguments filled, 3 = both. */
int convasr_star_alignment_states_per_block(void);
int convasr_star_alignment_chunk_frames(void);
int64_t convasr_star_alignment_workspace_bytes(int B, int T, int N_max);
int convasr_star_alignment(const float* log_probs, const int32_t* units, const int32_t* n_units, const int64_t* input_lengths, const int64_t* target_lengths,
                           float star_penalty, float star_enter, int64_t* alignment, int64_t* star_begin, int64_t* star_frames, float* score,
                           void* workspace, int64_t workspace_bytes, int B, int T, int C, int S_max, int N_max, int blank, int chunk_frames, void* stream);
int convasr_star_alignment_parts(const float* log_probs, const int32_t* units, const int32_t* n_units, const int64_t* input_lengths, const int64_t* target_lengths,
                                 float star_penalty, float star_enter, int64_t* alignment, int64_t* star_begin, int64_t* star_frames, float* score,
                                 void* workspace, int64_t workspace_bytes, int B, int T, int C, int S_max, int N_max, int blank, int chunk_frames, int parts,
                                 void* stream);
/* N-best minimum-word-error-rate (MWER) loss: the expected number of errors over an N-best list weighted by the hypotheses' CTC
 * likelihoods (csrc/mwer.hip).  The rule is this project's own (the sequence-level family of Prabhavalkar et al. 2018, Povey's sMBR),
 * pinned against no outside implementation; whether it lowers word error rate on speech is not shown anywhere in this project.
 * log_probs, olen, blank as in convasr_ctc_loss.  For utterance b and hypothesis n = 0 .. N - 1: hyps (B, N, L_max) int64, the first
 * hyp_lengths[b, n] entries are a collapsed label sequence (no blanks); hyp_lengths (B, N) int64: < 0 = the hypothesis is absent, 0 = the
 * empty transcript (a lattice of one blank state, valid); risk (B, N) fp32: a number of errors, any finite value, the caller's;
 * scale > 0, finite.
 *   ll[b,n] = log P_ctc(hyps[b,n] | log_probs[b, :olen[b]]), the ordinary CTC sum over alignments; hyp_nll = -ll, +inf where no
 *   alignment fits, where the hypothesis is absent, hyp_lengths[b,n] > L_max or olen[b] is outside [1, T].
 *   A hypothesis TAKES PART iff hyp_nll is finite.  Over those that take part: p[b,n] = softmax_n(scale * ll[b,n]) (hyp_posterior),
 *   E[b] = sum_n p risk, rbar[b] = the plain mean of their risks, loss[b] = E[b] - rbar[b], w[b,n] = scale p[b,n] (risk[b,n] - E[b]),
 *   grad[b,t,c] = sum_n w[b,n] posterior_{b,n}(class c at frame t) for t < olen[b], 0 beyond.  The others have p = 0 and w = 0.  With
 *   no hypothesis taking part, or only one (p = 1), loss and grad are exactly 0.
 *   sum_n w = 0, so the gradient's class sum is 0 in every frame: the true derivative with respect to the log-probs and
 *   convasr_ctc_loss's exp(lp) - posterior convention are the same tensor, and log_softmax's backward passes it unchanged.
 * grad (B,T,C) may be NULL (the third launch is left out).  Three plain launches on `stream`, no memset, copy, host synchronisation or
 * atomics on global memory: loss, hyp_nll, hyp_posterior and grad are bit-reproducible.  (1) one workgroup per (b, n), all N reading the
 * utterance's slab in place: both sweeps in one loop with a workgroup barrier per frame, every loop bounded by T or the state count,
 * fp32 in base 2 with convasr_ctc_loss's finite sentinel, every (blank, label) pair of states renormalised by an integer offset of its
 * own every convasr_mwer_renorm_frames() frames; a wave holds convasr_mwer_states_per_wave() states, a workgroup has a thread per 2 L_max + 1
 * states rounded up to that (what the tests straddle); (2) one wave per utterance, a lane per hypothesis; (3) one wave per (b, t).
 * workspace: convasr_mwer_workspace_bytes bytes, uninitialised: (2 B N T ls + B N (T / renorm + 1) ls + 5 B N) * 4 with ls = 2 L_max + 2
 * (both lattices of every hypothesis and their offsets).
 * Envelope, checked before any launch: N <= convasr_mwer_max_hyps() = 64, L_max <= convasr_mwer_max_labels() = 511 (1,023 states),
 * T <= 8192, 2 <= C <= 8192, B <= 65535; outside it CONVASR_EUNSUPPORTED (the workspace query returns that code) and nothing is
 * launched; scale <= 0 or not finite, NULL, blank outside [0, C): CONVASR_EINVAL.  What only the device sees is read defensively: a
 * label outside [0, C) matches nothing (hyp_nll = +inf). */
int convasr_mwer_states_per_wave(void);
int convasr_mwer_renorm_frames(void);
int convasr_mwer_max_labels(void);
int convasr_mwer_max_hyps(void);
int convasr_mwer_supported(int B, int N, int T, int C, int L_max);
int64_t convasr_mwer_workspace_bytes(int B, int N, int T, int C, int L_max);
int convasr_mwer_loss(const float* log_probs, const int64_t* hyps, const int64_t* hyp_lengths, const int64_t* olen, const float* risk, float scale,
                      float* loss, float* grad, float* hyp_nll, float* hyp_posterior, void* workspace,
                      int B, int N, int T, int C, int L_max, int blank, void* stream);
/* out[b,t,c] = grad[b,t,c] * gscale[b]  (chain rule for reduction='none'); with gdiv != NULL the factor is
 * gscale[b] / (float)gdiv[b * gdiv_stride]: the "/ ylen[:, 0]" of models.py:323 folded into the same pass.  gscale NULL (gdiv given):
 * the factor is 1 / gdiv -- the same division in the forward direction (per_b = 1: nll[b] / ylen[b, 0]). */
int convasr_scale_rows(const float* grad, const float* gscale, const int64_t* gdiv, int64_t gdiv_stride, float* out, int B, int64_t per_b, void* stream);

/* The scalar bookkeeping of one training iteration (train.py:754-756, 769) in one launch: loss_vec[b] = per-utterance loss
 * (models.py:323), w[b] = ylen[b * ylen_stride] (target lengths), entropy[b] (may be NULL) = models.entropy per utterance:
 *   out3[0] = mean(loss_vec * w) / accumulate_iterations, out3[1] = mean(loss_vec), out3[2] = mean(entropy);
 *   grad_loss_vec[b] (may be NULL) = d out3[0] / d loss_vec[b] = ((1 / accumulate_iterations) / B) * w[b];
 *   skipped (may be NULL, one byte) = out3[1] is inf or NaN (the gate of train.py:769).
 * loss_scaler (may be NULL): a dynamic loss scaler's state (below); grad_loss_vec is multiplied by its current scale, i.e. backward is
 * seeded with the gradient of the SCALED loss (`with apex.amp.scale_loss(loss, optimizer) as scaled_loss: scaled_loss.backward()`,
 * train.py:770-772).  metric_scale multiplies out3[1] and out3[2] (1 for one process; 1 / world size in data-parallel runs, so that the
 * SUM all-reduce of train.py:759-760 yields the mean of train.py:761-762 with no further kernel); skipped looks at the local mean. */
int convasr_loss_head(const float* loss_vec, const int64_t* ylen, int64_t ylen_stride, const float* entropy, int B, float accumulate_iterations, float* out3,
                      float* grad_loss_vec, unsigned char* skipped, const float* loss_scaler, float metric_scale, void* stream);

/* Dynamic loss scaler for fp16 training (the role of apex.amp's LossScaler, reference models.py:744-762 `apex.amp.initialize(opt_level)`
 * and train.py:770-779): CONVASR_LOSS_SCALER_FLOATS floats on the device,
 *   [0] scale  [1] clean steps since the last change  [2] did the last step overflow (0 / 1)  [3] growth window (0 = static scale)
 *   [4] min scale  [5] max scale  [6] factor  [7] number of steps skipped for overflow so far
 * read by convasr_loss_head (backward seed x scale), convasr_sumsq (the reported norm is that of the UNSCALED gradient, what
 * clip_grad_norm_ sees on apex's master gradients) and the fused optimizer steps (gradients x 1 / scale; a non-finite sum of squares =
 * overflow: parameters and optimizer state stay untouched).  The optimizer step writes the next state into a SECOND buffer
 * (scaler_in != scaler_out; the caller swaps them per step) with apex's update_scale(): overflow -> scale = max(min, scale / factor),
 * clean = 0; otherwise ++clean, and at clean == window: scale = min(max, scale * factor), clean = 0.  A step gated by a non-finite
 * LOSS (loss_gate) copies the state unchanged: the reference never enters scale_loss on such an iteration. */
#define CONVASR_LOSS_SCALER_FLOATS 8

/* ent[b] = sum_{t<olen} -sum_c p log p / (eps + olen[b])  (olen NULL: mean over T). */
int convasr_entropy(const float* log_probs, const int64_t* olen, float* ent, int B, int T, int C, float eps, void* stream);
/* weighted_mean_entropy (models.py:660-682, logged by train.py:137-139): per frame e = -sum_c p log p, w = 1 - p[eps_id]; out[b] =
 * sum_{t<olen} e w / (eps + sum_{t<olen} w)  (olen NULL: all T frames). */
int convasr_weighted_mean_entropy(const float* log_probs, const int64_t* olen, float* out, int B, int T, int C, int eps_id, float eps, void* stream);
/* idx[b,t] = argmax_c log_probs[b,t,c] (first maximum, like torch.argmax on CPU). */
int convasr_argmax(const float* log_probs, int64_t* idx, int64_t rows, int C, void* stream);

/* ---- optimizer: train.py:777-782 (clip_grad_norm_, SGD step), optimizers.py:66-90 (NovoGrad) ------------------- */

/* sumsq[0] = sum g^2 over n fp32 values, in double, added in a fixed order (partial sums in `workspace`, no atomics). */
int64_t convasr_sumsq_workspace_bytes(void);
/* norm_out (may be NULL) receives (float)(sqrt(sumsq) * norm_scale) (/ the loss scaler's scale when loss_scaler != NULL): what clip_grad_norm_ returns. */
int convasr_sumsq(const float* g, int64_t n, double* sumsq, void* workspace, float* norm_out, float norm_scale, const float* loss_scaler, void* stream);
/* torch.optim.SGD step with clip folded in: c = min(1, max_norm / (sqrt(sumsq) + 1e-6)) (c = 1 if sumsq NULL);
 * g' = c*g + wd*p; buf = first ? g' : mom*buf + g'; p -= lr * (nesterov ? g' + mom*buf : buf).
 * If grad_out != NULL the clipped gradient c*g is written back (what clip_grad_norm_ leaves in .grad).
 * grad_scale multiplies g before everything else (1 / world size when g holds rank-SUMMED gradients: the mean is never
 * materialised; sumsq is then the sum of squares of the summed gradient).
 * If loss_gate != NULL and *loss_gate (a device float, the all-reduced loss) is inf or NaN the launch changes nothing: the
 * reference's "skip the step on a non-finite loss" (train.py:769-772) without a host round trip in the middle of the step.
 * p16 (may be NULL): n values of p16_dtype (CONVASR_BF16 or CONVASR_F16), receives the updated parameters rounded to that type -- with
 * K-major masters that mirror IS the packed forward weight of every conv whose Cout is a multiple of the kernel's N tile (no
 * per-step packing launches).  scaler_in / scaler_out (both or neither): the dynamic loss scaler above; needs sumsq.
 * lr_dev (may be NULL; likewise in the two optimizers below): one device float that replaces `lr` when the kernel runs -- a captured
 * step graph follows the host's learning-rate schedule (optimizers.py:13-63, train.py:783) through it. */
int convasr_sgd_step(float* p, const float* g, float* buf, float* grad_out, int64_t n, const double* sumsq, float max_norm,
                     float lr, float momentum, float weight_decay, int nesterov, int first, const float* loss_gate, float grad_scale,
                     void* p16, int p16_dtype, const float* scaler_in, float* scaler_out, const float* lr_dev, void* stream);
/* torch.optim.AdamW step (train.py:663-668; decoupled weight decay, no amsgrad) with the same folded-in pieces as convasr_sgd_step:
 * g' = c*grad_scale*g (c from sumsq / max_norm as above); p *= 1 - lr*wd; m = b1*m + (1-b1)*g'; v = b2*v + (1-b2)*g'^2;
 * p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps), t = step_in[0] + 1.  step_in / step_out: one device float each, distinct
 * buffers the caller swaps per call: the number of steps APPLIED so far (a launch gated by loss_gate or skipped by the loss scaler
 * writes step_out[0] = step_in[0] and changes nothing else, so the bias corrections follow the applied steps like torch's state['step']).
 * loss_gate, grad_scale, p16 / p16_dtype, scaler_in / scaler_out: as in convasr_sgd_step. */
int convasr_adamw_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t n, const double* sumsq, float max_norm, float lr,
                       float beta1, float beta2, float eps, float weight_decay, const float* step_in, float* step_out, const float* loss_gate,
                       float grad_scale, void* p16, int p16_dtype, const float* scaler_in, float* scaler_out, const float* lr_dev, void* stream);

/* Fused backward step (bf16 / fp16 storage `dtype`, stride 1): dx = dgrad(dy) of one Conv1d -- i.e. dz of the Conv+BN+activation layer that produced
 * this conv's input -- plus pass 1 of THAT layer's batch-norm backward in the epilogue, on the tile just produced:
 * g = dx * act'(bn_y*bn_scale+bn_shift) * dropout * mask(bn_xlen); bn_sums[c] += sum g, bn_sums[C+c] += sum g*(bn_y-mean)*invstd

 * (C = Cin of this conv) written as per-m-tile partial rows bn_sums[rows][2][C], *bn_rows rows (<= convasr_conv_stats_max_rows(B, T_dx)).  It replaces
 * convasr_conv1d_fwd(dy, packed_dgrad) + convasr_bn_act_bwd_reduce(write_g = 0) (models.py:111-139 backward) when dx has this
 * single consumer.  dy is (B, T_dy, Cout), dx and bn_y are (B, T_dx, Cin); pad = dil*(K-1) - padding of the forward conv.  Returns 1 (nothing launched) when the shape is outside the
 * LDS-DMA kernel's envelope (Cout % 64 != 0): run the two calls separately.  bn_gate (may be NULL): that layer's one-bit gates
 * from convasr_bn_act_fwd, used instead of re-deriving act' / dropout / mask per element in the epilogue. */
int convasr_conv1d_dgrad_bn_reduce(const void* dy, const void* packed_dgrad, void* dx, int dtype, int B, int Cout, int Cin, int T_dy, int T_dx, int K,
                                   int dil, int pad, const void* bn_y, const float* bn_scale, const float* bn_shift, const float* bn_mean,
                                   const float* bn_invstd, int bn_act, float bn_act_lo, float bn_act_hi, float dropout_p, uint64_t seed,
                                   uint64_t offset, const uint64_t* step_key, const float* bn_xlen, double* bn_sums, int* bn_rows, const uint8_t* bn_gate, void* stream);
/* coef / dgamma / dbeta from those partial rows (the second half of convasr_bn_act_bwd_reduce), added in a fixed order; n = B*T. */
int convasr_bn_bwd_finalize(const double* sums, int sums_rows, const float* gamma, const float* mean, const float* invstd, float* coef,
                            float* dgamma, float* dbeta, int accumulate, int64_t n, int C, void* stream);

/* ---- grouped one-tap launches: the residual branches of a dense block (models.py:107-110, 129-131) ------------------ */

/* n (<= 12) independent Conv1d(kernel_size = 1) problems over the SAME B * T frames in one dispatch (two when some problems have a long
 * reduction into few channels): y_i (+)= x_i * w_i^T (+ bias_i).  x_i channels-last (B, T, cin[i]) and y_i (B, T, cout[i]) of `dtype`
 * (CONVASR_BF16 / CONVASR_F16), w_i the packed forward layout [1][cout[i]][cin[i]] (convasr_pack_conv_weight; for an input gradient: the
 * packed dgrad layout with the roles of the channel counts swapped), bias (array or NULL; entries may be NULL), stats (array or NULL;
 * entries may be NULL): per-m-tile partial rows exactly as convasr_conv1d_fwd writes them, *stats_rows rows each; accumulate (array or
 * NULL): entry != 0 adds into y_i (the sum of the two stored 16-bit values, rounded once) -- the input gradients of the branches land in
 * the tapped block output's gradient without autograd's pairwise adds.  Each problem is computed exactly as convasr_conv1d_fwd computes
 * it alone (bit-identical per element).  cin[i] % 64 == 0, cout[i] % 128 == 0, else CONVASR_EUNSUPPORTED (launch them one by one). */
int convasr_conv1x1_grouped(int n, const void* const* x, const void* const* w, void* const* y, const float* const* bias, double* const* stats,
                            const int* cin, const int* cout, const int* accumulate, int dtype, int B, int T, int* stats_rows, void* stream);
/* The weight gradients of the same n branches, dw_i[co][ci] (+)= sum over (b, t) of dy_i[b, t, co] * x_i[b, t, ci] (fp32, cout[i] x cin[i],
 * the memory order of a one-tap (Cout, Cin, 1) parameter in either layout), in ONE dispatch of the LDS-DMA weight-gradient kernel over all
 * problems' (co tile, ci tile, split) units + ONE streaming combine of the split-K slabs (deterministic: fixed order, no atomics).
 * zero (array or NULL; entries may be NULL): cout[i] floats set to zero by the combine -- the branch conv's bias gradient, identically zero
 * ahead of a train-mode batch norm.  accumulate (array or NULL): add into dw_i.  workspace: convasr_wgrad1x1_grouped_workspace_bytes()
 * bytes.  cin[i] % 128 == 0 and cout[i] % 128 == 0, else CONVASR_EUNSUPPORTED. */
int64_t convasr_wgrad1x1_grouped_workspace_bytes(int n, const int* cin, const int* cout, int B, int T);
/* out[2] = splits, chunks_per_split common to the n problems of a convasr_wgrad1x1_grouped launch; returns 1, or 0 where that launch would be
 * refused (more than 12 problems, channel counts not multiples of 128, fp32).  Launches nothing and needs no GPU. */
int convasr_wgrad1x1_grouped_plan(int n, const int* cin, const int* cout, int dtype, int B, int T, int* out);
int convasr_wgrad1x1_grouped(int n, const void* const* x, const void* const* dy, float* const* dw, float* const* zero, const int* cin, const int* cout,
                             const int* accumulate, void* workspace, int dtype, int B, int T, void* stream);
/* The batch norms of those branches (nn.BatchNorm1d at models.py:110, one per branch, all of the block's channel count C), grouped the same
 * way.  convasr_bn_finalize_grouped: convasr_bn_finalize for `count` (<= 13) batch norms in one launch; out[i] receives 4 C floats (mean,
 * invstd, scale, shift), stats[i] has stats_rows partial rows.  convasr_bn_bwd_finalize_grouped: convasr_bn_bwd_finalize for `count` sets of
 * sums (sums_rows[i] partial rows each).  convasr_bn_bwd_apply_grouped: dy_i = coef_i[c] * g + coef_i[C + c] * y_i + coef_i[2 C + c] for
 * `count` (y_i, coef_i, dy_i) triples sharing ONE g, which is read once (count + 1 launches of convasr_bn_act_bwd_apply(from_dz = 0) read it
 * count + 1 times); 16-bit storage. */
int convasr_bn_finalize_grouped(int count, const double* const* stats, int stats_rows, int64_t n, const float* const* gamma, const float* const* beta,
                                float* const* running_mean, float* const* running_var, const float* momentum, const float* eps, float* const* out,
                                int64_t* const* num_batches_tracked, int C, void* stream);
int convasr_bn_bwd_finalize_grouped(int count, const double* const* sums, const int* sums_rows, const float* const* gamma, const float* const* mean,
                                    const float* const* invstd, float* const* coef, float* const* dgamma, float* const* dbeta, const int* accumulate,
                                    int64_t n, int C, void* stream);
int convasr_bn_bwd_apply_grouped(const void* g, int count, const void* const* y, const float* const* coef, void* const* dy, int dtype, int B, int T, int C, void* stream);
/* Pass 1 of a dense block's backward (models.py:127-139 backward) in ONE sweep, from the one-bit gates convasr_bn_act_fwd stored for the block's
 * output: g = gate ? dz / (1 - p) : 0 is written once, and for each of the `count` (<= 13) batch norms that feed the block's sum -- the main
 * one and the residual branches' (y_i its input, mean_i / invstd_i its batch statistics) -- sum g and sum g * (y_i - mean_i) * invstd_i
 * are formed (block partials in `workspace`, convasr_bn_bwd_reduce_many_workspace_bytes() bytes, then an fp64 sum in a fixed order: no
 * atomics) and turned into coef_i (3 C floats, as convasr_bn_act_bwd_reduce's), dgamma_i, dbeta_i (added to when accumulate[i]).  Replaces
 * convasr_bn_act_bwd_reduce (which re-derives the pre-activation from all residual inputs) + one further sweep per two branches. */
int64_t convasr_bn_bwd_reduce_many_workspace_bytes(int count, int B, int T, int C);
int convasr_bn_bwd_reduce_many(const void* dz, const uint8_t* gate, float dropout_p, void* g, int count, const void* const* y, const float* const* mean,
                               const float* const* invstd, const float* const* gamma, float* const* coef, float* const* dgamma, float* const* dbeta,
                               const int* accumulate, void* workspace, int dtype, int B, int T, int C, void* stream);
/* out = a + b over n 16-bit values (n % 8 == 0; in place allowed): the one explicit add a tapped block output's gradient needs (the main
 * path's input gradient + the branches' accumulated ones), in place of autograd's InputBuffer accumulation (models.py:129-131 backward). */
int convasr_add16(const void* a, const void* b, void* out, int64_t n, int dtype, void* stream);

/* The dgrad operands (convasr_pack_conv_weight's packed_dgrad, from packed_fwd, 16-bit) of MANY layers in one launch.  items: n_items
 * records in DEVICE memory, convasr_pack_dgrad_item_bytes() bytes each: {const void* packed_fwd; void* packed_dgrad; int Cout, Cin, K,
 * co_pad (= convasr_conv_cout_pad(Cout)), ci_pad (= convasr_conv_cout_pad(Cin)), first;} with first = the running sum of the earlier items'
 * K * ceil(Cout / 64) * ceil(Cin / 64) blocks and total_blocks = that sum over all items; Cout and Cin even. */
int convasr_pack_dgrad_item_bytes(void);
int convasr_pack_dgrad_grouped(const void* items, int n_items, int total_blocks, void* stream);

/* out[c] (+)= sum over the rows of a channels-last (rows, C) matrix of `dtype`: the bias gradient of nn.Conv1d (models.py:26, the decoder head) on
 * its own -- two launches, per-block partial rows in `workspace` (convasr_colsum_workspace_bytes) added in a fixed order: no atomics. */
int64_t convasr_colsum_workspace_bytes(int64_t rows, int C);
int convasr_colsum(const void* y, int dtype, int64_t rows, int C, float* out, void* workspace, int accumulate, void* stream);

/* dst[i] = src[i] * scale over n elements (n % 8 == 0), fp32 -> CONVASR_BF16 / CONVASR_F16 or back: the two ends of a 16-bit gradient
 * exchange (apex O2 keeps and all-reduces fp16 model gradients, models.py:744-762 / train.py:771): a bucket of the fp32 gradient arena is
 * packed into a 16-bit send buffer (scale = 1 / world size: the mean, formed before the sum so that fp16 cannot overflow in it),
 * all-reduced by RCCL at half the bytes, and unpacked into the arena. */
int convasr_cast_scale(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, float scale, void* stream);

/* ---- split-operand ("x3") convs: fp32-class accuracy on the 16-bit matrix pipe (models.py:47-77 computed as nn.Conv1d does in fp32) ---- */

/* A value v travels as hi = rn16(v), lo = rn16(v - hi) and a product as hi*hi + hi*lo + lo*hi: three 16-bit MFMAs, each exact in fp32,
 * fp32 accumulation (bf16 planes: 16 significant bits per operand; fp16 planes: 22, but fp16's range).  The three products ride in the
 * REDUCTION axis of the ordinary conv entry points above, so no conv kernel of its own exists:
 *   convasr_split3: x fp32 channels-last [rows = B * T][C] -> out [rows][3][C] of `dtype` (CONVASR_BF16 / CONVASR_F16), planes
 *     order 0 = (hi, lo, hi) for a conv INPUT, order 1 = (hi, hi, lo) for an OUTPUT GRADIENT.  C % 8 == 0.
 *   forward:  convasr_conv1d_fwd(x3 as a (B, T, 3 Cin) input, packed_fwd of convasr_pack_conv_weight_split3, y fp32, Cin -> 3 Cin);
 *   dgrad:    convasr_conv1d_fwd(dy3 as a (B, T, 3 Cout) input, packed_dgrad of the same call, dx fp32, the usual transposed geometry);
 *   wgrad:    convasr_conv1d_wgrad(x3 read as (B, 3 Tin, Cin), dy3 read as (B, 3 Tout, Cout), dil -> 3 dil, pad -> 3 pad): frame 3 t + p is
 *             plane p of frame t, so the reduction over frames pairs plane p of x with plane p of dy.
 * convasr_pack_conv_weight_split3: (Cout, Cin, K) fp32 parameter in layout w_layout ->
 *   packed_fwd   [K][cout_pad(Cout)][3 Cin] : row (k, co)         = (w_hi[co][.][k], w_hi[co][.][k], w_lo[co][.][k])
 *   packed_dgrad [K][cout_pad(Cin)][3 Cout] : row (K - 1 - k, ci) = (w_hi[.][ci][k], w_lo[.][ci][k], w_hi[.][ci][k])      (dgrad_planes = 3)
 *             or [K][cout_pad(Cin)][Cout]   : row (K - 1 - k, ci) =  w_hi[.][ci][k], the ordinary 16-bit dgrad operand    (dgrad_planes = 1)
 * either may be NULL; rows beyond Cout / Cin are not written (zero-fill once).
 *
 * Split forward, ONE-product backward (compute types 'bf16x3f' / 'f16x3f': the loss carries the split forward's fp32-class accuracy, the
 * gradients the 16-bit path's, as under the reference's apex O2, models.py:744-762; two thirds of the backward's MFMA work are gone):
 *   dy:    convasr_bn_act_bwd_apply_to_half -- the fp32 BN backward with dy rounded once to a dense 16-bit tensor [B * T][C];
 *   dgrad: convasr_conv1d_fwd(dy16, packed_dgrad with dgrad_planes = 1, dx fp32);
 *   wgrad: convasr_conv1d_wgrad_ld -- convasr_conv1d_wgrad (stride 1) over operands whose frames are x_ld / dy_ld elements apart: plane 0 (hi)
 *          of the forward's saved planes x3 read IN PLACE (x_ld = 3 Cin) against dy16.  16-bit storage, Cin % 128 == 0, Cout % 128 == 0,
 *          ld % 8 == 0; CONVASR_EUNSUPPORTED outside -- convasr_conv1d_wgrad_ld_supported answers beforehand (the host then copies the plane out and calls
 *          convasr_conv1d_wgrad). */
int convasr_split3(const float* x, void* out, int dtype, int64_t rows, int C, int order, void* stream);
/* The two fp32 streaming passes whose result is consumed by split convs only, with the split folded in (the separate convasr_split3 pass --
 * 4 bytes read + 6 written per element -- disappears):
 *   convasr_bn_act_fwd_split3:       convasr_bn_act_fwd on fp32 y, the result z stored as its planes z3 [B * T][3][C], order 0 (scale / shift
 *                                    present and a clamp-type activation, i.e. the training launches; else CONVASR_EUNSUPPORTED);
 *   convasr_bn_act_bwd_apply_split3: convasr_bn_act_bwd_apply on fp32 inputs, dy stored as its planes dy3 [B * T][3][C], order 1.
 * Arguments as in the plain entry points, with the plane type (CONVASR_BF16 / CONVASR_F16) in place of `dtype`; the values are the
 * plain pass's values split exactly as convasr_split3 splits them (bit-identical planes). */
int convasr_bn_act_fwd_split3(const void* y, void* z3, int plane_dtype, const float* scale, const float* shift,
                              int n_res, const void* const* res, const float* const* rscale, const float* const* rshift,
                              int act, float act_lo, float act_hi, float dropout_p, uint64_t seed, uint64_t offset, const uint64_t* step_key,
                              const float* xlen, int B, int T, int C, uint8_t* gate, void* stream);
int convasr_bn_act_bwd_apply_split3(const void* dz_or_g, const void* y, void* dy3, int plane_dtype, const float* coef, int from_dz,
                                    const float* scale, const float* shift, int act, float act_lo, float act_hi, float dropout_p,
                                    uint64_t seed, uint64_t offset, const uint64_t* step_key, const float* xlen, int B, int T, int C,
                                    const uint8_t* gate, void* stream);
int convasr_pack_conv_weight_split3(const float* w, int w_layout, void* packed_fwd, void* packed_dgrad, int dgrad_planes, int dtype, int Cout, int Cin, int K, void* stream);
int convasr_bn_act_bwd_apply_to_half(const void* dz_or_g, const void* y, void* dy16, int out_dtype, const float* coef, int from_dz,
                                     const float* scale, const float* shift, int act, float act_lo, float act_hi, float dropout_p,
                                     uint64_t seed, uint64_t offset, const uint64_t* step_key, const float* xlen, int B, int T, int C,
                                     const uint8_t* gate, void* stream);
/* 1 when convasr_conv1d_wgrad_ld takes this geometry, 0 when the caller must make the operands dense and call convasr_conv1d_wgrad (no launch). */
int convasr_conv1d_wgrad_ld_supported(int dtype, int B, int Cin, int Cout, int Tin, int Tout, int K, int dil, int x_ld, int dy_ld);
int convasr_conv1d_wgrad_ld(const void* x, int x_ld, const void* dy, int dy_ld, float* dw, void* workspace, int dtype,
                            int B, int Cin, int Cout, int Tin, int Tout, int K, int dil, int pad, int accumulate, int dw_layout, void* stream);

/* ---- per-step device state: what lets train.py:745-783 replay from a HIP graph ------------------------------------- */

/* state: four device words {dropout seed (the caller's, models.py:365-369 draws from torch's generator), steps begun, key of the
 * current step, reserved}.  Enqueues state[1] += 1; state[2] = mix(state[0] ^ mix(state[1])) -- one thread.  The training step calls it
 * first; &state[2] is the `step_key` of the dropout entry points above.  Eager and graph-replayed steps advance the same words. */
int convasr_step_begin(uint64_t* state, void* stream);
/* dst[0..nbytes) = src[0..nbytes), device to device, on `stream` (a memcpy node under capture): hands a double-buffered device state
 * (loss scaler, NovoGrad EMAs, AdamW step count) back to the buffer a captured graph reads. */
int convasr_copy(const void* src, void* dst, int64_t nbytes, void* stream);

/* ---- weight averaging: an exponential moving average of the parameter arena (train.WeightEMA) ------------------------ */

/* One streaming pass over n fp32 elements (n a multiple of 8; w, e and e16 16-byte aligned; w != e), in this order of operations:
 *   k = k_in[0]                                 the number of updates APPLIED so far (a device float, saturating at 2^24)
 *   d = min(decay, (1 + k) / (10 + k))          fp32: each sum and the quotient correctly rounded;  omd = 1 - d, rounded
 *   e[i] = k == 0 ? w[i] : fma(omd, w[i] - e[i], e[i])      i.e. e + (1 - d) (w - e): the difference is rounded, then one fused multiply-add
 *   e16[i] = e[i] rounded to nearest-even in e16_dtype (CONVASR_BF16 / CONVASR_F16), when e16 != NULL
 *   k_out[0] = min(k + 1, 2^24)
 * k_in / k_out: one device float each, distinct buffers the caller swaps per call (every workgroup reads k while one thread writes the
 * next value), as convasr_adamw_step's step_in / step_out.  decay in [0, 1].
 * Skip rule -- the one of the three fused optimizer steps, which return early on `gated || overflow`: when loss_gate != NULL and
 * *loss_gate is inf or NaN, or when scaler_state != NULL and scaler_state[2] (the loss scaler's "did the last step overflow") is not 0,
 * the call writes k_out[0] = k_in[0] and nothing else.  Called after an optimizer step with that step's loss_gate and the scaler state
 * that step WROTE (its scaler_out), it skips exactly when the step did: the step records its overflow verdict there unless it was gated,
 * and a gated step is caught by loss_gate itself.  No atomics, one kernel node under capture. */
int convasr_ema_update(const float* w, float* e, void* e16, int e16_dtype, int64_t n, float decay, const float* k_in, float* k_out,
                       const float* loss_gate, const float* scaler_state, void* stream);
/* elements one workgroup of convasr_ema_update covers per grid pass, and the largest grid it launches (larger arenas loop) */
int64_t convasr_ema_update_span(void);
int64_t convasr_ema_update_max_blocks(void);
/* Exchanges the contents of a[0..nbytes) and b[0..nbytes) in place (device buffers, 16-byte aligned, nbytes a multiple of 16, not
 * overlapping): one kernel, every lane reads and writes its own 16 bytes of both.  The addresses stay what they were -- captured step
 * graphs and packed weight copies that are keyed by the arena's address stay valid. */
int convasr_swap(void* a, void* b, int64_t nbytes, void* stream);
/* bytes one workgroup of convasr_swap covers per grid pass */
int64_t convasr_swap_span_bytes(void);

/* ---- SURVEY 8(f) "next" rows ------------------------------------------------------------------------------------ */

/* NovoGrad.step (optimizers.py:66-90) with torch.nn.utils.clip_grad_norm_ (train.py:777) folded in, over a flat arena of n
 * fp32 values cut into n_seg tensors by offsets[n_seg + 1] (device int64; a tensor's padding belongs to it and must hold
 * zero gradients).  Per tensor s: g2 = sum (c*g)^2 with c = min(1, max_norm / (||g||_all + 1e-6)) (c = 1 if max_norm <= 0);
 * ema_out[s] = first ? g2 : ema_in[s]*beta2 + g2*(1-beta2); d = c*g / sqrt(ema_out[s] + eps) (+ wd*p) (* (1-beta1) if
 * dampening); mom = first ? d : mom*beta1 + d; p -= lr*mom.  ema_in / ema_out must be different buffers (the caller swaps
 * them every call); g2 is n_seg doubles of scratch; the per-tensor sums of squares are formed without atomics from a static work table:
 * items[n_items][3] = {tensor, begin, end} cuts every tensor into pieces of at most convasr_novograd_item_elems() elements, in tensor
 * order, seg_first[n_seg + 1] indexes the first piece of each tensor, item_part is n_items doubles of scratch (device int64 / fp64); total_norm (may be NULL) receives ||g||_all; loss_gate and grad_scale as in
 * convasr_sgd_step (a gated call copies ema_in to ema_out and changes nothing else).  first: 1 / 0 decided by the caller, or -1 =
 * decided on the device: ema_in / ema_out then hold n_seg + 1 floats, the last one the number of steps applied so far (the call
 * writes ema_out[n_seg] = ema_in[n_seg] + 1 unless gated), and first = (ema_in[n_seg] == 0) -- a gated first iteration then leaves
 * no optimizer state behind, like the reference, which creates state only when a step runs (optimizers.py:76-80).  p16 / p16_dtype and
 * scaler_in / scaler_out as in convasr_sgd_step (the overflow check uses the per-tensor sums of squares formed here). */
int convasr_novograd_step(float* p, const float* g, float* mom, const float* ema_in, float* ema_out, double* g2, const int64_t* offsets,
                          int n_seg, int64_t n, const int64_t* items, int n_items, const int64_t* seg_first, double* item_part,
                          float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, int dampening, int first,
                          const float* loss_gate, float* total_norm, float grad_scale, void* p16, int p16_dtype, const float* scaler_in,
                          float* scaler_out, const float* lr_dev, void* stream);
/* largest item the table may hold (elements) */
int64_t convasr_novograd_item_elems(void);

/* Bytes of back-pointer workspace for the call below (ABI v8: S_max added -- targets longer than 511 labels run one workgroup per
 * utterance instead of one wave and keep 1024 packed words per frame instead of 64). */
int64_t convasr_ctc_alignment_workspace_bytes(int B, int T, int S_max);
/* ctc.alignment (ctc.py:7-75): forced alignment of targets[b, :target_lengths[b]] to log_probs[b, :input_lengths[b]]
 * (log_probs batch-major (B, T, C) fp32; the reference's (T, B, C) tensor permuted).  alignment (B, S_max) int64: the last
 * frame the best path spends in each label's state, 0 for padded labels.  Forward variable = the reference's sum recursion
 * with finfo.min as log-zero over all T frames, back-pointer = first maximum of (stay, s-1, s-2), end state chosen from the
 * column at T-1, walk started at input_lengths[b]-1.  S_max <= 8191 (a recording of ten minutes aligned to its transcript in one call,
 * transcribe.py:176 without segmentation); longer targets return CONVASR_EUNSUPPORTED here: convasr_ctc_alignment_long below takes them. */
int convasr_ctc_alignment(const float* log_probs, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths,
                          int64_t* alignment, void* workspace, int B, int T, int C, int S_max, int blank, void* stream);

/* The same alignment -- arguments, quirks and result, bit for bit -- for whole recordings, at every target length: the lattice is cut
 * into tiles of convasr_ctc_alignment_long_states_per_block() states x chunk frames, one wave per tile, one plain launch per
 * anti-diagonal of tiles (ceil(T / chunk) + ceil((2 S_max + 1) / states_per_block) - 1 launches at most; tiles in which no state can be
 * reached yet, s > 2t + 1, are not launched), then one launch that walks the path back through windows of back-pointers staged in LDS.
 * Nothing waits inside a launch.  chunk_frames: 0 = convasr_ctc_alignment_long_chunk_frames() (256), or 16 .. 4096 to force the chunk
 * length (tests and tuning; the result does not depend on it).  workspace: at least convasr_ctc_alignment_long_workspace_bytes bytes,
 * 16-byte aligned, uninitialised: back-pointers [B][T][ceil((2 S_max + 1) / 16)] dwords (2 bits per state), the column carried between
 * chunks [B][blocks][states_per_block] fp32 and the two last states of every block at every frame [B][blocks][T][2] fp32 -- an hour
 * (180,000 frames, 48,000 labels) takes about 4.9 GB.  Envelope: 1 <= S_max <= 131071, 1 <= T <= 2^20, 1 <= B <= 65535; outside it
 * CONVASR_EUNSUPPORTED (the query returns -1); any other bad argument CONVASR_EINVAL. */
int convasr_ctc_alignment_long_states_per_block(void);
int convasr_ctc_alignment_long_chunk_frames(void);
int64_t convasr_ctc_alignment_long_workspace_bytes(int B, int T, int S_max);
int convasr_ctc_alignment_long(const float* log_probs, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths,
                               int64_t* alignment, void* workspace, int64_t workspace_bytes, int B, int T, int C, int S_max, int blank,
                               int chunk_frames, void* stream);
/* The same in parts, for measurements that time the two apart: parts = 1 the sweep, 2 the walk over a workspace that a sweep with the same
 * arguments filled, 3 both (= the call above). */
int convasr_ctc_alignment_long_parts(const float* log_probs, const int64_t* targets, const int64_t* input_lengths, const int64_t* target_lengths,
                                     int64_t* alignment, void* workspace, int64_t workspace_bytes, int B, int T, int C, int S_max, int blank,
                                     int chunk_frames, int parts, void* stream);

/* The padding half of AudioTextDataset.collate_fn (datasets.py:320-330) on the device: B ragged samples of `rows` rows each,
 * delivered as one packed buffer (sample b starts at element offsets[b], its rows are lengths[b] long and contiguous), become the
 * zero-padded batch out (B, rows, Tpad).  elem_bytes: 2 (int16 / bf16), 4 (fp32 / int32) or 8 (int64 targets). */
int convasr_collate_pad(const void* packed, const int64_t* offsets, const int64_t* lengths, void* out, int elem_bytes, int B, int rows,
                        int64_t Tpad, void* stream);

/* ---- CTC prefix beam search without a language model: decoders.py:19-55 (BeamSearchDecoder, ctcdecode.CTCBeamDecoder with
 * lm_path = None), train.py:975-995 / transcribe.py:323-327 (--decoder BeamSearchDecoder, --beam-width, --decoder-topk) ---------- */

/* Bytes of workspace convasr_ctc_beam_search needs (the prefix-node arena: B * T * W nodes of 8 bytes); a negative CONVASR_E* code
 * with a message when the arguments are outside the envelope below. */
int64_t convasr_ctc_beam_search_workspace_bytes(int B, int T, int C, int W, int N, int topk);
/* log_probs: fp32, element (b, c, t) at ((b * T + t) * C + c); lengths (B,) int64, frames t < lengths[b] are decoded (clamped to
 * [0, T]).  One workgroup per utterance, the frame loop inside the kernel; the workspace needs no initialisation and the call has no
 * memset, copy or host synchronisation, so it can be captured into a graph.  Per frame t:
 *   P_t = the classes sorted by lp[t] descending (ties: lower index), the first N; cutoff_prob < 1 keeps the shortest leading run whose
 *   cumulative probability reaches cutoff_prob (at least one class).  For every beam l (lpb / lpnb: log-probability that it ends
 *   in blank / non-blank; the search starts from the empty prefix, lpb = 0, lpnb = -inf) and c in P_t, with logaddexp as the sum:
 *   c == blank: nb(l) += lp + lpb(l) + lpnb(l); c == last(l): nnb(l) += lp + lpnb(l), nnb(l + c) += lp + lpb(l); otherwise
 *   nnb(l + c) += lp + lpb(l) + lpnb(l).  An extension equal to a beam already held is folded into that beam's candidate; a candidate
 *   that got no contribution or whose total is -inf is dropped.  The best W candidates by lpb + lpnb survive, ties broken by
 *   ascending key (rank of the source beam, -1) for a beam's own candidate and (rank of i, c) for an unmerged extension of beam i
 *   by c; that order is the next frame's ranking.  Beam scores are kept in fp64.
 * Outputs, best hypothesis first: tokens (B, topk, T) int64 and offsets (B, topk, T) int32 (the frame at which each token was appended
 * by the extension that created it; 0 past a hypothesis' length), out_lengths (B, topk) int64, log_prob (B, topk) fp32 = lpb + lpnb
 * (the MOST probable hypotheses; a slot the search could not fill has length 0 and -inf).  lengths[b] = 0: one empty hypothesis, 0.
 * Envelope, checked before any launch: 1 <= W <= 1024, 1 <= N <= min(C, 128), 1 <= topk <= W, 2 <= C <= 8192, 0 <= blank < C,
 * 0 < cutoff_prob <= 1, B * T * W < 2^31; outside it CONVASR_EINVAL / CONVASR_EUNSUPPORTED (the reference's default
 * --beam-width 5000 among them: convasr_ctc_beam_search_wide below takes it). */
int convasr_ctc_beam_search(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                            float* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                            void* stream);

/* ---- CTC prefix beam search with an n-gram language model: decoders.py:19-55 (BeamSearchDecoder, ctcdecode.CTCBeamDecoder with a KenLM
 * Scorer), train.py:975-995 / transcribe.py:323-328 (--lm, --beam-alpha, --beam-beta).  The model comes from an ARPA text file; the
 * tables are built on the host by convasr_amd/lm.py (NgramLM, which documents their layout) and the C side keeps no state.
 * Everything not stated here is as in convasr_ctc_beam_search above: candidate rules, merging, tie keys, top-N / cutoff_prob, fp64
 * scores, the output layout (log_prob is fp64 here).  The rules, modelled on ctcdecode's Scorer and PathTrie:
 *   labels: one character per class, lowercased; the space class s is the one labelled ' ' (exactly one; s != blank).
 *   ARPA: \data\ counts, \N-grams: sections, \end\; each entry log10 p, the n-gram, an optional log10 backoff weight (missing: 0);
 *   order 1 <= N_lm <= 6.  An n-gram whose context (first N - 1 words) is not listed is refused (lm.py raises ValueError).
 *   V: the unigrams other than <s>, </s>, <unk> whose characters all map to labels other than the blank and s.  Empty V: ValueError;
 *   every word of V one character (ctcdecode's character-LM mode): NotImplementedError.
 *   log10 P(w | h): the listed probability of (h, w) when the model lists it, otherwise bow(h) + log10 P(w | h[1:]) (bow = 0 when h is
 *   not listed).  The context of a word = the words completed before it in the prefix, truncated to N_lm - 1; with fewer, one <s> in
 *   front.  LM term = alpha * ln P(w | ctx) + beta, ln = log10 * ln 10.
 *   cw(l) = the label characters after the last space of l.
 *   Dictionary constraint: an extension l + c (c not blank / s; c != last(l), or c == last(l) from lpb(l)) exists only if cw(l) + labels[c]
 *   is a prefix of a word in V; l + s exists only if cw(l) is non-empty and in V (no leading space, no two spaces in a row).
 *   Fusion: every contribution to nnb(l + s) -- from lpb(l), from lpnb(l), and an extension folded into a beam already held -- gets
 *   the LM term of cw(l) added (the stay nnb(l) += lp + lpnb(l) of a beam ending in s does not); selection ranks by lpb + lpnb as before.
 *   End of utterance: the hypotheses are ranked by lpb + lpnb + F(l) (ties: rank), F = 0 for an empty l or one ending in s, the LM term
 *   of cw(l) when cw(l) is in V, alpha * -1000 + beta otherwise (ctcdecode's OOV_SCORE, unconverted); log_prob returns that score.
 *   alpha = beta = 0 still applies the dictionary constraint: it is NOT the LM-free search.
 *   A frame that leaves no candidate (no allowed class and no blank among P_t) ends the search without a hypothesis: every slot of the
 *   utterance has length 0 and log_prob -inf.
 * Known divergences from ctcdecode (not compared against ctcdecode itself, which was not available):
 *   - no min_cutoff early exit: selection stays the exact top W;
 *   - scores are the fused log p, not ctcdecode's "approximate CTC" score with the LM removed and negated;
 *   - no </s> term at the end of the utterance.
 * Envelope, checked before any launch: that of convasr_ctc_beam_search, plus C <= 256, 1 <= order <= 6, s in [0, C) and s != blank,
 * finite alpha and beta, n_nodes >= 1, n_ent >= 1, n_slots a power of two, -1 <= start_state < n_ent, and the beam state within
 * 160 KiB of LDS: W = 1024 fits for every C <= 256 at N <= 64 and for C <= 160 at N = 128; at C = 256, N = 128 it would need 166,992
 * bytes and the largest W is 1001.  Outside the envelope CONVASR_EINVAL / CONVASR_EUNSUPPORTED. */
int64_t convasr_ctc_beam_search_lm_workspace_bytes(int B, int T, int C, int W, int N, int topk);
int convasr_ctc_beam_search_lm(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                               double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                               const uint32_t* node_mask, const int32_t* node_child, const int32_t* node_word, int n_nodes,
                               const double* ent_pb, const int32_t* ent_sl, int n_ent, const int32_t* slots, int n_slots,
                               int space, int order, int start_state, double alpha, double beta, void* stream);

/* ---- The wide CTC prefix beam search: beam widths up to 8192 (the reference transcribe.py's default --beam-width 5000) ---------------
 * convasr_ctc_beam_search_wide and convasr_ctc_beam_search_lm_wide take the arguments of convasr_ctc_beam_search and
 * convasr_ctc_beam_search_lm and compute the same search, word for word: candidates, merging, tie keys, top-N / cutoff_prob, fp64 scores,
 * the LM rules and the output layout.  At a width both forms accept they return the same bits.  They keep the beam state in the workspace
 * instead of LDS; as before the workspace needs no initialisation and the call can be captured into a graph.  Only these differ:
 *   Envelope, checked before any launch: 1 <= W <= 8192, 1 <= N <= min(C, 128), 1 <= topk <= W, 2 <= C <= 8192, 0 <= blank < C,
 *   0 < cutoff_prob <= 1, B * T * W < 2^31, B * topk * T < 2^31; for the LM form also everything convasr_ctc_beam_search_lm checks except
 *   its LDS budget (C <= 256 stays).  LDS use stays within 160 KiB over the whole envelope (117,328 bytes at W = C = 8192).  Outside it
 *   CONVASR_EINVAL / CONVASR_EUNSUPPORTED.
 *   Workspace bytes: up256(8 * B * T * W) + B * S, up_k(x) = x rounded up to a multiple of k, with
 *     A = up16(52 * W) (LM form: up16(68 * W + 4 * W * MW), MW = ceil(C / 32)),
 *     S = up256(2 * A + 24 * W + 4 * W * NW + 4 * TB), NW = ceil(N / 32), TB = the smallest power of two >= max(2 * W, 64):
 *   the prefix-node arena, then per utterance two copies of the beam state and the per-frame candidate state and hash table. */
int64_t convasr_ctc_beam_search_wide_workspace_bytes(int B, int T, int C, int W, int N, int topk);
int convasr_ctc_beam_search_wide(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                 float* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                                 void* stream);
int64_t convasr_ctc_beam_search_lm_wide_workspace_bytes(int B, int T, int C, int W, int N, int topk);
int convasr_ctc_beam_search_lm_wide(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                    double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                                    const uint32_t* node_mask, const int32_t* node_child, const int32_t* node_word, int n_nodes,
                                    const double* ent_pb, const int32_t* ent_sl, int n_ent, const int32_t* slots, int n_slots,
                                    int space, int order, int start_state, double alpha, double beta, void* stream);

/* ---- CTC prefix beam search biased towards hot phrases (contextual biasing; this package's own, the reference has none) ---------------
 * convasr_ctc_beam_search_hot / _lm_hot and their _wide forms are the four searches above with one more term in the score.  Everything
 * not stated here is as above: candidates, merging, tie keys, top-N / cutoff_prob, fp64 scores, the LM rules, the output layout, the
 * workspace (no initialisation) and graph capture (the tables are uploaded before the call).  The tables are built on the host by
 * convasr_amd/hotwords.py (HotWords, which documents their layout); the C side keeps no state.
 *   Labels: as for the LM: one lowercased character per class, exactly one space class s, s != blank, C <= 256.
 *   Phrases: lowercased, stripped, inner whitespace runs reduced to one space; a non-empty sequence of classes, none the blank, that
 *   neither begins nor ends with s.
 *   Trie: all phrases form one trie.  Node 0 is the root; a node is terminal when a phrase ends there; the children of a node are stored
 *   contiguously in class order; hot_mask (n_nodes, MW) has bit c of node u set when u has a child by class c, MW = ceil(C / 32);
 *   hot_child (n_nodes,) is the index of u's first child, so child(u, c) = hot_child[u] + (set bits of u's mask below c); hot_term
 *   (n_nodes,) is 1 for a terminal node.
 *   Weight: one w >= 0, a double, in natural-log units per matched label.
 *   State: every prefix l has a hot state (u, k): u a trie node or DEAD, k the number of labels matched since the last completed phrase
 *   (the pending count).  The empty prefix has (root, 0).
 *   Creating l + c (an extension, not the stay of a repeated last token):
 *     match: u != DEAD and v = child(u, c) exists: delta = +w; the new state is (v, 0) if v is terminal, else (v, k + 1).
 *     mismatch at a word start: no such child, last(l) == s and v = child(root, c) exists: delta = -(w * k) + w; the new state is (v, 0)
 *     if v is terminal, else (v, 1).
 *     mismatch: anything else: delta = -(w * k); the new state is (root, 0) if c == s, else (DEAD, 0).
 *   So a match can start only at the beginning of the utterance or right after a space; a completed phrase keeps its bonus and a partial
 *   match gives all of it back; there are no failure links; the state is a function of the prefix's labels alone, so merged prefixes
 *   agree on it.
 *   Fusion: delta(l, c) is added to every contribution to nnb(l + c): the candidate extension's score, and the fold of l_i + last(l_j)
 *   into a held beam l_j.  The fp64 operations, in this order: ((lp + base) + the LM term if any) + delta, with -(w * k) formed as one
 *   multiply and one negation (no fused multiply-add).
 *   End of utterance: the ranking score is lpb + lpnb (+ the LM's F(l)) + F_hot(l), F_hot = -(w * k(l)); the beams are re-ranked by it
 *   (ties: rank) and log_prob returns it, fp64 on all four entry points.
 *   With an LM its dictionary constraint still decides which extensions exist; the hot rule only adds to scores.  Every word of every
 *   phrase must be in V (hotwords.py raises ValueError naming the others).
 *   w = 0 or a trie of the root alone: the search above.  Tokens, offsets and lengths are identical; with an LM the scores are identical
 *   bit for bit, without one log_prob is the fp64 value that convasr_ctc_beam_search rounds to fp32.
 * Arguments after those of the search above: hot_mask, hot_child, hot_term, n_hot_nodes, hot_mask_words (= MW, checked against C), for the
 * LM-free forms the space class s (the LM forms use the LM's), and w.
 * Envelope, checked before any launch: that of the search above, plus C <= 256, n_hot_nodes >= 1, hot_mask_words == ceil(C / 32), s in
 * [0, C) and s != blank, w finite and >= 0.  A child index outside [0, n_hot_nodes) makes the state DEAD and no walk over the tables loops,
 * so tables that break the builder's invariants give wrong words, not a fault.  The LDS forms keep 8 + 4 * MW more bytes per beam (and MW
 * words for the root's mask) and stay within 160 KiB: without an LM W = 1024 fits for every C <= 256 and N <= 128; with an LM W = 1024 fits
 * for C <= 96 (C = 38 among them) at N <= 64, and the largest W is 1003 at C = 128 (N <= 64), 948 at C = 160 (N <= 64), 814 at C = 256
 * (N <= 64) and 778 at C = 256, N = 128.  A width the LDS form refuses runs in the wide form (W <= 8192), whose workspace per utterance
 * has A = up16(60 * W + 4 * W * MW) without an LM and up16(76 * W + 8 * W * MW) with one.  Outside the envelope CONVASR_EINVAL /
 * CONVASR_EUNSUPPORTED. */
int64_t convasr_ctc_beam_search_hot_workspace_bytes(int B, int T, int C, int W, int N, int topk);
int convasr_ctc_beam_search_hot(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                                const uint32_t* hot_mask, const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes, int hot_mask_words,
                                int space, double weight, void* stream);
int64_t convasr_ctc_beam_search_hot_wide_workspace_bytes(int B, int T, int C, int W, int N, int topk);
int convasr_ctc_beam_search_hot_wide(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                     double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                                     const uint32_t* hot_mask, const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes,
                                     int hot_mask_words, int space, double weight, void* stream);
int64_t convasr_ctc_beam_search_lm_hot_workspace_bytes(int B, int T, int C, int W, int N, int topk);
int convasr_ctc_beam_search_lm_hot(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                   double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob, int topk,
                                   const uint32_t* node_mask, const int32_t* node_child, const int32_t* node_word, int n_nodes,
                                   const double* ent_pb, const int32_t* ent_sl, int n_ent, const int32_t* slots, int n_slots,
                                   int space, int order, int start_state, double alpha, double beta, const uint32_t* hot_mask,
                                   const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes, int hot_mask_words, double weight,
                                   void* stream);
int64_t convasr_ctc_beam_search_lm_hot_wide_workspace_bytes(int B, int T, int C, int W, int N, int topk);
int convasr_ctc_beam_search_lm_hot_wide(const float* log_probs, const int64_t* lengths, int64_t* tokens, int32_t* offsets, int64_t* out_lengths,
                                        double* log_prob, void* workspace, int B, int T, int C, int blank, int W, int N, float cutoff_prob,
                                        int topk, const uint32_t* node_mask, const int32_t* node_child, const int32_t* node_word, int n_nodes,
                                        const double* ent_pb, const int32_t* ent_sl, int n_ent, const int32_t* slots, int n_slots,
                                        int space, int order, int start_state, double alpha, double beta, const uint32_t* hot_mask,
                                        const int32_t* hot_child, const int32_t* hot_term, int n_hot_nodes, int hot_mask_words, double weight,
                                        void* stream);

/* ---- Validation metrics: metrics.py:409-421 (cer / wer, the edit distances train.py:evaluate_model scores every validation utterance
 * with), transcript_generators.py:8-93 (the greedy collapse of GreedyCTCGenerator.generate) -------------------------------------------- */

enum { CONVASR_METRIC_CHARS = 0, CONVASR_METRIC_WORDS = 1 };
#define CONVASR_METRIC_MAX_LEN 16383

/* Levenshtein distances of B x K hypotheses against B references, one launch.
 * hyp (B, K, Lh) int64, contiguous; hyp_lengths (B, K) int64.  Reference b is ref[b * ref_stride + t], its length
 * ref_lengths[b * ref_lengths_stride] (so y[:, 0] / ylen[:, 0] of a (B, n_targets, Lpad) batch are read in place).  Only tokens below each
 * length are read; the lengths are clamped to [0, Lh] / [0, Lr] on the device.
 * Units, with `space` a token id:
 *   CONVASR_METRIC_CHARS: the tokens that are not `space` (str.replace(' ', '') over tokens); space < 0: every token is a unit.
 *   CONVASR_METRIC_WORDS: the maximal runs of tokens that are not `space` (str.split() over tokens): leading, trailing and repeated spaces
 *   make no empty words.  Two words are equal exactly when they have the same length and the same tokens (compared in full, never by hash).
 * distance (B, K) int32 = the exact Levenshtein distance between the two unit sequences (unit cost for an insertion, a deletion and a
 * substitution); ref_units (B,) int32 = the number of units of reference b (not clamped to 1).
 * One 64-thread workgroup per pair; no workspace, no initialised memory, no memset or copy: the call can be captured into a graph.
 * Envelope, checked before any launch: B >= 1, K >= 1, B * K < 2^20, 0 <= Lh, Lr <= CONVASR_METRIC_MAX_LEN, strides >= 0, a valid mode,
 * space >= 0 in WORDS mode, no NULL pointer; outside it CONVASR_EINVAL. */
int convasr_edit_distance(const int64_t* hyp, const int64_t* hyp_lengths, const int64_t* ref, int64_t ref_stride,
                          const int64_t* ref_lengths, int64_t ref_lengths_stride, int32_t* distance, int32_t* ref_units, int B, int K,
                          int Lh, int Lr, int mode, int64_t space, void* stream);

/* The greedy CTC collapse of GreedyCTCGenerator.generate with time_stamps = None and a tokenizer whose silence tokens are {eps, space}
 * and whose word-start token is space (CharTokenizerLegacy).  path (B, T) int64: the per-frame argmax (convasr_argmax); frames
 * t < lengths[b] are read (clamped to [0, T]).  Per utterance, with `last` = eps, blanks = 0, repeat_ok = false:
 *   frames before the first one that is neither eps nor space are skipped (when there is none, nothing is emitted);
 *   then per frame c: c == eps: if last == space nothing happens; otherwise repeat_ok = true, ++blanks, and when
 *   blanks >= blank_amount_to_space, space is emitted.  c != eps: if c == last and not repeat_ok nothing happens; otherwise c is
 *   emitted, repeat_ok = false, blanks = 0.  `last` is the token emitted last (blanks is not reset by a suppressed repeat; a space
 *   can be emitted twice in a row or at the end).
 * tokens (B, T) int64 = the emitted tokens, 0 past out_lengths[b]; out_lengths (B,) int64.  One workgroup per utterance; no workspace,
 * no memset or copy: the call can be captured into a graph.  Envelope, checked before any launch: B >= 1, T >= 1, B * T < 2^31,
 * eps != space, both >= 0, blank_amount_to_space >= 0, no NULL pointer; outside it CONVASR_EINVAL. */
int convasr_ctc_greedy_collapse(const int64_t* path, const int64_t* lengths, int64_t* tokens, int64_t* out_lengths, int B, int T,
                                int eps, int space, int blank_amount_to_space, void* stream);

/* The greedy CTC decode of GreedyCTCGenerator.generate WITH the frame of every token and the word segments, for a tokenizer whose silence
 * tokens are {eps, space} and whose word-start token is space (CharTokenizerLegacy).  path (B, T) int64: the per-frame argmax
 * (convasr_argmax); lengths (B,) int64.  The host loop (GreedyCTCGenerator.generate_host) is the oracle; this is the same rule in a form
 * that decides every frame on its own.  Per utterance, with n = clamp(lengths[b], 0, T) and gap = max(blank_amount_to_space, 1):
 *   start = the first frame in [0, n) whose class is neither eps nor space; when there is none the utterance yields nothing (a non-silent
 *   frame at or after n does not count).
 *   A non-blank frame t in [start, n) (class != eps), with p = the previous non-blank frame >= start and g = t - p - 1 blanks between them:
 *     frame `start` always emits its class; if path[p] == space, t emits iff path[t] != space; otherwise t emits iff g >= 1 or
 *     path[t] != path[p].
 *   A blank frame t in (start, n) emits one INSERTED space iff path[p] != space and t - p == gap -- also in a blank run that reaches n.
 *     (A space frame of the path after an inserted space is emitted again: g >= 1.)
 *   Segments, split_words != 0 (time stamps given): the first emission opens segment 0; every space emitted from the path opens a new
 *     segment and is stored TWICE at its front (the host loop's tokens = [eps, c]; tokens.append(c)), both with its frame; an inserted space
 *     opens nothing.  A segment's begin frame is the frame of its first emission, its end frame the frame of its last emission that came
 *     from the path (inserted spaces do not move it).  split_words == 0: one segment per non-empty utterance, from `start` to the last
 *     path emission, and no token is doubled.
 * Outputs, packed over the batch in utterance order: tokens int64 / frames int32, room for B * T * (split_words ? 2 : 1) entries each;
 * counts (2, B) int64 = tokens per utterance, then segments per utterance; seg_first int64 (the segment's first token, an index into the
 * packed tokens), seg_begin / seg_end int32 (frames inside the utterance), room for B * T entries each.  Nothing past the counts is written.
 * Utterances are cut into chunks of convasr_ctc_greedy_segments_chunk_frames() frames, one workgroup per (utterance, chunk); five plain
 * launches in stream order (chunk summaries, their carry, counts, offsets, writes), no workgroup waits on another, no memset or copy: the
 * call can be captured into a graph.  workspace: convasr_ctc_greedy_segments_workspace_bytes(B, T) bytes (-1 outside the envelope),
 * uninitialised.  Envelope, checked before any launch: B >= 1, T >= 1, B * T < 2^31, eps != space, both >= 0,
 * blank_amount_to_space >= 0, no NULL pointer, a workspace of at least that size; outside it CONVASR_EINVAL. */
int convasr_ctc_greedy_segments_chunk_frames(void);
int64_t convasr_ctc_greedy_segments_workspace_bytes(int B, int T);
int convasr_ctc_greedy_segments(const int64_t* path, const int64_t* lengths, int64_t* tokens, int32_t* frames, int64_t* counts,
                                int64_t* seg_first, int32_t* seg_begin, int32_t* seg_end, void* workspace, int64_t workspace_bytes, int B, int T,
                                int eps, int space, int blank_amount_to_space, int split_words, void* stream);

/* ---- Uncertainty: how sure the model is of a frame and of a word (models.py:645-678 entropy / weighted_mean_entropy / margin in their
 * per-frame forms, the per-frame curves of vis.py:365-369, 382) --------------------------------------------------------------------------- */

/* Per-frame statistics of channels-last fp32 log-probs (B, T, C) in ONE read.  lengths (B,) int64 may be NULL (all T frames); n_b =
 * clamp(lengths[b], 0, T).  Every output is (B, T) and any output pointer may be NULL.
 *   idx int64: the index convasr_argmax gives, under the same total order on (value, index) pairs: NaN ranks above every number, two NaNs
 *     are equal, among equals the lower index wins.  Written for EVERY frame, also t >= n_b: bit for bit convasr_argmax's output.
 * For a frame t < n_b, in fp32:
 *   p1 = expf(lp[idx]);  p2 = expf(the largest value among the classes c != idx, same order);  margin = p1 - p2 (models.margin: the
 *     difference of the two largest probabilities; an exact tie gives exactly 0).
 *   entropy = -sum_c expf(lp[c]) * lp[c], the product written out as in the reference: a class at -inf gives NaN (0 * inf), as
 *     convasr_entropy and torch do.
 *   p_eps = expf(lp[eps_id]).
 *   entropy_nb = the entropy of log_softmax over the classes c != eps_id (vis.py:367-368), from a max-subtracted log-sum-exp of its own:
 *     with m = max_{c != eps_id} lp[c], d_c = lp[c] - m, S = sum expf(d_c), A = sum expf(d_c) * d_c:  entropy_nb = logf(S) - A / S.
 *     (Not derived from entropy and p_eps: that form cancels when p_eps -> 1.)  Exactly 0 when C == 2; NaN when such a class is at -inf.
 *   A frame that holds a NaN has all five float outputs NaN.
 * For a frame t >= n_b the five float outputs are 0 (the reference's temporal_mask multiply, as a select: nothing past the length shows).
 * Sums run in a fixed order: C <= convasr_frame_uncertainty_row_classes() in class order, one thread per frame; above it per-lane partial
 * sums over c = lane, lane + 64, ... and a xor butterfly over the 64 lanes, one wave per frame.  Two runs are bit-equal.
 * One launch, no workspace, no memset or copy: the call can be captured into a graph.  Envelope, checked before any launch: B >= 1,
 * T >= 1, B * T < 2^31, 2 <= C <= CONVASR_UNCERTAINTY_MAX_CLASSES, 0 <= eps_id < C, log_probs not NULL; outside it CONVASR_EINVAL. */
#define CONVASR_UNCERTAINTY_MAX_CLASSES 8192
int convasr_frame_uncertainty_row_classes(void);
int convasr_frame_uncertainty(const float* log_probs, const int64_t* lengths, int64_t* idx, float* p1, float* margin, float* entropy,
                              float* entropy_nb, float* p_eps, int B, int T, int C, int eps_id, void* stream);

/* Statistics of N spans (words) over the per-frame arrays above.  Span k lies in utterance utt[k] (int64) and covers the positions
 * [begin[k], end[k]] (int32, inclusive) of a grid of Tp positions per utterance.  frame_map NULL: Tp == T and position p IS frame p.
 * frame_map (B, Tp) int64 given: position p of utterance b stands for frame frame_map[b, p] of the (B, T) arrays (a forced alignment: the
 * positions are those of a transcript); the span then covers the frames [frame_map[begin], max(frame_map[begin], frame_map[end])].
 * Events (optional; first, tokens and frames come together): span k owns the events j in [first[k], first[k + 1]) of n_events packed
 * pairs (tokens[j] int64, frames[j] int32 = a position); first has N + 1 entries.  Event j COUNTS unless
 *   (a) path (B, Tp) int64 is given and path[utt, frames[j]] != tokens[j]: an inserted space of the greedy rule, which its frame does not
 *       assert; or
 *   (b) j > first[k] and event j equals event j - 1 in token and position: the word-start space convasr_ctc_greedy_segments stores twice.
 * Both are decided on the positions, before the map.  With f_j the frame of event j, l_j = log_probs[utt, f_j, tokens[j]] over the n events
 * that count:
 *   n_events_out int32 = n
 *   confidence     = expf((sum_j l_j) / n)          the geometric mean of the tokens' probabilities
 *   confidence_min = expf(min_j l_j)
 *   margin         = min_j m_j,  m_j = margin[utt, f_j] when tokens[j] == idx[utt, f_j], else expf(l_j) - p1[utt, f_j]  (<= 0)
 *   entropy        = the mean of entropy[utt, t] over the span's frames
 *   uncertainty    = sum_t entropy_t (1 - p_eps_t) / (eps + sum_t (1 - p_eps_t)) over the span's frames: weighted_mean_entropy
 *                    (models.py:660-674) of the word alone
 * n == 0: confidence, confidence_min and margin are 0.  Without events only entropy and uncertainty are written (the other four output
 * pointers and log_probs, idx, p1, margin may be NULL).  A NaN among the l_j or m_j makes the minimum NaN.
 * Sums are taken in fp64 and rounded to fp32 once: thread i of the span's 256-thread workgroup adds frames begin + i, begin + i + 256, ...
 * (events likewise), then a xor butterfly per wave, then the four waves in order.  The order depends on the span alone: a span's outputs do
 * not change with N, with the other spans or with their order, and two runs are bit-equal.  A span may be one frame or a whole recording.
 * One launch, no workspace, no memset or copy: the call can be captured into a graph.  Envelope: 1 <= N < 2^31, B >= 1, T >= 1, Tp >= 1,
 * B * T and B * Tp < 2^31, Tp == T without a map, 2 <= C <= CONVASR_UNCERTAINTY_MAX_CLASSES, eps >= 0, n_events >= 0, no path without
 * events, no NULL among the pointers a form needs: checked before the launch, CONVASR_EINVAL outside it.  What only the device sees is
 * clamped there and never read out of bounds: utt into [0, B), begin into [0, Tp), end into [begin, Tp), first into [0, n_events] and
 * non-decreasing, event positions into [0, Tp), tokens into [0, C) (rule (a) and (b) compare the values as given), mapped frames into [0, T). */
int convasr_span_uncertainty(const float* log_probs, const int64_t* idx, const float* p1, const float* margin, const float* entropy,
                             const float* p_eps, const int64_t* utt, const int32_t* begin, const int32_t* end, const int64_t* first,
                             const int64_t* tokens, const int32_t* frames, int64_t n_events, const int64_t* path, const int64_t* frame_map,
                             int Tp, int32_t* n_events_out, float* confidence, float* confidence_min, float* margin_out, float* entropy_out,
                             float* uncertainty, int64_t N, int B, int T, int C, float eps, void* stream);

/* ---- Distillation: the k largest logits of every frame (models.py:788-809 sparse_topk / sparse_topk_todense, the storage format behind
 * train.py --logits / --logits-topk) and the frame-level KL term of a student against such a teacher ---------------------------------- */

/* The k largest logits of every frame of channels-last fp32 logits (B, T, C) and their classes, in descending order, in ONE read.
 * Order: a strict total order on (value, class) pairs.  A larger value comes first; equal values (-0.0 == 0.0 included) go lower class
 *   first; a NaN ranks above every number (torch.topk's rule) and among NaNs the lower class comes first.  Entry j of a frame is the j-th
 *   pair of that order: the result does not depend on the mapping, and two runs are bit-equal.
 * values (B, T, k): fp32 (CONVASR_F32; the logit's own bits, the sign of a zero included) or fp16 (CONVASR_F16: round-to-nearest-even,
 *   +-inf beyond 65504 -- the bits of tensor.to(torch.float16)).  indices (B, T, k): CONVASR_INDEX_U8 (uint8), CONVASR_INDEX_I16 (int16) or
 *   CONVASR_INDEX_I32 (int32).
 * Mapping: C <= convasr_frame_uncertainty_row_classes() one thread per frame over rows staged through LDS; above it one wave per frame
 * (csrc/distill.hip).  The logits become unsigned keys in LDS whose integer order is the value order; k rounds of "take the largest key
 * left, lowest class first": k * C integer compares a frame.
 * One launch, no workspace, no memset or copy, no atomics: the call can be captured into a graph.  Envelope, checked before any launch:
 * B >= 1, T >= 1, B * T < 2^31, 2 <= C <= CONVASR_UNCERTAINTY_MAX_CLASSES, 1 <= k <= min(C, CONVASR_TOPK_MAX_K), a value and an index
 * type of the lists above, C <= 256 with uint8 indices, no NULL pointer; outside it CONVASR_EINVAL with a message and nothing written. */
#define CONVASR_TOPK_MAX_K 32
#define CONVASR_INDEX_U8 0
#define CONVASR_INDEX_I16 1
#define CONVASR_INDEX_I32 2
int convasr_topk_frames_max_k(void);
int convasr_topk_frames(const float* logits, void* values, int values_dtype, void* indices, int indices_dtype, int B, int T, int C, int k,
                        void* stream);

/* KL of a truncated teacher against a student, per frame and per utterance, with the gradient, in one pass over the student's logits.
 * Inputs: logits (B, T, C) channels-last fp32 (the student); values / indices (B, T, k) as convasr_topk_frames writes them (the teacher's
 * k kept logits of every frame and their classes, any order); lengths (B,) int64, n_b = clamp(lengths[b], 0, T); a temperature tau > 0.
 * Per frame t < n_b, in fp32, with it = 1 / tau rounded once:
 *   s_c = z_c * it over all C classes, m = max_c s_c, S = sum_c expf(s_c - m):         q = softmax(z / tau), log q_c = s_c - m - logf(S)
 *   u_j = v_j * it over the k kept logits, mu = max_j u_j, Sp = sum_j expf(u_j - mu):   p = softmax(v / tau) over the kept classes ONLY --
 *     the truncated teacher, renormalised; a class that was not kept carries no mass
 *   KL_t = sum_j p_j (log p_j - log q[idx_j]) = (sum_j expf(u_j - mu) ((u_j - mu) - (s_idx_j - m))) / Sp - (logf(Sp) - logf(S))
 *   (both softmaxes subtract their maximum; the differences are formed before they are weighted, so a student equal to the teacher gives 0
 *   up to the rounding of the two logf).
 * Outputs:
 *   kd_frames (B, T) fp32, always written: tau^2 KL_t, and 0 at the frames t >= n_b.
 *   kd (B,) fp32 or NULL: the sum of kd_frames[b, t] over t < n_b -- a second small launch, one workgroup per utterance, thread i adds the
 *     frames i, i + 256, ... in fp64, a xor butterfly per wave, the four waves in order, one rounding to fp32.  n_b == 0 gives exactly 0.
 *   grad (B, T, C) fp32 or NULL: d kd[b] / d z = tau (q - p scattered to its classes); exactly 0 at the frames t >= n_b.  A class that the
 *     teacher names twice loses both shares, subtracted in teacher order.
 * A teacher index outside [0, C) makes that frame's kd_frames entry and gradient row NaN (and so kd[b]): loud, and no other frame changes.
 * Non-finite teacher values are OUTSIDE the envelope and not looked for (an inf or NaN among a frame's kept logits gives a NaN or a
 * meaningless KL for that frame); a NaN student logit gives NaN for its frame.
 * Sums run in a fixed order -- classes in index order per thread (row mapping), or per-lane partials over c = lane, lane + 64, ... and a
 * xor butterfly (wave mapping); the teacher's entries in their order, or one per lane and a butterfly.  No atomics; two runs are bit-equal.
 * Mapping: as convasr_topk_frames; the row mapping writes the gradient over the staged rows in LDS and stores the tile coalesced.
 * Two launches (one without kd), no workspace beyond kd_frames, no memset or copy: the call can be captured into a graph.  Envelope,
 * checked before any launch: that of convasr_topk_frames, and 0 < tau < inf; logits, values, indices, lengths and kd_frames not NULL;
 * outside it CONVASR_EINVAL. */
int convasr_distill_kl(const float* logits, const void* values, int values_dtype, const void* indices, int indices_dtype,
                       const int64_t* lengths, float* kd, float* kd_frames, float* grad, int B, int T, int C, int k, float tau, void* stream);

/* ---- Keyword search: where in an utterance is a phrase said, and how sure is the model.  The project's own detector (the reference has
 * none): unpinned against any outside keyword spotter ------------------------------------------------------------------------------------- */

/* The CTC lattice of each of K phrases, started at every frame of every utterance and scored against the frame-wise best path; one launch.
 * Inputs: log_probs (B, T, C) channels-last fp32 (only differences within a frame matter, so logits give the same result); lengths (B,)
 * int64 or NULL (all T frames), n_b = clamp(lengths[b], 0, T); tokens (K, L_max) int32 with token_lengths (K,) int32 labels each, every
 * label in [0, C) and != blank; thresholds (K,) fp32; min_gap >= 0 frames; a capacity of H >= 1 hits per (utterance, phrase).
 * Frame scores: m_t = the largest lp[t, c] over c, NaNs ignored (fmaxf); d_t(c) = lp[t, c] - m_t in ONE fp32 subtraction, a NaN result
 *   counts as -inf.  So d <= 0 and d = 0 on the frame's argmax: the sum of d along a path is the log-likelihood ratio of that path
 *   against the greedy path.
 * Values: a value is a pair (score fp32, begin int32).  better(...) takes the largest score, among equal finite scores the smallest begin; a
 *   score of -inf always carries begin -1.  v + x adds x to the score in ONE fp32 addition and keeps begin; a result of -inf resets begin
 *   to -1.
 * Recurrence, for a phrase y_0 .. y_{L-1} over the frames t = 0 .. n_b - 1, everything (-inf, -1) before frame 0:
 *   A_0(t) = better(A_0(t-1), (0, t))                                             + d_t(y_0)
 *   A_i(t) = better(A_i(t-1), Z_{i-1}(t-1), A_{i-1}(t-1) only if y_i != y_{i-1})  + d_t(y_i)     0 < i < L
 *   Z_i(t) = better(Z_i(t-1), A_i(t-1))                                           + d_t(blank)   0 <= i < L - 1
 *   E(t)   = A_{L-1}(t)
 *   A_i is the label, Z_i the blank after it; no blank before the first label or after the last one, so a span is tight.  E(t) is the best
 *   occurrence that ends at frame t, with its first frame: the maximum over all start frames and all CTC alignments of the phrase on
 *   [begin, t], ties to the earliest begin.  A phrase's spaces are ordinary labels: the model has to emit them.
 * Hit picker, per (utterance, phrase), sequential in t, with cand = none and last_end = -1:
 *   (s, b) = E(t)
 *   if s >= threshold and b > last_end and (cand is none or s > cand.score or (s == cand.score and b == cand.begin)): cand = (s, b, t)
 *   if cand is not none and t - cand.end >= min_gap: emit cand; last_end = cand.end; cand = none
 *   after the last frame: emit cand if there is one
 *   Hits come out in the order of their end frames and are disjoint.
 * Outputs: count (B, K) int32 counts EVERY hit; hit_score fp32, hit_begin, hit_end int32, each (B, K, H), hold the first H of them and are
 *   untouched beyond (an utterance of length 0: count 0, rows untouched).  dense_score fp32 / dense_begin int32 (B, K, T), both or neither
 *   (NULL): E(t), and (-inf, -1) at the frames t >= n_b.
 * Every score is a chain of fp32 additions along one path in time order, with no multiplication, and the maximum does not depend on order:
 * the result is independent of how the kernel maps work to lanes, bit-equal to a float32 restatement (tests/_kws_ref.py) on any finite or
 * -inf input, and two runs are bit-equal.  Scores are acoustic log-likelihood ratios, not calibrated probabilities.
 * Mapping: one wave per (utterance, phrase), lane i holds A_i and Z_i; the waves of a workgroup take phrases of one utterance and share its
 * frames, staged through LDS in tiles up to the staging limit of classes, gathered from global memory above it (csrc/kws.hip).  One launch, no
 * workspace, no memset or copy: the call can be captured into a graph.
 * Envelope, checked before the launch: 1 <= L_max <= CONVASR_KWS_MAX_LABELS, 2 <= C <= CONVASR_KWS_MAX_CLASSES, 1 <= T <=
 * CONVASR_KWS_MAX_FRAMES, 1 <= B, K <= 65535; outside it CONVASR_EUNSUPPORTED with a message and nothing written.  Any other bad argument
 * (NULL, H < 1, min_gap < 0, blank outside [0, C), one dense pointer without the other) CONVASR_EINVAL.  What only the device sees is clamped
 * there and never read out of bounds: token_lengths into [0, L_max] (0: count 0, no hit), labels into [0, C).
 * Pure queries (what the tests straddle): the label limit; the phrases (= waves) of one workgroup; the class count up to which frames are
 * staged through LDS; the frames of one tile at C classes (negative outside the envelope of C). */
#define CONVASR_KWS_MAX_LABELS 64
#define CONVASR_KWS_MAX_CLASSES 8192
#define CONVASR_KWS_MAX_FRAMES (1 << 20)
int convasr_ctc_keyword_search_max_labels(void);
int convasr_ctc_keyword_search_phrases_per_block(void);
int convasr_ctc_keyword_search_staged_classes(void);
int convasr_ctc_keyword_search_tile_frames(int C);
int convasr_ctc_keyword_search(const float* log_probs, const int64_t* lengths, const int32_t* tokens, const int32_t* token_lengths,
                               const float* thresholds, int32_t* count, float* hit_score, int32_t* hit_begin, int32_t* hit_end,
                               float* dense_score, int32_t* dense_begin, int B, int T, int C, int K, int L_max, int H, int blank, int min_gap,
                               void* stream);

/* ---- Alignment: metrics.py:365-407 (align_strings) and its aligner (metrics.py:447-645), the step every error analysis of the reference
 * starts with (ErrorAnalyzer.analyze, transcribe.py --align-words) ------------------------------------------------------------------------ */

/* Semi-global Needleman-Wunsch alignment with traceback of N pairs of integer sequences, one launch.
 * a (N, La) int32: the hypothesis units of every pair, a_lengths (N,) int32; b (N, Lb) int32: the reference units, b_lengths (N,) int32.
 * Only units below a length are read; the lengths are clamped to [0, La] / [0, Lb] on the device.  Two units match when their ids are equal.
 * Per pair, with la / lb the lengths and four integer scores match, sub, del, ins:
 *   Matrix.  M has (la + 1) x (lb + 1) cells.  M[i][0] = M[0][j] = 0 (leading units of either side cost nothing: the semi-global part).
 *     M[i][j] = max(M[i-1][j-1] + (a[i-1] == b[j-1] ? match : sub), M[i-1][j] + del, M[i][j-1] + ins).
 *   End cell.  If la < lb: i = la and j = the LOWEST column that maximises M[la][j] over 0..lb; the units b[j:] are emitted against gaps.
 *     Otherwise: j = lb and i = the lowest row that maximises M[i][lb] over 0..la; the units a[i:] are emitted against gaps.
 *   Walk back from the end cell while i > 0 or j > 0:
 *     1. if i == 0 or j == 0, the remaining prefix of the other sequence is emitted against gaps and the walk stops;
 *     2. otherwise, if M[i][j] == M[i][j-1] + ins: the column (gap, b[j-1]) and j -= 1;
 *     3. else if M[i][j] == M[i-1][j] + del: the column (a[i-1], gap) and i -= 1;
 *     4. else the column (a[i-1], b[j-1]) and both decrease.
 *     The priority ins, del, diagonal makes the alignment unique.
 * Output per pair, rows of La + Lb entries: a_index / b_index (N, La + Lb) int32 = per alignment column, in forward order, the 0-based
 * unit of a / of b, or -1 for a gap; -1 past the last column.  n_cols (N,) int32 = the number of columns (max(la, lb) <= n_cols <= la + lb).
 * score (N,) int32 = M at the end cell.  Empty sequences are legal: an empty side gives gaps only, two empty sides no column.
 * One 64-thread workgroup per pair.  workspace: at least convasr_nw_align_workspace_bytes(N, La, Lb) =
 * N * La * ceil(Lb / 64) * 16 + N * (La + Lb) * 4 bytes (2 direction bits per cell, then the walked columns), 16-byte aligned,
 * uninitialised; no memset or copy: the call can be captured into a graph.  The query returns -1 outside the envelope of N, La, Lb.
 * Envelope, checked before any launch: 1 <= N < 2^20, 0 <= La, Lb <= CONVASR_METRIC_MAX_LEN, every score in [-32768, 32768] (so that no
 * cell leaves int32), no NULL pointer, workspace_bytes at least the query's answer; outside it CONVASR_EINVAL. */
int64_t convasr_nw_align_workspace_bytes(int N, int La, int Lb);
int convasr_nw_align(const int32_t* a, const int32_t* a_lengths, const int32_t* b, const int32_t* b_lengths, int32_t* a_index,
                     int32_t* b_index, int32_t* n_cols, int32_t* score, void* workspace, int64_t workspace_bytes, int N, int La, int Lb,
                     int match, int sub, int del, int ins, void* stream);

/* The same alignment for whole recordings: up to CONVASR_NW_LONG_MAX_LEN units a side, on many CUs.  Arguments, matrix, end-cell rule,
 * walk priority and outputs are those of convasr_nw_align, and every output equals convasr_nw_align's bit for bit wherever both accept
 * the arguments.  The matrix is cut into square tiles of convasr_nw_align_long_tile() cells a side (a multiple of 64; 256), one wave per
 * tile; launch k of ceil(La / tile) + ceil(Lb / tile) - 1 plain launches runs the k-th anti-diagonal of tiles of all N pairs (the count
 * comes from La and Lb, nothing is read back; a tile wholly outside a pair's own la x lb ends at once).  What crosses a tile edge -- the
 * last row of every tile row, the last column of every tile column -- is stored whole in the workspace and only ever read by a later
 * launch: no workgroup waits on another, no cooperative launch, no atomics.  The tiles of the last tile row (la < lb) or column leave a
 * per-tile best end cell; one more launch, one wave per pair, reduces them and walks back through the directions a tile at a time.
 * workspace: at least convasr_nw_align_long_workspace_bytes(N, La, Lb) bytes, 16-byte aligned, uninitialised.  With T the tile edge,
 * ti = ceil(La / T), tj = ceil(Lb / T) and up(n) = n rounded up to a multiple of 256, the query returns
 *   up(N * ti * tj * T * T / 4)            2 direction bits per cell, per tile contiguously (16 KiB a tile: 4 GiB for 131,071 x 131,071)
 * + up(N * ti * (Lb + 1) * 4)              the last row of every tile row
 * + up(N * tj * (La + 1) * 4)              the last column of every tile column
 * + up(N * max(ti, tj, 1) * 8)             the per-tile end-cell keys
 * + up(N * (La + Lb) * 8)                  the walked columns,
 * or -1 outside the envelope of N, La, Lb.  No memset or copy; the call makes hundreds of launches for a long pair and is NOT meant for
 * graph capture.
 * Envelope, checked before any launch: 1 <= N < 2^20, 0 <= La, Lb <= CONVASR_NW_LONG_MAX_LEN (ctc_alignment_long's label limit), every
 * score in [-2048, 2048] (a cell is at most 2048 * 262,142 < 2^29 in magnitude, E[k] - k * ins below 2^30: int32 cells), no NULL
 * pointer, workspace_bytes at least the query's answer; outside it CONVASR_EINVAL (a length past the limit: CONVASR_EUNSUPPORTED).
 * convasr_nw_align_long_parts: parts 1 = the fill only, 2 = the end cell and the walk over a workspace that a fill with the same
 * arguments left, 3 = both (for measurements that time the two apart). */
#define CONVASR_NW_LONG_MAX_LEN 131071
int convasr_nw_align_long_tile(void);
int64_t convasr_nw_align_long_workspace_bytes(int N, int La, int Lb);
int convasr_nw_align_long(const int32_t* a, const int32_t* a_lengths, const int32_t* b, const int32_t* b_lengths, int32_t* a_index,
                          int32_t* b_index, int32_t* n_cols, int32_t* score, void* workspace, int64_t workspace_bytes, int N, int La, int Lb,
                          int match, int sub, int del, int ins, void* stream);
int convasr_nw_align_long_parts(const int32_t* a, const int32_t* a_lengths, const int32_t* b, const int32_t* b_lengths, int32_t* a_index,
                                int32_t* b_index, int32_t* n_cols, int32_t* score, void* workspace, int64_t workspace_bytes, int N, int La,
                                int Lb, int match, int sub, int del, int ins, int parts, void* stream);

/* Levenshtein distances of N pairs of integer unit ids, up to CONVASR_NW_LONG_MAX_LEN units a side, on many CUs (convasr_edit_distance
 * stops at CONVASR_METRIC_MAX_LEN and makes the ids itself; here the caller does).  a (N, La) int32 with a_lengths (N,) int32, b (N, Lb)
 * int32 with b_lengths (N,) int32; only units below a length are read, the lengths are clamped to [0, La] / [0, Lb] on the device; two
 * units are equal iff their ids are equal.  distance (N,) int32 = D[la][lb] with D[i][0] = i, D[0][j] = j,
 * D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + (a[i-1] != b[j-1])): exact.
 * The tiles and launches of convasr_nw_align_long with min for max (one more small launch writes the pairs with an empty side); no
 * directions, no end-cell search, no walk.  workspace: at least convasr_edit_distance_long_workspace_bytes(N, La, Lb) =
 * up(N * ti * (Lb + 1) * 4) + up(N * tj * (La + 1) * 4) bytes (the two boundary families above: 268 MB each at the limit), 16-byte
 * aligned, uninitialised; -1 outside the envelope.  No memset or copy; not meant for graph capture.
 * Envelope, checked before any launch: 1 <= N < 2^20, 0 <= La, Lb <= CONVASR_NW_LONG_MAX_LEN, no NULL pointer, workspace_bytes at least
 * the query's answer; outside it CONVASR_EINVAL (a length past the limit: CONVASR_EUNSUPPORTED). */
int64_t convasr_edit_distance_long_workspace_bytes(int N, int La, int Lb);
int convasr_edit_distance_long(const int32_t* a, const int32_t* a_lengths, const int32_t* b, const int32_t* b_lengths, int32_t* distance,
                               void* workspace, int64_t workspace_bytes, int N, int La, int Lb, void* stream);

/* ---- Two-channel diarization: diarization.py:58-99 (select_speaker, a channel-energy diarizer with a primitive VAD), models.py:777-785
 * (rle1d, which turns its masks into segments), diarization.py:175-201 (the counts behind speaker_error).  Every result is exact: maxima,
 * comparisons, integer sums, and one IEEE add and divide per channel and position. --------------------------------------------------------- */

#define CONVASR_DIAR_MAX_LEN 268435456LL /* samples per channel: 2^28, 4.6 hours at 16 kHz */
#define CONVASR_DIAR_MAX_KERNEL 16384
#define CONVASR_RLE_MAX_LEN 1073741824LL /* 2^30 elements */
#define CONVASR_SPEAKER_MAX_PERMS 8
enum { CONVASR_SLIDE_ABS = 1, CONVASR_SLIDE_NEG = 2 };

/* Sliding maximum of C rows, stride 1, window K, -inf padding of K / 2 (integer division) on both sides: F.max_pool1d(x.unsqueeze(1), K,
 * stride = 1, padding = K // 2).  in (C, Lin) fp32, out (C, Lout) fp32 with Lout = Lin + 2 * (K / 2) - K + 1 (Lin for an odd K, Lin + 1 for
 * an even one; the out_len query returns it, -1 outside the envelope): out[c][i] = max over j in [i - K / 2, i - K / 2 + K - 1] within
 * [0, Lin) of f(in[c][j]).  flags: CONVASR_SLIDE_ABS: f(x) = |x|; CONVASR_SLIDE_NEG: f(x) = -x and the result is negated again, i.e. a
 * sliding MINIMUM with +inf padding (the erosion -max_pool1d(-x)); both: the minimum of |x|.  The cost does not depend on K (van Herk /
 * Gil-Werman, one launch).  The tile query returns how many outputs one workgroup produces for a window K (7,936 - K + 1 up to K = 2,048,
 * 31,744 - K + 1 above), for tests that straddle it.  Samples are assumed finite (not checked; a NaN is dropped by the maximum).
 * Envelope, checked before any launch: 1 <= C <= 65535, 1 <= Lin <= CONVASR_DIAR_MAX_LEN, 1 <= K <= CONVASR_DIAR_MAX_KERNEL, known flags,
 * no NULL pointer; outside it CONVASR_EINVAL. */
int64_t convasr_sliding_max_out_len(int64_t Lin, int K);
int convasr_sliding_max_tile(int K);
int convasr_sliding_max(const float* in, float* out, int C, int64_t Lin, int K, int flags, void* stream);

/* out[c] = the k-th smallest (k 1-based, as torch.kthvalue) of the L values of row c of x (C, L) fp32, every value >= +0 (not checked: the
 * bit patterns are ordered as unsigned integers).  A radix select: three histogram passes over x, no sort.  workspace: at least
 * convasr_kth_value_workspace_bytes(C) bytes, 16-byte aligned, uninitialised.  Envelope: 1 <= C <= 65535, 1 <= L <= CONVASR_DIAR_MAX_LEN + 1,
 * 1 <= k <= L, no NULL pointer; outside it CONVASR_EINVAL (the query returns -1). */
int64_t convasr_kth_value_workspace_bytes(int C);
int convasr_kth_value(const float* x, float* out, void* workspace, int64_t workspace_bytes, int C, int64_t L, int64_t k, void* stream);

/* prefix[i] = sum over j <= i of s[j], s[j] = +1 / 0 / -1 as d[0][j] is above / equal to / below d[1][j]; d (2, L) fp32, prefix (L,) int32.
 * Three launches (tile sums, their scan, tile scans); convasr_scan_tile returns the elements one workgroup scans (2,048), here and in the
 * run-length encoding below, for tests that straddle it.  Envelope: 1 <= L <= CONVASR_DIAR_MAX_LEN + 1, a workspace of at least the query's
 * bytes, no NULL pointer; outside it CONVASR_EINVAL (the query returns -1). */
int convasr_scan_tile(void);
int64_t convasr_sign_prefix_sum_workspace_bytes(int64_t L);
int convasr_sign_prefix_sum(const float* d, int32_t* prefix, void* workspace, int64_t workspace_bytes, int64_t L, void* stream);

/* select_speaker.  signal (2, N) fp32, contiguous, finite (not checked).  With Ksig / Ksil / Kspk = kernel_size_smooth_signal / _silence /
 * _speaker and len(L, K) = L + 2 * (K / 2) - K + 1:
 *   smoothed (2, L1) = sliding maximum of |signal|, window Ksig, L1 = len(N, Ksig);
 *   eroded (2, Le) = sliding minimum, window Ksil, of the sliding maximum, window Ksil, of |signal|; Le = len(len(N, Ksil), Ksil);
 *   kth[c] = the k-th smallest of smoothed[c] (the caller computes k = int(normalization_percentile * L1) in double);
 *   silence[c][i] = eroded[c][i] < silence_absolute_threshold or eroded[c][i] / (eps + kth[c]) < silence_relative_threshold, in fp32, the
 *     add and the divide correctly rounded;
 *   s[j] = the sign of smoothed[0][j] - smoothed[1][j]; b[i] = the sign of the zero-padded box sum of s over window Kspk, i < Ls = len(L1, Kspk);
 *     then every b[i] == 0 whose neighbours (0 outside [0, Ls)) are +1 and -1 in either order becomes +1 (all at once, on the unrepaired b);
 *   L = min(Le, Ls) (the out_len query returns it).
 * speaker_id (L,) fp32 = 0 where both channels are silent or b == 0, else 1 for b == +1 and 2 for b == -1.  mask (3, L) bytes of 0 / 1:
 * row 0 = both channels silent, row 1 = not silence[0] and b == +1, row 2 = not silence[1] and b == -1.
 * workspace: at least convasr_select_speaker_workspace_bytes(N, Ksil, Ksig, Kspk) bytes (about 28 N), 16-byte aligned, uninitialised; no
 * memset or copy: the call can be captured into a graph.  14 launches, none of whose cost depends on a kernel size.
 * Envelope, checked before any launch: 1 <= N <= CONVASR_DIAR_MAX_LEN, every kernel size in [1, CONVASR_DIAR_MAX_KERNEL], 1 <= k <= L1, no
 * NULL pointer, workspace_bytes at least the query's answer; outside it CONVASR_EINVAL (the queries return -1). */
int64_t convasr_select_speaker_out_len(int64_t N, int kernel_size_smooth_silence, int kernel_size_smooth_signal, int kernel_size_smooth_speaker);
int64_t convasr_select_speaker_workspace_bytes(int64_t N, int kernel_size_smooth_silence, int kernel_size_smooth_signal, int kernel_size_smooth_speaker);
int convasr_select_speaker(const float* signal, float* speaker_id, uint8_t* mask, void* workspace, int64_t workspace_bytes, int64_t N,
                           int kernel_size_smooth_silence, int kernel_size_smooth_signal, int kernel_size_smooth_speaker,
                           float silence_absolute_threshold, float silence_relative_threshold, float eps, int64_t k, void* stream);

/* Run-length encoding of n elements (models.rle1d) in two calls around one host read, because the output size depends on the data.
 * Elements: integers of 1, 2, 4 or 8 bytes compared bit for bit (bool included), or fp32 compared as floats (is_float = 1, elem_bytes = 4).
 * convasr_rle1d_count leaves, as an int32 at byte convasr_rle1d_count_offset(n) of the workspace, the number of i >= 1 with x[i] != x[i-1];
 * runs = that number + 1.  convasr_rle1d_write, given the same workspace untouched and `runs`, writes starts (runs,) int64, lengths (runs,)
 * int64 and values (runs,) of the element type.  Envelope: 1 <= n <= CONVASR_RLE_MAX_LEN, a listed element type, 1 <= runs <= n, a workspace
 * of at least convasr_rle1d_workspace_bytes(n), no NULL pointer; outside it CONVASR_EINVAL (the queries return -1). */
int64_t convasr_rle1d_workspace_bytes(int64_t n);
int64_t convasr_rle1d_count_offset(int64_t n);
int convasr_rle1d_count(const void* x, int elem_bytes, int is_float, int64_t n, void* workspace, int64_t workspace_bytes, void* stream);
int convasr_rle1d_write(const void* x, int elem_bytes, int is_float, int64_t n, const void* workspace, int64_t workspace_bytes, int64_t runs,
                        int64_t* starts, int64_t* lengths, void* values, void* stream);

/* The counts behind speaker_error for n_perms mappings at once.  ref_mask, hyp_mask (3, n) bytes of 0 / 1 on the device (rows 1 and 2: where
 * speakers 1 and 2 talk); perms: n_perms x 3 int32 ON THE HOST, mapping p reading the hypothesis rows perms[3p + 1] and perms[3p + 2] as
 * speakers 1 and 2.  counts (n_perms, 7) int64 on the device, per mapping with r1, r2 the reference rows and h1, h2 the mapped hypothesis rows:
 *   0: positions with (r1 != h1 or r2 != h2) and r1 != r2;   1: positions with r1 != h1 or r2 != h2;
 *   2: confusion (h1 and r2 and not r1) or (h2 and r1 and not r2);   3: false alarm (h1 or h2) and not r1 and not r2;
 *   4: miss, not h1 and not h2 and (r1 or r2);   5: positions with r1 != r2;   6: total, r1 or r2.
 * One pass over both masks and a finishing launch.  Envelope: 1 <= n <= CONVASR_RLE_MAX_LEN, 1 <= n_perms <= CONVASR_SPEAKER_MAX_PERMS, rows
 * in [0, 2], a workspace of at least the query's bytes, 8-byte aligned, no NULL pointer; outside it CONVASR_EINVAL (the query returns -1). */
int64_t convasr_speaker_error_counts_workspace_bytes(int64_t n);
int convasr_speaker_error_counts(const uint8_t* ref_mask, const uint8_t* hyp_mask, const int32_t* perms, int n_perms, int64_t n, int64_t* counts,
                                 void* workspace, int64_t workspace_bytes, void* stream);

/* ---- audio.read_audio / audio.resample (audio.py:17-128, 150-159) ------------------------------------------------------------------ */

/* Decode + de-interleave + optional mono mix + band-limited rational resampling in one pass.  The reference resamples with librosa
 * (audio.py:156); the resampler here is DEFINED BY THIS PROJECT and unpinned against librosa (which is not a dependency): same output
 * length and timing, its own filter.
 *   g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, T_out = ceil(T_in * L / M) (librosa's length rule; convasr_resample_out_len);
 *   s = rolloff * min(1, L / M); output n sits at input time tau = n * M / L:
 *     y[n] = s * sum over k of x[k] * sinc(s * (k - tau)) * w((k - tau) * s / Z),  the integers k with |k - tau| * s <= Z, x[k] = 0 outside [0, T_in);
 *     sinc(u) = sin(pi u) / (pi u);  w(v) = I0(beta * sqrt(1 - v * v)) / I0(beta) for |v| <= 1, otherwise 0;
 *   defaults Z = 64 zero crossings, beta = 14.769656459379492, rolloff = 0.9475937167399596 (the parameters resampy publishes for
 *   'kaiser_best'), the filter evaluated at the exact rational phases, not from an interpolated table.
 * table: taps x L fp32 on the device, computed by the caller in float64 and rounded once, taps = 2 * floor(Z / s) + 2 = 2 H + 2
 * (convasr_resample_taps): table[j * L + p] = s * sinc(s * d) * w(d * s / Z) with d = (L * (j - H) - p) / L where |d| * s <= Z, else 0.  With
 * k0 = floor(n * M / L) and p = (n * M) mod L the kernel computes y[n] = sum over j = 0 .. taps - 1, in that order, of
 * fma(x[k0 - H + j], table[j * L + p], .) in fp32: bit-repeatable and the same on every route.
 * x: x_dtype CONVASR_I16 = interleaved (T_in, C) int16 as a wav file holds it, each sample (float)v / 32767.f correctly rounded (s2f_numpy,
 * audio.py:15); CONVASR_F32 = planar (C, T_in) fp32.  out: planar (C, T_out) fp32; with mono != 0 (1, T_out), the filter applied to the fp32
 * mean of the channels (their sum in ascending channel order, divided by C: numpy's mean for C <= 7), mixed on the inputs in the same pass.
 * sr_in == sr_out: decode, de-interleave and mix only; table and taps are ignored.  T_in == 0: nothing is launched.
 * route: 0 = automatic; 1 = a workgroup per convasr_resample_tile() (256) consecutive outputs with their input span decoded into LDS
 * (CONVASR_EUNSUPPORTED when the span does not fit in 64 KiB: a steep downsampling); 2 = one output per thread reading global memory (tests
 * and tuning; the result does not depend on the route).  No workspace, no memset or copy: the call is one kernel node.
 * Envelope, checked before any launch: L * taps <= 2^22 table entries, 1 <= C <= 8, T_in * C < 2^40; outside it CONVASR_EUNSUPPORTED (the
 * queries return -1 / the code); any other bad argument (rates <= 0, odd taps, T_out not the length rule's, NULL) CONVASR_EINVAL. */
int convasr_resample_tile(void);
int64_t convasr_resample_out_len(int64_t T_in, int sr_in, int sr_out);
int convasr_resample_taps(int sr_in, int sr_out, double zeros, double rolloff);
int convasr_resample(const void* x, int x_dtype, int64_t T_in, int C, int mono, const float* table, int taps, int sr_in, int sr_out,
                     float* out, int64_t T_out, int route, void* stream);

/* ---- Speech activity and segments of a long recording: vad.py (detect_speech; its postprocess_cut / postprocess_batching are empty stubs)
 * and the batched_transcript slices of datasets.py:261-262.  The reference's detector is webrtcvad; the one here is DEFINED BY THIS PROJECT
 * and unpinned against it.  Every result is exact: maxima, a selection, comparisons, integers, one IEEE add and divide per frame. ----------- */

/* signal (C, N), contiguous, int16 or fp32, finite (not checked); F = frame_len; nF = ceil(N / F) frames, of which nfull = N / F (integer
 * division) are whole.
 *   peak[c][f] = max of |x[c][i]| over i in [f F, min((f + 1) F, N)): fp32 exact; int16 the maximum of |int32(x)|, then ONE correctly rounded
 *     fp32 divide by 32767 (s2f_numpy, audio.py:15), so -32768 gives 32768 / 32767.  The last, partial frame has a peak too.
 *   level[c] = the k-th smallest of peak[c][0 : nfull], k = max(1, int(percentile * nfull)) computed by the caller in double
 *     (convasr_kth_value).  With nfull == 0 every result is empty or false and the caller launches nothing.
 *   raw[c][f] = f < nfull and not (peak < abs_thr or peak / (eps + level) < rel_thr), in fp32, the add and the divide correctly rounded
 *     (select_speaker's silence test); a partial last frame is never raw speech (the reference's detect_speech drops it).
 *   mask = raw smoothed per channel in three steps of whole frames G, S, P >= 0, each on the complete result of the one before:
 *     1. a silent run with speech on both sides and length < G becomes speech;
 *     2. a speech run of length < S becomes silence, whether or not it touches an end of the recording;
 *     3. every remaining speech run [s, e) becomes [max(0, s - P), min(nF, e + P)).
 *   segments: the speech runs [a, b) of mask, by channel and then time; with M = max_frames >= 2 (0: no cutting) a run longer than M is cut:
 *     while b - a > M: j = the lowest index that minimises peak[c][j] over [a + ceil(M / 2), a + M); emit [a, j); a = j.
 *     Every segment then has 1 to M frames and the segments tile the mask.  first = a F, count = min(b F, N) - a F samples.
 *   gather: out[b][t] = value(signal[channel_b][first_b + t]) for t < count_b, 0 for count_b <= t < Tpad; value = the sample (fp32) or
 *     int16 / 32767 in fp32, correctly rounded.
 *
 * convasr_frame_peak: peaks (C, nF) fp32.  One launch: a group of 1 to 64 lanes per frame (about 16 samples a lane), 16-byte loads between a
 * scalar head up to the first 16-byte boundary and a scalar tail, so rows that start unaligned (odd N) are read the same way; 64-bit
 * indices.  convasr_frame_peak_tile(F) = frames one workgroup takes per step (256 / lanes per frame), for tests that straddle it.
 * convasr_vad_frames: raw, mask (C, nF) bytes of 0 / 1; level (C,) fp32 on the device.  One launch, one workgroup per channel walking the
 * frames in tiles of 8,192 with its scan state carried over; workspace: convasr_vad_frames_workspace_bytes(C, nF) bytes, 4-byte aligned,
 * uninitialised.  n_full is nF or nF - 1, at least 1.
 * convasr_vad_segments_count / _write: two calls around one host read, because the number of segments depends on the data.  count leaves the
 * number of segments of channel c as int32 number c of the workspace (convasr_vad_segments_workspace_bytes(C, nF) bytes, 4-byte aligned,
 * uninitialised); write, given the same workspace untouched and total = their sum >= 1, writes channel, first, count (total,) int64.  A wave
 * per run makes the cuts one after the other.
 * convasr_gather_segments: segments (3, B) int64 -- the rows channel, first, count -- once ON THE HOST (segments_host: checked here) and
 * once on the device (read by the kernel); out (B, Tpad) fp32, Tpad >= the longest count.  One launch.
 * None of them issues a memset or a copy: every call is one kernel node.
 * Envelope, checked before any launch: 1 <= C <= 8, 1 <= N <= 2^28 (1 <= nF <= 2^28), 1 <= F <= 65536, G, S, P >= 0, max_frames 0 or >= 2,
 * 1 <= B <= 65535, 0 <= channel < C, 0 <= first, 1 <= count, first + count <= N, a listed dtype, a workspace of the query's size, no NULL
 * pointer; outside it CONVASR_EINVAL (the queries return -1 / the code). */
int convasr_frame_peak_tile(int frame_len);
int convasr_frame_peak(const void* signal, int dtype, int C, int64_t N, int frame_len, float* peaks, void* stream);
int64_t convasr_vad_frames_workspace_bytes(int C, int64_t n_frames);
int convasr_vad_frames(const float* peaks, const float* level, int C, int64_t n_frames, int64_t n_full, float abs_thr, float rel_thr, float eps,
                       int64_t G, int64_t S, int64_t P, uint8_t* raw, uint8_t* mask, void* workspace, int64_t workspace_bytes, void* stream);
int64_t convasr_vad_segments_workspace_bytes(int C, int64_t n_frames);
int convasr_vad_segments_count(const uint8_t* mask, const float* peaks, int C, int64_t n_frames, int64_t max_frames, void* workspace,
                               int64_t workspace_bytes, void* stream);
int convasr_vad_segments_write(const uint8_t* mask, int C, int64_t n_frames, int frame_len, int64_t N, const void* workspace,
                               int64_t workspace_bytes, int64_t total, int64_t* channel, int64_t* first, int64_t* count, void* stream);
int convasr_gather_segments(const void* signal, int dtype, int C, int64_t N, const int64_t* segments_host, const int64_t* segments, int B,
                            float* out, int64_t Tpad, void* stream);

/* ---- Training-time augmentation of a collated batch: speed, gain, noise on the waveforms, SpecAugment on the features.  The reference has
 * none (its frontend's dither is commented out); this augmentation is DEFINED BY THIS PROJECT and unpinned against torchaudio, NeMo or Kaldi
 * (none of which is a dependency).  Integers (which augmentations fire, table indices, lengths, mask positions) are exact and restatable on
 * the host; samples are fp32 sums in a fixed order. ------------------------------------------------------------------------------------ */

/* The generator: Philox4x32-10 (Salmon et al. 2011; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85).  A random
 * decision is word 0 of the block with
 *   counter = (key & 0xffffffff, key >> 32, epoch, purpose << 16 | index),  Philox key = (seed & 0xffffffff, seed >> 32),
 * key = the utterance's id (64 bits), epoch < 2^32, index = the number of the mask (0 elsewhere), purpose: 0 speed fires, 1 speed, 2 gain fires,
 * 3 gain, 4 noise fires, 5 noise row, 6 noise offset, 7 SNR, 8 / 9 frequency-mask width / start, 10 / 11 time-mask width / start.  Nothing else
 * enters: not the utterance's place in the batch, not the batch, not the rank, not the steps run before.  With r the word:
 *   "fires with probability p": (r >> 8) < floor(p * 2^24), the threshold computed once by the caller;
 *   a uniform integer in [0, n]: ((r >> 8) * (n + 1)) >> 24 in 64 bits (n < 2^40).
 * No kernel of this section evaluates log, exp, sin or cos: gains, SNR factors and filters are tables the caller computed in float64 and
 * rounded once.
 * convasr_philox: the raw generator, for tests.  counters (n, 4) int64 holding 32-bit words, out (n, 4) int64 the four words of each block.
 *
 * convasr_augment_params -- one launch, one lane per utterance -- writes params (B, 8) int64 and xlen_out (B,) fp32:
 *   len = ceil(xlen[b] * T) in fp32 (convasr_output_lengths' rule), clamped to [0, T];
 *   speed: i = uniform in [0, n_speeds - 1], step = steps[i] = round(speed_i * 2^32), out_len = floor(len * 2^32 / step).  The utterance keeps
 *     speed 1 (i = -1, step = 2^32, out_len = len) when the draw does not fire, when out_len > T, or when min_out_len is given and out_len <
 *     min_out_len[b]: exact integer comparisons.
 *   gain: index uniform in [0, gain_steps - 1] when gain_steps > 0 and the draw fires, else -1;
 *   noise: row uniform in [0, noise_rows - 1], offset uniform in [0, noise_len - 1], SNR index uniform in [0, snr_steps - 1] when noise_rows > 0
 *     and the draw fires, else row -1, offset 0, SNR index 0.
 *   params[b] = (speed index, step, gain index, noise row, noise offset, SNR index, len, out_len);  xlen_out[b] = out_len / T, one fp32 divide.
 *   steps: n_speeds 64-bit words ON THE HOST.
 *
 * convasr_augment_waveform -- one launch -- x (B, T) fp32 or int16 (each sample (float)v / 32767.f correctly rounded), out (B, T) fp32 of the
 * SAME padded length.  With x[k] = 0 outside [0, len), P = convasr_augment_phases() = 128 and H = taps / 2 - 1, for n < out_len:
 *   step == 2^32: y = x[n], bit for bit;
 *   otherwise pos = n * step (64-bit), k0 = pos >> 32, frac = pos & 0xffffffff, p = frac >> 25, f = ((frac << 7) & 0xffffffff) >> 8 scaled by
 *     2^-24 (exact in fp32), and y = sum over j = 0 .. taps - 1, in that order, of fma(x[k0 - H + j], c_j, .) with c_j = fma(f, t1 - t0, t0),
 *     t0 = table[i][j][p], t1 = table[i][j][p + 1]: LINEAR INTERPOLATION between the two neighbouring of P tabulated phases;
 *   then y = y * gain_table[gain index] when the index is >= 0.
 *   out[b][n] = y for n < out_len and 0 for out_len <= n < T.
 *   table: (n_speeds, taps, P + 1) fp32 on the device, table[i][j][p] = h_i((j - H) - p / P), h(d) = c * sinc(c * d) * w(d * c / Z) where
 *     |d| * c <= Z and 0 elsewhere, c = rolloff * min(1, 1 / speed_i), sinc and the Kaiser window w as in convasr_resample, taps = 2 * floor(Z /
 *     c_min) + 2 for the smallest c of the table.  taps == 0: no table, every utterance is copied (its step must be 2^32).
 *   partials: (B, convasr_augment_parts(), 2) float64 workspace, uninitialised.  A workgroup owns the tiles part, part + nparts, ... of an
 *     utterance (tiles of convasr_augment_tile() = 1024 outputs, nparts = min(tiles, parts)) and leaves (sum of y^2, sum of v^2) over its outputs
 *     n < out_len, v = noise[row][(offset + n) mod noise_len] (0 without a row): float64 products and sums per lane, then a fixed tree.
 * convasr_augment_mix -- one launch, only with a noise bank -- Ex, En = the partial pairs added in index order in float64;
 *   scale = (float)(snr_table[SNR index] * sqrt(Ex / En)) in float64 when the utterance has a row and Ex > 0 and En > 0, else 0 (nothing is
 *   added); out[b][n] = fma(scale, v_n, out[b][n]) for n < out_len; scales (B,) fp32 is an output.  Two runs are bit-equal.
 * Three plain launches (two without noise), no memset, no copy, no host synchronisation, no atomics.  B == 0 or T == 0 launches nothing.
 * Envelope, checked before any launch: B <= 65535, T < 2^31, 1 <= n_speeds <= 32, every step in [2^31, 2^33] (speeds in [0.5, 2]), gain_steps and
 * snr_steps <= 4096, noise rows and samples < 2^31 each, the table of one speed and a tile's input span within 160 KiB of LDS (taps <= 298);
 * outside it CONVASR_EUNSUPPORTED; any other bad argument (odd taps, a threshold above 2^24, epoch outside [0, 2^32), NULL) CONVASR_EINVAL.
 * A params tensor of the caller's own making is read defensively: indices outside their tables mean "none". */
int convasr_philox(const int64_t* counters, int64_t n, uint32_t key0, uint32_t key1, int64_t* out, void* stream);
int convasr_augment_tile(void);
int convasr_augment_phases(void);
int convasr_augment_parts(void);
int convasr_augment_params(const float* xlen, const int64_t* keys, const int64_t* min_out_len, int B, int64_t T, uint64_t seed, int64_t epoch,
                           const uint64_t* steps, int n_speeds, uint32_t speed_thr, int gain_steps, uint32_t gain_thr, int64_t noise_rows,
                           int64_t noise_len, int snr_steps, uint32_t noise_thr, int64_t* params, float* xlen_out, void* stream);
int convasr_augment_waveform(const void* x, int x_dtype, int B, int64_t T, const int64_t* params, const float* table, int n_speeds, int taps,
                             const float* gain_table, int gain_steps, const float* noise, int64_t noise_rows, int64_t noise_len, float* out,
                             double* partials, void* stream);
int convasr_augment_mix(float* out, int B, int64_t T, const int64_t* params, const float* noise, int64_t noise_rows, int64_t noise_len,
                        const float* snr_table, int snr_steps, const double* partials, float* scales, void* stream);

/* Room reverberation, between the gain and the noise: the order per utterance is speed, gain, reverberation, noise.  Like the rest of the
 * section it is this project's own and unpinned.
 *   The bank: rir (R, Lmax) fp32 on the device, rir_len (R,) int64 with 1 <= rir_len[r] <= Lmax, rir_delay (R,) int64 = d_r, the index of the
 *     first largest |h_r[k]| (the direct path), computed once by the caller.  rir_len and rir_delay are passed twice: on the device for the
 *     kernels and ON THE HOST (rir_len_host, rir_delay_host) for the checks below, which therefore cost no synchronisation.
 *   Two more purposes of the generator: 12 "reverb fires", 13 the row, uniform in [0, R - 1]; purposes 0 - 11 keep their meaning and draws.
 * convasr_augment_reverb_params -- one launch, one lane per utterance -- writes rir_row (B,) int64: the row when the draw fires (threshold
 *   reverb_thr = floor(p * 2^24)), else -1.  The (B, 8) params tensor is untouched.
 * convasr_augment_reverb -- three launches -- y (B, T) fp32 = convasr_augment_waveform's output, out (B, T) fp32, y != out.  With out_len =
 *   params' out_len clamped to [0, T], r = rir_row[b], y[k] = 0 outside [0, out_len):
 *     z[n] = sum over k < rir_len[r] of h_r[k] * y[n + d_r - k]  for n < out_len,   z[n] = 0 for out_len <= n < T:
 *   the output is shifted by the direct-path delay and cut at out_len, so xlen_out does not change and the labels stay aligned.  r == -1
 *   copies y bit for bit; a row outside the bank, or whose device-side length or delay is outside its range, is read as -1.
 *   Method: uniformly partitioned overlap-save, blocks of Bk = convasr_augment_reverb_block() = 1024 outputs, FFTs of 2 Bk complex points in
 *     LDS (radix-2 Stockham), P = ceil(rir_len / Bk) parts; two output blocks share one complex FFT (block m in the real parts, block m +
 *     ceil(M / 2) of the utterance's M blocks in the imaginary ones); per frequency bin the P complex products are added in ascending part
 *     index, four fma each.  The order is fixed and depends neither on B nor on the utterance's place in the batch: two runs are bit-equal,
 *     and an utterance's output is bit-equal wherever it sits.  An utterance with min(rir_len, out_len) <= convasr_augment_reverb_direct() = 32
 *     skips the FFTs: the at most 32 products of a sample with 0 <= n + d_r - k < out_len are summed directly, one fma each in ascending k.
 *   twiddles: (Bk, 4) fp32 on the device, 16-byte aligned, (c_hi, s_hi, c_lo, s_lo) for t < Bk with c = cos(pi t / Bk), s = -sin(pi t / Bk)
 *     computed in float64 by the caller, hi = the value rounded to fp32 and lo = the remainder rounded to fp32: a twiddle of one float per
 *     component misses |w| = 1 by up to 3e-8, which biases the energy of z by more than the noise scale's last fp32 bit.
 *   partials: (B, convasr_augment_parts(), 2) float64, (sum of z^2, sum of v^2) over n < out_len in exactly the layout, tile ownership and
 *     order that convasr_augment_waveform leaves them in (for r == -1 the same bits), so convasr_augment_mix runs unchanged afterwards and its
 *     SNR is relative to the reverberated speech.  noise may be NULL (rows 0).
 *   workspace: convasr_augment_reverb_workspace_bytes(B, T, the longest rir_len) bytes, uninitialised.
 * Plain launches only: no memset or copy nodes, no atomics, no host synchronisation.  B == 0 or T == 0 launches nothing.
 * Envelope, checked before any launch: every rir_len <= 32768, R < 2^31, B <= 65535, T < 2^31; outside it CONVASR_EUNSUPPORTED.  A NULL pointer,
 * R or Lmax or a length of 0, a length above Lmax, a delay outside [0, rir_len), y == out or a workspace that is too small: CONVASR_EINVAL. */
int convasr_augment_reverb_block(void);
int convasr_augment_reverb_direct(void);
int64_t convasr_augment_reverb_workspace_bytes(int B, int64_t T, int64_t max_rir_len);
int convasr_augment_reverb_params(const int64_t* keys, int B, uint64_t seed, int64_t epoch, int64_t rir_rows, uint32_t reverb_thr,
                                  int64_t* rir_row, void* stream);
int convasr_augment_reverb(const float* y, int B, int64_t T, const int64_t* params, const int64_t* rir_row, const float* rir, int64_t rir_rows,
                           int64_t rir_max_len, const int64_t* rir_len, const int64_t* rir_delay, const int64_t* rir_len_host,
                           const int64_t* rir_delay_host, const float* twiddles, const float* noise, int64_t noise_rows, int64_t noise_len,
                           float* out, double* partials, void* workspace, int64_t workspace_bytes, void* stream);

/* SpecAugment (Park et al. 2019, without time warping) on x (B, F, T) fp32 log-mel features, out of the same shape, x != out.
 *   valid = ceil(xlen[b] * T) in fp32, clamped to [0, T];
 *   frequency mask i < freq_masks: w = uniform in [0, min(freq_width, F)], start = uniform in [0, F - w];
 *   time mask i < time_masks: w = uniform in [0, min(time_width, (valid * time_fraction_q24) >> 24)] -- floor(time_fraction * valid) with the
 *     fraction in 24-bit fixed point, time_fraction_q24 = floor(time_fraction * 2^24) by the caller -- start = uniform in [0, valid - w];
 *   out[b][f][t] = fill where t < valid and (f lies in a frequency mask or t in a time mask); every other value, the frames past valid
 *     included, is copied bit for bit.  No mask leaves the valid region.
 *   fill: fill_mean == 0: fill_value; otherwise the mean of x[b] over all channels and the valid frames (0 when there is none): float64 sums
 *     per lane over the elements lane, lane + 1024, ... of the valid region in (channel, frame) order, a fixed tree, one divide, one rounding
 *     to fp32.  fill_out (B,) fp32 receives the fill used; masks_out (optional) (B, freq_masks + time_masks, 2) int32 the (start, width) pairs.
 *   keys (>= B int64) and epoch (one int64) are DEVICE buffers read by the kernel: a captured graph that holds the launch draws fresh masks
 *   on every replay when the caller rewrote them beforehand in stream order.
 * One launch -- 1 to 8 workgroups per utterance, each forming the same mean in the same order and writing its share in steps of
 * convasr_spec_augment_tile() = 1024 elements -- no workspace, no memset or copy: one kernel node.  B, F or T == 0 launches nothing.
 * Envelope: B <= 65535, F * T < 2^31, at most 16 masks of each kind; outside it CONVASR_EUNSUPPORTED; negative widths, a fraction above 2^24,
 * x == out or NULL: CONVASR_EINVAL. */
int convasr_spec_augment_tile(void);
int convasr_spec_augment(const float* x, const float* xlen, const int64_t* keys, const int64_t* epoch, uint64_t seed, int B, int F, int T,
                         int freq_masks, int freq_width, int time_masks, int time_width, uint32_t time_fraction_q24, int fill_mean,
                         float fill_value, float* out, float* fill_out, int32_t* masks_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif

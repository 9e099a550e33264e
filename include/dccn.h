/*
 * dccn.h -- C ABI of libdccn.so, the MI355X (gfx950) implementation of the DCCN OFDM
 * receiver hot path.
 *
 * The reference (zhongyuanzhao/dl_ofdm) has no FFI: its boundary is the Python layer
 * API of dev/py/complex.py + dev/py/model.py sitting on TensorFlow library ops.  Each
 * entry point below replaces the TF ops behind one of those call sites (cited per
 * function as dev/py/<file>:<lines>).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (16-byte aligned), unless
 *     the parameter comment says "host";
 *   - all tensors are dense row-major float32; complex values carry a trailing
 *     {I,Q} axis of size 2 (dev/py/ofdm.py:375-377);
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous and
 *     stream-ordered, allocates nothing, and is re-entrant given distinct workspaces;
 *   - the return value is 0 (DCCN_OK) or a negative dccn_status; no C++ exception
 *     crosses the ABI.  dccn_strerror() turns a status into text;
 *   - `*_workspace_size()` return the scratch bytes the matching call needs.
 */
#ifndef DCCN_H_
#define DCCN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dccn_stream_t;

typedef enum dccn_status {
    DCCN_OK = 0,
    DCCN_ERR_INVALID_ARG = -1,   /* bad size / null pointer / unsupported nbits */
    DCCN_ERR_WORKSPACE = -2,     /* workspace too small */
    DCCN_ERR_LAUNCH = -3,        /* hipLaunch / runtime error (see dccn_last_hip_error) */
    DCCN_ERR_NO_DEVICE = -4,     /* no gfx950 device visible */
    DCCN_ERR_STATE = -5,         /* plan used in the wrong state */
    DCCN_ERR_UNSUPPORTED = -6    /* a grouped call (dccn_eq_*_grouped) reached a launch that cannot carry several chains */
} dccn_status;

const char* dccn_strerror(int status);
int dccn_version(void);                                       /* 100*major + minor */
/* 16 hex digits: hash of the sources this library was built from (csrc/Makefile).  Measurements that are kept next to the code
 * (profiles/pmc_traffic.json) carry it, so a reader can tell whether they describe the library that is loaded. */
const char* dccn_build_id(void);
int dccn_last_hip_error(void);                       /* hipError_t of the last failure */
/* host out-params; returns DCCN_ERR_NO_DEVICE when no GPU is visible */
int dccn_device_info(int* cu_count, int* wavefront, size_t* hbm_bytes, char* arch, int arch_len);

/* ---- R0: input normalisation ------------------------------------------------------
 * dev/py/ofdmreceiver_np.py:128-129  tf.nn.moments(x,[0]) + batch_normalization/sqrt(2).
 * x,y [batch, cols]; mean,var [cols] (nullable).  y = (x*inv + (-mean*inv)) / sqrt(2),
 * inv = rsqrt(var + eps), biased variance over the batch axis. */
size_t dccn_batch_moment_norm_workspace_size(int batch, int cols);
int dccn_batch_moment_norm_fwd(const float* x, float* y, float* mean, float* var,
                               int batch, int cols, float eps,
                               void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* ---- R8: complex_clip --------------------------------------------------------------
 * dev/py/complex.py:21-27  clip_by_norm over the IQ axis + mean clipped power.
 * x,y [n_pairs,2] (y nullable: power only); power_out: device float[1]. */
size_t dccn_clip_power_workspace_size(long long n_pairs);
int dccn_clip_power(const float* x, float* y, float* power_out, long long n_pairs, float peak,
                    void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* ---- R1 / R1': complex convolution as one fused real GEMM ---------------------------
 * dev/py/complex.py:140-196 (layers_conv2d_complex) and :51-92 (layers_conv1d_complex):
 * conv3d/conv2d with 2F filters + 4-way combine.  GEMM form over an (im2col) patch axis:
 *   x    [rows, kin, 2]      rows = output positions, kin = taps*channels per position
 *   w    [kin, 2F]           [Wa | Wb] (the live taps of the TF kernel)
 *   bias [2F]                [ba | bb], nullable
 *   out  [rows, F, 2]        re = I.Wa - Q.Wb + (ba-bb),  im = I.Wb - Q.Wa + (bb-ba)
 * The four real products run as ONE MFMA GEMM [rows,2kin] x [2kin,2F] whose B tile is
 * expanded from w while it is staged into LDS.  Forward is bitwise deterministic. */
int dccn_cconv_gemm_fwd(const float* x, const float* w, const float* bias, float* out,
                        int rows, int kin, int F, dccn_stream_t stream);
size_t dccn_cconv_gemm_bwd_w_workspace_size(int rows, int kin, int F);
/* dw [kin,2F], dbias [2F] (nullable) from x and dout [rows,F,2] */
int dccn_cconv_gemm_bwd_w(const float* x, const float* dout, float* dw, float* dbias,
                          int rows, int kin, int F,
                          void* workspace, size_t workspace_bytes, dccn_stream_t stream);
/* dx [rows,kin,2] from dout and w */
int dccn_cconv_gemm_bwd_x(const float* dout, const float* w, float* dx,
                          int rows, int kin, int F, dccn_stream_t stream);

/* ---- R2: dense layer ---------------------------------------------------------------
 * dev/py/model.py:1268-1275  tf.layers.dense: y[M,N] = x[M,K] . w[K,N] + bias[N]. */
int dccn_dense_fwd(const float* x, const float* w, const float* bias, float* y,
                   int M, int K, int N, dccn_stream_t stream);
int dccn_dense_bwd_x(const float* dy, const float* w, float* dx,
                     int M, int K, int N, dccn_stream_t stream);
size_t dccn_dense_bwd_w_workspace_size(int M, int K, int N);
int dccn_dense_bwd_w(const float* x, const float* dy, float* dw, float* dbias,
                     int M, int K, int N,
                     void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* both gradients of the dense layer in ONE grouped launch (dx = dy.w^T and dw = x^T.dy are independent
 * GEMMs that share dy; packing their blocks on one grid fills the CUs far better than two launches);
 * workspace as dccn_dense_bwd_w_workspace_size(M,K,N). */
int dccn_dense_bwd(const float* x, const float* dy, const float* w, float* dx, float* dw, float* dbias,
                   int M, int K, int N, void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* the same grouped launch, stopping before the split-K reduction: dx is final, the weight gradient is left
 * as `*splits` slabs [splits][K*N] at the start of the workspace (bias slabs [splits][N] follow, 256-byte
 * aligned) -- this is the stage the fused training step runs (its Adam kernel sums the slabs).
 * `splits` is a host out-parameter (1 = dw/dbias were written directly). */
int dccn_dense_bwd_slabs(const float* x, const float* dy, const float* w, float* dx, float* dw, float* dbias,
                         int M, int K, int N, void* workspace, size_t workspace_bytes, int* splits,
                         dccn_stream_t stream);

/* ---- R3-R6: demodulation tail + loss + BER ----------------------------------------
 * dev/py/model.py:1278-1291 (1x1 conv2d 2->m, leaky-ReLU 0.2, concat, dense (m+2)->2b,
 * leaky-ReLU, softmax over bit pairs), dev/py/ofdmreceiver_np.py:154-169 (one_hot,
 * softmax_cross_entropy_with_logits on the softmax OUTPUT, argmax, confusion matrix),
 * dev/py/util.py:44-48 (ber_tensor).  m = 2^nbits, nbits in 1..4.
 *   z      [cells, 2]         dense output viewed per data cell
 *   bits   [cells, nbits]     int32 labels
 *   tailp  [dccn_tail_param_count(nbits)]  packed: w1[2,m] | b1[m] | w2[m+2,2b] | b2[2b]
 *   prob   [cells, nbits, 2]  (nullable)
 *   metrics: device dccn_metrics, written by the call (deterministic two-stage reduce)
 * _fwd_bwd additionally emits dz [cells,2] and dtailp (same packing), the gradient of
 * ce_mean = mean over cells*nbits of the cross entropy. */
typedef struct dccn_metrics {
    double ce_sum;             /* sum of per-bit cross entropies */
    long long conf[4];         /* confusion matrix, row = label, col = decision */
    long long count;           /* cells * nbits */
    float ce_mean;             /* ce_sum / count */
    float berlin;              /* (conf[1]+conf[2]) / count, f64 division cast to f32 */
    float log_ber;             /* logf(berlin) (-inf when error free) */
    float reserved;
} dccn_metrics;

int dccn_tail_param_count(int nbits);
size_t dccn_demod_tail_workspace_size(long long cells, int nbits);
int dccn_demod_tail_loss_fwd(const float* z, const int32_t* bits, const float* tailp,
                             float* prob, dccn_metrics* metrics, long long cells, int nbits,
                             void* workspace, size_t workspace_bytes, dccn_stream_t stream);
int dccn_demod_tail_loss_fwd_bwd(const float* z, const int32_t* bits, const float* tailp,
                                 float* prob, dccn_metrics* metrics, float* dz, float* dtailp,
                                 long long cells, int nbits,
                                 void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* R2 with R3-R6 fused into its epilogue (nbits 1..2): the demodulation tail runs on the dense output tile
 * while it is still in registers, so z never has to exist in memory (dev/py/model.py:1268-1291 +
 * dev/py/ofdmreceiver_np.py:154-169 in one launch, plus the metrics finalize).
 *   x [M,K], w [K,N], bias [N], z [M,N] (nullable: not materialised), bits [M, N/2, nbits],
 *   prob [M, N/2, nbits, 2] (nullable), metrics as above; _fwd_bwd also emits dz [M,N] and dtailp.
 * Requires 16-byte aligned x/w and K % 4 == N % 4 == 0; returns DCCN_ERR_INVALID_ARG otherwise (use the separate
 * dccn_dense_fwd + dccn_demod_tail_loss_* calls then). */
size_t dccn_dense_tail_workspace_size(int M, int N, int nbits);
int dccn_dense_tail_fwd(const float* x, const float* w, const float* bias, float* z, const int32_t* bits,
                        const float* tailp, float* prob, dccn_metrics* metrics, int M, int K, int N, int nbits,
                        void* workspace, size_t workspace_bytes, dccn_stream_t stream);
int dccn_dense_tail_fwd_bwd(const float* x, const float* w, const float* bias, float* z, const int32_t* bits,
                            const float* tailp, float* prob, dccn_metrics* metrics, float* dz, float* dtailp,
                            int M, int K, int N, int nbits, void* workspace, size_t workspace_bytes,
                            dccn_stream_t stream);

/* The equaliser's pilot bottleneck (dev/py/model.py:394-412: dense SK2 -> P, dense P -> SK2, no activation in between) as
 * ONE launch per direction, a block per 16 frames x a chunk of columns (csrc/eq_bottleneck.h).  P = 2 * pilot_size must be
 * 16 or 32, SK2 a multiple of 64 (dccn_eq_bottleneck_supported); otherwise use dccn_dense_fwd / dccn_dense_bwd twice.
 *   fwd: d1 [B,P] = y [B,SK2] . W1 [SK2,P] + b1;  d2 [B,SK2] = d1 . W2 [P,SK2] + b2
 *   bwd: given dd2 = dLoss/dd2: dy_out = dy_in + (dd2 . W2^T) . W1^T  (the branch's input gradient ADDED to dy_in),
 *        dW2 = d1^T . dd2, db2, dW1 = y^T . (dd2 . W2^T), db1   (per-block partials summed in a fixed order) */
int dccn_eq_bottleneck_supported(int B, int SK2, int P);
size_t dccn_eq_bottleneck_workspace_size(int B, int SK2, int P);
int dccn_eq_bottleneck_fwd(const float* y, const float* W1, const float* b1, const float* W2, const float* b2, float* d1,
                           float* d2, int B, int SK2, int P, dccn_stream_t stream);
int dccn_eq_bottleneck_bwd(const float* dd2, const float* d1, const float* y, const float* W1, const float* W2,
                           const float* dy_in, float* dy_out, float* dW1, float* db1, float* dW2, float* db2, int B, int SK2,
                           int P, void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* Patch gather in front of dccn_cconv_gemm_* for the general-k cases of dev/py/complex.py:51-92 / :140-196 (k taps over
 * one or two axes, strides, TF SAME / VALID geometry): x [B, L, Wd, C, 2] -> rows [B*Lo*Wo, ntl*ntw*C, 2], zeros where
 * SAME padding lies; only the live taps tl0..tl0+ntl-1 / tw0..tw0+ntw-1 (those that ever meet data) are gathered.
 * _col2im is its adjoint: dx [B, L, Wd, C, 2] = sum of the patch entries that read each input element (deterministic). */
int dccn_cconv_im2col(const float* x, float* rows, int B, int L, int Wd, int C, int Lo, int Wo, int ntl, int ntw, int tl0,
                      int tw0, int sL, int sW, int pl0, int pw0, dccn_stream_t stream);
int dccn_cconv_col2im(const float* drows, float* dx, int B, int L, int Wd, int C, int Lo, int Wo, int ntl, int ntw, int tl0,
                      int tw0, int sL, int sW, int pl0, int pw0, dccn_stream_t stream);
/* The forward of the same convolutions WITHOUT the patch tensor (dev/py/complex.py:51-92, :140-196 as an implicit GEMM):
 * out [B*Lo*Wo, F, 2] = patches(x) . Weff(w) + bias, the GEMM's operand loader gathering the taps from x [B, L, Wd, C, 2]
 * itself; w [ntl*ntw*C, 2F] = [Wa|Wb] over the live taps, bias [2F] nullable.  dccn_cconv_patch_supported: 1 when the
 * shapes qualify (even C and F, 32-bit element offsets); otherwise use dccn_cconv_im2col + dccn_cconv_gemm_fwd. */
int dccn_cconv_patch_supported(int B, int L, int Wd, int C, int Lo, int Wo, int ntl, int ntw, int F);
int dccn_cconv_patch_fwd(const float* x, const float* w, const float* bias, float* out, int B, int L, int Wd, int C, int Lo,
                         int Wo, int ntl, int ntw, int tl0, int tw0, int sL, int sW, int pl0, int pw0, int F,
                         dccn_stream_t stream);
/* The backward of the same convolutions without patch-sized tensors either (the gradients TensorFlow derives for
 * dev/py/complex.py:51-92, :140-196).  _bwd_supported: bit 0 = the weight gradient qualifies, bit 1 = the input gradient does
 * (ANY stride since round 6), bit 2 = ... and is expected to be the faster route than GEMM + col2im (2C <= 32: 16-column
 * tiles, strides by phase decomposition, csrc/cconv_dx_narrow.h -- unless the taps outnumber the channels ~10:1; wider inputs:
 * 64-column tiles whose operand loader reads dout where a tap's fine position is a multiple of the stride -- at stride 1, or
 * where the zeros a strided gather multiplies cost less than the [rows, kin, 2] round trip);
 * 0 -> dccn_cconv_im2col / _gemm_bwd_w / _gemm_bwd_x / _col2im as before.
 * _bwd_w: dw [ntl*ntw*C, 2F] (+ dbias [2F], nullable) = patches(x)^T . dout, the patch rows gathered from x [B, L, Wd, C, 2]
 *   by the weight-gradient GEMM's operand loader; dout [B*Lo*Wo, F, 2].  Deterministic (split-K slabs, fixed-order fold).
 * _bwd_x: dx [B, L, Wd, C, 2] = the convolution of dout with the tap-flipped transposed weights, as the same implicit GEMM
 *   gathering from dout (no [rows, kin, 2] intermediate, no scatter), any strides.  workspace: the flipped weights,
 *   4*C*ntl*ntw*F floats. */
int dccn_cconv_patch_bwd_supported(int B, int L, int Wd, int C, int Lo, int Wo, int ntl, int ntw, int sL, int sW, int F);
size_t dccn_cconv_patch_bwd_w_workspace_size(int B, int Lo, int Wo, int C, int ntl, int ntw, int F);
int dccn_cconv_patch_bwd_w(const float* x, const float* dout, float* dw, float* dbias, int B, int L, int Wd, int C, int Lo,
                           int Wo, int ntl, int ntw, int tl0, int tw0, int sL, int sW, int pl0, int pw0, int F,
                           void* workspace, size_t workspace_bytes, dccn_stream_t stream);
size_t dccn_cconv_patch_bwd_x_workspace_size(int C, int ntl, int ntw, int F);
int dccn_cconv_patch_bwd_x(const float* dout, const float* w, float* dx, int B, int L, int Wd, int C, int Lo, int Wo, int ntl,
                           int ntw, int tl0, int tw0, int sL, int sW, int pl0, int pw0, int F, void* workspace,
                           size_t workspace_bytes, dccn_stream_t stream);

/* Few-channel 1-D C-Convs (layers_conv1d_complex, dev/py/complex.py:51-92: x [B, L, C, 2], ntl live taps from tl0, stride sL,
 * pl0 samples of padding in front; 2*ntl*C <= 30, F = 32 or 64): dx, dw [ntl*C, 2F] and dbias [2F] (nullable) in ONE pass over
 * dout [B*Lo, F, 2] (csrc/cconv1d_bwd.h) -- the three gradients of dccn_cconv_patch_bwd_w / _bwd_x, same 1e-5 parity, for
 * about the cost of one of them on these shapes (dout is the only large tensor).  Deterministic. */
int dccn_cconv1d_bwd_supported(int B, int L, int C, int Lo, int ntl, int sL, int F);
size_t dccn_cconv1d_bwd_workspace_size(int F);
int dccn_cconv1d_bwd(const float* x, const float* dout, const float* w, float* dx, float* dw, float* dbias, int B, int L, int C,
                     int Lo, int ntl, int tl0, int sL, int pl0, int F, void* workspace, size_t workspace_bytes,
                     dccn_stream_t stream);

/* What the four operators above are about to launch for a geometry (host only, no device work; a sibling of
 * dccn_gemm_route_query below).  The operators take these decisions from the functions the query calls, so a case that is
 * written for one kernel variant can assert that the variant is what its shape runs.
 *   op                      operator                   fields that carry the answer
 *   DCCN_PATCH_FWD          dccn_cconv_patch_fwd       kernel = GEMM; tile_rows x tile_cols x tile_k
 *   DCCN_PATCH_BWD_W        dccn_cconv_patch_bwd_w     kernel = KMAJOR (64x64x64 tiles); splits, klen (the last k range may be shorter)
 *   DCCN_PATCH_BWD_X        dccn_cconv_patch_bwd_x     kernel = GEMM: the wide inverse-stride gather, tile_* as in the forward;
 *                                                      kernel = DX_NARROW (csrc/cconv_dx_narrow.h): col_tiles (1 or 2 tiles of 16
 *                                                      columns), depth (float4s per lane and k group: 1 or 2), bt_lds (1: the
 *                                                      flipped weights staged in LDS, 0: read from global memory), taps_fastest
 *                                                      (1: the k walk runs over the taps fastest), phases (sL * sW), tiles (64
 *                                                      positions each, over all phases), grid (persistent blocks)
 *   DCCN_PATCH_BWD_1D       dccn_cconv1d_bwd           kernel = CONV1D_FUSED: positions (owned per chunk), chunks (per batch
 *                           (Wd = Wo = ntw = sW = 1)   item), items (B * chunks), grid (persistent blocks)
 * Fields an operator does not decide are 0.  Returns DCCN_ERR_INVALID_ARG, *plan untouched, exactly where the operator refuses
 * the geometry (tap origins and pads, which move none of these decisions, are not part of the query). */
enum { DCCN_PATCH_FWD = 0, DCCN_PATCH_BWD_W = 1, DCCN_PATCH_BWD_X = 2, DCCN_PATCH_BWD_1D = 3 };
enum { DCCN_PATCH_KERNEL_GEMM = 0, DCCN_PATCH_KERNEL_KMAJOR = 1, DCCN_PATCH_KERNEL_DX_NARROW = 2, DCCN_PATCH_KERNEL_CONV1D_FUSED = 3 };
typedef struct dccn_cconv_patch_plan {
    int kernel;
    int tile_rows, tile_cols, tile_k;
    int splits, klen;
    int col_tiles, depth, bt_lds, taps_fastest, phases, tiles;
    int positions, chunks, items;
    int grid;
} dccn_cconv_patch_plan;
int dccn_cconv_patch_plan_query(int op, int B, int L, int Wd, int C, int Lo, int Wo, int ntl, int ntw, int sL, int sW, int F,
                                dccn_cconv_patch_plan* plan);

/* The in-graph AWGN monitor branch of the receiver graph (dev/py/radio.py:62-88 AWGN_channel, called at
 * dev/py/ofdmreceiver_np.py:136; tensors `tx_signal:0`, `iq_tx:0`, `iq_rx:0`, `noise_power:0`, :151-152,172-183):
 * tx_signal = complex_clip(x_norm, peak); xn = batch_norm(tx_signal, eps 1e-8)/sqrt(2);
 * noise = (|a| sin p, |a| cos p), a = sqrt(.5) 10^(-SNR/20) N(0,1), p = U(0, 2 pi) (Philox stream keyed by seed/offset);
 * iq_rx = fp16(xn + noise) [frames*pairs, 2], iq_tx = fp16(tx_signal), noise_power = mean |noise|^2.
 * The receiver itself never consumes this branch (`rx_iq_data = iq_tx_re`, :138).  tx_signal / iq_tx / iq_rx nullable. */
size_t dccn_ingraph_awgn_workspace_size(int frames, int pairs_per_frame);
int dccn_ingraph_awgn(const float* x_norm, const float* snr_db, float* tx_signal, uint16_t* iq_tx_f16,
                      uint16_t* iq_rx_f16, float* noise_power, int frames, int pairs_per_frame, float peak,
                      unsigned long long seed, unsigned offset, void* workspace, size_t workspace_bytes,
                      dccn_stream_t stream);

/* ---- classical pilot-aided receivers: dev/m/OFDM_Benchmark_dev.m:339-456 ----------------------
 * The estimator family the "DCCN vs LS / LMMSE" curves are drawn against, as device operators (the contractions -- DFT
 * of the FFT window, pilot interpolation, long-term LMMSE smoothing -- are dccn_dense_fwd[_ld] calls on constant
 * matrices; host mirror dl_ofdm_amd/benchmark_gpu.py, NumPy restatement = oracle: dl_ofdm_amd/benchmark.py).
 * Y [n, S*K, 2] frequency-domain frames, pil [P] / dat [D] flat cell indices (symbol*K + carrier), H [n, S*K, 2] the
 * channel's true response (Perfect / ideal LMMSE only).
 *   dccn_dense_fwd_ld        dccn_dense_fwd with a row stride on x (a column window of wider rows: the FFT window)
 *   dccn_classical_pilot_ls  gp [2][n][P] = Re / Im planes of Y[pilot] / pilot_value          (:345-352 LS at the pilots)
 *   dccn_classical_gain      block partials (left in the workspace for _estimate) of the scalar mapping the unit-gain
 *                            response onto the power-normalised frames and of sum |G_ls|^2; sums4 (nullable, device
 *                            double[4]) = {Re, Im of sum Y_p conj(H_p pv), sum |H_p pv|^2, sum |G_ls|^2}
 *   dccn_classical_estimate  mode 0 LS (planes -> interleaved), 1 ideal per-symbol LMMSE (:353-372), 2 ALMMSE (:437-446),
 *                            3 Perfect, 4 frame mean V [n, K, 2] (input of the PDP variants :399-416); Gls [2][n][S*K].
 *                            ORDER CONTRACT: modes 1 and 3 scale H by the gain whose block partials dccn_classical_gain
 *                            left in the SAME workspace -- call dccn_classical_gain(..., H != NULL, same n, same workspace)
 *                            on the same stream first; without it the partials are whatever the workspace held and G is
 *                            garbage (no error can be raised: the partials carry no tag)
 *   dccn_classical_detect    x = Y / G at the data cells, nearest point of table [m, 2], labels [m, nbits]; det (nullable)
 *                            [n, D, nbits]; errors[0] = bit errors against bits [n, D, nbits]; G rows of g_row cells per
 *                            frame, cell index taken modulo g_mod when g_mod > 0 (one estimate row per frame)      */
size_t dccn_classical_workspace_size(void);
int dccn_dense_fwd_ld(const float* x, int ldx, const float* w, const float* bias, float* y, int M, int K, int N,
                      dccn_stream_t stream);
int dccn_classical_pilot_ls(const float* Y, const int* pil, float* gp, int n, int SK, int P, float pv_re, float pv_im,
                            dccn_stream_t stream);
int dccn_classical_gain(const float* Y, const float* H, const float* Gls, const int* pil, int n, int SK, int P, float pv_re,
                        float pv_im, double* sums4, void* workspace, size_t workspace_bytes, dccn_stream_t stream);
int dccn_classical_estimate(const float* Gls, const float* H, float* G, int n, int S, int K, int mode, float c_var,
                            void* workspace, size_t workspace_bytes, dccn_stream_t stream);
int dccn_classical_detect(const float* Y, const float* G, const int* dat, const float* table, const int* labels,
                          const int32_t* bits, int32_t* det, long long* errors, int n, int SK, int D, int m, int nbits,
                          int g_row, int g_mod, void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* ---- classical receive: the label-free pilot-aided detector of the receive path as ONE launch -------------------------
 * Frames as the front end writes them -> FFT window -> pilot LS -> interpolation -> (ALMMSE) -> one-tap equalisation -> hard
 * bits packed as the receive path packs them (see "receive path"), plus max-log LLRs.  No labels, no true SNR, no workspace, no
 * atomics; no frame depends on another, a frame's outputs do not depend on how many frames the call carries, and two runs give
 * the same bits (every sum runs in the fixed order dl_ofdm_amd/csrc/classical_receive.h states).  Host mirror:
 * dl_ofdm_amd/classical_receive.py.  Per frame f of x [frames, S, K+CP, 2] (fp32):
 *   1. FFT window  xw[s, t] = x[f, s, win + t], t < K, 0 <= win <= CP;  Y[s] = xw[s] . dft with the caller's real-expanded
 *      matrix dft [2K, 2K] (rows / columns 2t, 2t+1 = I, Q; the phase ramp of the window position folded in by the host)
 *   2. LS at the pilots  gp[j] = Y[pil[j]] / pv                      (the expressions of dccn_classical_pilot_ls)
 *   3. interpolation     Gls[c] = sum_j gp[j] w[j, c],  w [P, S*K] real (any such matrix)
 *   4. noise             noise_var > 0: that value for every frame;  noise_var == 0: nv[f] = max(mean_{c in empty} |Y[c]|^2,
 *      1e-20) over the caller's list empty [E] (the guard and DC cells of the reference grid).  The floor keeps the LLRs of a
 *      noise-free frame finite while |G|^2 (d0 - d1) < 3e18.  c = nv / |pv|^2.  (With a prefix shorter than the channel the
 *      empty cells also hold the inter-symbol interference: the estimate then reads high -- 1.8x at CP = 4 on ETU, 30 dB.)
 *   5. estimate          mode 0 (LS): G = Gls;  mode 2 (ALMMSE): v[k] = mean_s Gls[s, k], e = sum_k |v[k]|^2 / S,
 *      G[s, k] = v[k] e / (e + c)                                    (the expressions of dccn_classical_estimate)
 *   6. decision at dat [D]: xh = Y / G, d_q = |xh - table[q]|^2 (the expressions of dccn_classical_detect: the hard decision
 *      is bit for bit that entry's on this call's y_freq and chest), best = first minimum, hard = labels[best];
 *      llr[b] = (|G|^2 / nv) (min_{labels[q,b]=0} d_q - min_{labels[q,b]=1} d_q), positive = bit 1, from the same d_q values
 *      that pick best: llr > 0 => bit 1 and llr < 0 => bit 0 exactly
 *   7. packed uint8 [frames, ceil(D*nbits/8)] in the receive path's row layout; rows need no alignment, padding bits are 0
 * Outputs: packed (required); llr [frames, D, nbits], chest [frames, S*K, 2] (= G), y_freq [frames, S*K, 2] (= Y),
 * noise [frames] (= nv): each nullable.  table [m, 2], labels [m, nbits] (0 / non-zero), m = 2^nbits.
 * pil / dat / empty are device lists the host cannot look into: every entry is clamped to [0, S*K).
 * sizeof(dccn_classical_receive_args) == 160.
 * dccn_classical_receive_supported: 1 exactly where the call is accepted for the shape with 16-byte aligned buffers and valid
 * scalars: 1 <= S <= 16, K a multiple of 16, K + CP even, P, D, E >= 1, nbits 1..4, and the block's LDS (16 (4K + 4) + 2 (16/S) P
 * + 32 floats) within 48 KB -- the reference grids at N = 64 (CP 16 and 4) and N = 128 (CP 32) among them.
 * Refused with DCCN_ERR_INVALID_ARG before anything is launched, nothing written: an unsupported shape; frames < 1; win outside
 * [0, CP]; mode other than 0 / 2 (the other estimators need the true channel); noise_var negative or not finite; pv zero or not
 * finite; m != 2^nbits; a NULL dft, w, pil, dat, empty, table, labels, x or packed; x off a 16-byte boundary, chest / y_freq /
 * table off an 8-byte one, any other pointer off a 4-byte one.  Inside a chain group DCCN_ERR_UNSUPPORTED. */
typedef struct dccn_classical_receive_args {
    int frames, S, K, CP, P, D, E, nbits, m, win, mode;
    float noise_var, pv_re, pv_im;
    const float* dft;
    const float* w;
    const int* pil;
    const int* dat;
    const int* empty;
    const float* table;
    const int* labels;
    const float* x;
    unsigned char* packed;
    float* llr;
    float* chest;
    float* y_freq;
    float* noise;
} dccn_classical_receive_args;
int dccn_classical_receive_supported(int S, int K, int CP, int P, int D, int E, int nbits);
int dccn_classical_receive(const dccn_classical_receive_args* args, dccn_stream_t stream);

/* ---- classical receive for several links: up to dccn_chain_group_max() links' detectors in ONE launch ------
 * What dccn_frame_sync_grouped and its kin are for the front end, for the detector behind it: the solo entry's kernel body runs for
 * n_links links in one launch, the link index on a grid dimension and a link's blocks laid out as the solo launch lays them out
 * (ceil(frames / (16 / S)) tiles of whole frames of THAT link; no tile holds frames of two links).  Link i's packed / llr / chest /
 * y_freq / noise are bit for bit what dccn_classical_receive writes for link i's arguments, and n_links == 1 writes what the solo
 * entry writes.  The links travel as a HOST array of n_links descriptors, copied by value into the kernel arguments.
 *   common to the call: frames, S, K, CP, P, D, E;
 *   per link: nbits and m (any mix of BPSK .. 16-QAM in one launch: the kernel switches block-uniformly on the link's nbits),
 *             mode, win, noise_var, pv, and every pointer.  Link i's packed row is ceil(D * nbits_i / 8) bytes.
 * Two links may share any input (x, dft, w, the index lists, the tables).  llr, chest, y_freq and noise are each given for every
 * link or for none.  sizeof(dccn_classical_link) == 136.
 * Plan first, then issue: every link is checked by the solo entry's own rules (dccn_classical_receive_supported(S, K, CP, P, D, E,
 * nbits_i), then win, mode, noise_var, pv, m, NULLs and alignments), and the call adds: n_links outside
 * 1 .. dccn_chain_group_max(); links NULL; frames < 1; an output given for some links only; any output range of one link (packed,
 * llr, chest, y_freq, noise) overlapping an output range or an input range of ANOTHER link -- all DCCN_ERR_INVALID_ARG.  A refused
 * call launches nothing and writes nothing for any link.  Inside a chain group DCCN_ERR_UNSUPPORTED, as the solo entry.  No
 * workspace, no atomics, every sum in the solo entry's order: two runs give the same bits. */
typedef struct dccn_classical_link {
    int nbits, m, mode, win;
    float noise_var, pv_re, pv_im;
    const float* dft;
    const float* w;
    const int* pil;
    const int* dat;
    const int* empty;
    const float* table;
    const int* labels;
    const float* x;
    unsigned char* packed;
    float* llr;                /* nullable (for all links or none) */
    float* chest;              /* nullable (all or none) */
    float* y_freq;             /* nullable (all or none) */
    float* noise;              /* nullable (all or none) */
} dccn_classical_link;
int dccn_classical_receive_grouped(int n_links, const dccn_classical_link* links, int frames, int S, int K, int CP, int P, int D,
                                   int E, dccn_stream_t stream);

/* One row of the sweep table {c00,c01,c10,c11,ce_sum,count} (float64, device): row6 += the metrics record of the
 * last step, stream-ordered, no host round trip (dev/py/ofdmreceiver_np.py:80-85 accumulates the same on the host). */
int dccn_metrics_table_add(const dccn_metrics* metrics, double* row6, dccn_stream_t stream);
/* acc3[0] += metrics->ce_mean; acc3[1] += *tx_power; acc3[2] += *noise_power (each nullable): the per-step monitors of the
 * training loop (dev/py/ofdmreceiver_np.py:222-229) accumulated on the device in one stream-ordered launch. */
int dccn_step_monitor_add(const dccn_metrics* metrics, const float* tx_power, const float* noise_power, float* acc3,
                          dccn_stream_t stream);
/* row6 = the record (the one-point table of a single evaluation: no clearing launch needed in front of it) */
int dccn_metrics_table_set(const dccn_metrics* metrics, double* row6, dccn_stream_t stream);

/* Kernel-configuration knobs for experiments and profiling.  The table is a process-wide set of DEFAULTS; a call copies it once
 * when it begins (never mid-plan), and a plan that captured its own table (dccn_tuning_snapshot -> dccn_rx_buffers.tuning /
 * dccn_eq_buffers.tuning) is not affected by later changes at all.
 *  0 dense forward with the tail in its epilogue (> 0 on; 0: separate launches)
 *  1 grouped dense backward: 0 = 32x32x2 family; 1-6 = gemm16 dX / dW tile pairs (64x64 / 64x64, 48x64 / 64x64, 64x64 / 64x64
 *    with 64-deep k-tiles, 96x64 / 64x64, 64x128 / 64x128, 64x64 / 64x128) for layers of more than 96 rows and fewer than
 *    2 x CUs 128x128 tiles with vector-legal operands; 7 = k-major dW (default).  8 and above: DCCN_ERR_INVALID_ARG where a
 *    table row would have run, elsewhere as 0
 *  2 C-Conv forward: 0 = 32x32x2 family; 1-6 = gemm16 tiles (32x128, 32x128 with 32x32 waves, 16x128, 64x64, 16x128 on 8
 *    waves, 32x64); 7 = staged whole-k tile (default), 8 / 9 its other store slots, 10 / 11 its 32x128 tiles.  12 and above: as 0
 *  3 C-Conv weight gradient: 0 = 32x32x2 family; 1-4 = gemm16 tiles (64x64, 32x64, 80x128, 32x128), taken only by the receiver
 *    step's own launch (outputs up to 512 x 512); 7 = k-major (default).  5, 6, 8 and above: the step returns
 *    DCCN_ERR_INVALID_ARG where a table row would have run; dccn_cconv_gemm_bwd_w runs them as 0
 *  4 / 5 split-K counts of the two weight gradients (0 = automatic; cut to the slab capacity: 8 / 128)
 *  6 minimum LDS per block in KiB      7 single-tile launches for short k ranges (default 1)
 *  8 GEMMs of at most 96 rows: 0 = as every other; 1-4 = skinny gemm16 tiles (16x64 = default, 32x64, 32x32, 16x64 on 8 waves)
 *    where the few-row tiles of knob 21 do not apply; any value > 0 also enables those and the one-grid backward of knob 17.
 *    5 and above: DCCN_ERR_INVALID_ARG where a skinny tile would have run
 *  (dccn_gemm_route_query answers which of these a shape takes)
 *  9 grouped backward of large layers      10 gemm16 tiles for the un-fused dense forward
 * 11 C-Conv weight gradient in the epilogue of the dense dX tiles (default 1)      12 wave priority of those tiles
 * 13 fused dense + tail launch for 8-QAM / 16-QAM steps (bit 0 lane-per-cell forms, bit 1 quad-lane training form)
 * 14 graded k ranges of the dense weight-gradient items in the fused backward launch (presets 1-24, default 14 = {9,5,2,2,1}/19;
 *    0, 25 and above, or fewer than 768 frames: the uniform split plan)
 * 17 few-row dense backward as one grid (default 1)
 * 18 R0 of the next batch on the backward launch of double-buffered pipelined steps (default 0)
 * 19 equaliser step: element-wise stages in GEMM stores (1 few-row tiles, 2 = default: also larger batches)
 * 20 equaliser step plan (1 = default: grouped corr/eq C-Convs, concat / split in GEMM stores, ONE job-table optimizer launch;
 *    0 = launch per stage; 3 = plan 1 without the fused pilot bottleneck)
 * 21 few-row GEMMs (<= 96 rows) on one-latency 16x16 tiles (default 1)
 * 24 equaliser step: Adam updates of dense_3 / dense_4 and the smoothing kernel's fold ride behind the bottleneck backward launch
 * 25 large layers: the dense kernel's optimizer update on the library's own low-priority stream (0 off, 1 on, 2 = default: with
 *    non-temporal loads and stores)
 * 27 (default 1) large layers' fused dense + tail: a short last row tile (<= 32 of 80 rows) runs as 32x64 blocks in the same grid
 * Keys 15, 16, 22, 23, 26 were removed in round 6 (alternatives that were built, measured without gain and deleted): setting
 * them returns DCCN_ERR_INVALID_ARG.  Set knobs before workspaces are sized. */
int dccn_set_tuning(int key, int value);
int dccn_get_tuning(int key);
/* the knobs as a table (n >= dccn_tuning_count() ints; returns the count): what a plan captures to be immune to later
 * dccn_set_tuning calls -- see dccn_rx_buffers.tuning */
int dccn_tuning_count(void);
int dccn_tuning_snapshot(int* table, int n);

/* Plan queries: which launch plan the library will take for a shape under the current knobs, so that callers size
 * their buffers from the library's own rule instead of restating it.
 *   dccn_dense_tail_supported   1: dccn_dense_tail_fwd[_bwd] accepts (M, K, N, nbits) with 16-byte aligned operands
 *                               (the fused receiver step then runs R2..R6 as one launch and `z` may be NULL);
 *   dccn_rx_bwd_fused_supported 1: the training step runs its backward half as one launch (dense dX tiles with the
 *                               C-Conv weight gradient in their epilogue + dense dW items): `dfft` may be NULL.
 *   dccn_dense_tail_grid        which grid dccn_dense_tail_fwd[_bwd] (and, for nbits <= 2, dccn_dense_decide_fwd) launches for
 *                               (M, K, N, nbits) with 16-byte aligned operands: *grid = 0 uniform tiles, 1 few-row 16x16 tiles,
 *                               2 ragged (80x64 tiles + one row of 32x64 blocks); *tile_rows = 48 or 80 (16 for the few-row
 *                               tiles); *ragged_rows = rows of the short last tile row of the ragged grid, else 0; *blocks =
 *                               blocks of the launch.  Outputs are nullable.  Host-only, launches nothing.  Returns
 *                               DCCN_ERR_INVALID_ARG, outputs untouched, exactly where dccn_dense_tail_supported answers 0. */
int dccn_dense_tail_supported(int M, int K, int N, int nbits);
int dccn_dense_tail_grid(int M, int K, int N, int nbits, int* grid, int* tile_rows, int* ragged_rows, int* blocks);

/* Which launch a stand-alone GEMM-shaped operator issues for a shape under the current knob table, with 16-byte aligned
 * operands.  Host-only: launches nothing.  The operators decide their launch from the same route value this reports.
 *   op, (d0 .. d4)                       operator
 *   DCCN_ROUTE_DENSE_FWD     (M, K, N)               dccn_dense_fwd
 *   DCCN_ROUTE_DENSE_BWD_X   (M, K, N)               dccn_dense_bwd_x
 *   DCCN_ROUTE_DENSE_BWD_W   (M, K, N)               dccn_dense_bwd_w
 *   DCCN_ROUTE_DENSE_BWD     (M, K, N)               dccn_dense_bwd / dccn_dense_bwd_slabs (grouped dX + dW)
 *   DCCN_ROUTE_CCONV_FWD     (rows, kin, F)          dccn_cconv_gemm_fwd
 *   DCCN_ROUTE_CCONV_BWD_W   (rows, kin, F)          the C-Conv weight gradient as the receiver's training step launches it (the
 *                                                    tail's slab reduction rides on the launch, the optimizer launch folds the
 *                                                    slabs); dccn_cconv_gemm_bwd_w itself never takes the gemm16 rows of knob 3
 *   DCCN_ROUTE_RX_BACKWARD   (batch, S, kin, F, D)   dccn_rx_backward
 * unused d's are ignored.  family:
 *   DCCN_FAMILY_GENERIC         gemm_f32_mfma.h: 64x64 tiles, k-tiles 64 (or 32) deep, or the whole k range (tile_k = K) as
 *                               one tile; 128x128x32 when that still gives two blocks per CU
 *   DCCN_FAMILY_GEMM16          a row of the knob's gemm16 table (variant = the row; the 48x64 tiles of knob 10: variant 0)
 *   DCCN_FAMILY_SKINNY          <= 96 rows: the small gemm16 tiles of knob 8 (variant 1-4).  DENSE_BWD: dX on 16x64 tiles and
 *                               the unsplit dW on 64x64 tiles in one grid
 *   DCCN_FAMILY_FEWROW          <= 96 rows: one-latency 16x16 tiles (tile_k = the k depth in 64-k slots x 64).  DENSE_BWD: dX
 *                               on them and the unsplit dW in one grid
 *   DCCN_FAMILY_KMAJOR          split-K weight gradient in the k-major form, 64x64 tiles
 *   DCCN_FAMILY_STAGED          staged whole-k C-Conv forward (variant 7-11)
 *   DCCN_FAMILY_GROUPED_BIG     DENSE_BWD: dX and dW on 128x128x32 tiles in one grid
 *   DCCN_FAMILY_GROUPED_KMAJOR  DENSE_BWD: dX on 64x64x64 tiles and the k-major dW items in one grid
 *   DCCN_FAMILY_GROUPED         DENSE_BWD: dX and dW on 64x64x64 tiles in one grid
 *   DCCN_FAMILY_TWO_LAUNCH      DENSE_BWD: the DENSE_BWD_W route, then the DENSE_BWD_X route, as two launches
 *   DCCN_FAMILY_RX_FUSED        the fused backward launch of rx_bwd.h
 * tile_rows x tile_cols: the output tile (of dX where a grid holds both); w_tile_rows x w_tile_cols: the dW tile of a grouped
 * grid, else 0; tile_k: k-tile depth; splits: k ranges of the weight gradient (1 elsewhere; > 1: slabs that a later launch
 * sums); klen: length of a k range, the last one may be shorter (RX_BACKWARD with graded ranges: the uniform plan's, unused);
 * nranges / koff: RX_BACKWARD with graded dW ranges (knob 14): their count (= splits) and the nranges + 1 offsets into the
 * batch, else 0.
 * Returns DCCN_ERR_INVALID_ARG, *route untouched, exactly where the operator refuses the shape or the knob value (a table-backed
 * knob one past its last row where that row would have run). */
enum {
    DCCN_ROUTE_DENSE_FWD = 0, DCCN_ROUTE_DENSE_BWD_X = 1, DCCN_ROUTE_DENSE_BWD_W = 2, DCCN_ROUTE_DENSE_BWD = 3,
    DCCN_ROUTE_CCONV_FWD = 4, DCCN_ROUTE_CCONV_BWD_W = 5, DCCN_ROUTE_RX_BACKWARD = 6
};
enum {
    DCCN_FAMILY_GENERIC = 0, DCCN_FAMILY_GEMM16 = 1, DCCN_FAMILY_SKINNY = 2, DCCN_FAMILY_FEWROW = 3, DCCN_FAMILY_KMAJOR = 4,
    DCCN_FAMILY_STAGED = 5, DCCN_FAMILY_GROUPED_BIG = 6, DCCN_FAMILY_GROUPED_KMAJOR = 7, DCCN_FAMILY_GROUPED = 8,
    DCCN_FAMILY_TWO_LAUNCH = 9, DCCN_FAMILY_RX_FUSED = 10
};
typedef struct dccn_gemm_route {
    int family, variant;
    int tile_rows, tile_cols, tile_k;
    int w_tile_rows, w_tile_cols;
    int splits, klen;
    int nranges, koff[9];
    int stage;          /* element-wise stage riding in the stores (the equaliser step's calls); the query: always 1 = none */
} dccn_gemm_route;
int dccn_gemm_route_query(int op, int d0, int d1, int d2, int d3, int d4, dccn_gemm_route* route);

/* ---- R7: optimizer -----------------------------------------------------------------
 * dev/py/ofdmreceiver_np.py:185-189  exponential_decay(1e-3, step, 500, 0.98, staircase)
 * + tf.train.AdamOptimizer (TF 1.15 ApplyAdam kernel form).  All state lives on the
 * device so a captured step can be replayed without host-side parameter changes.
 *   state: device dccn_adam_state (global_step, beta powers; advanced by the call)
 *   param/grad/m/v [n]: flat arenas
 *   reg_coef [n] (nullable): per-element L2 coefficient c; the gradient used is
 *       g + (*reg_gate) * c * param    (reg_gate: device float*, nullable -> 1.0).
 *       The receiver passes c = REG_COEFF*2*0.01 on regularised tensors and
 *       reg_gate = &metrics->berlin  (ofdmreceiver_np.py:171). */
typedef struct dccn_adam_state {
    float global_step;         /* float32 variable, ofdmreceiver_np.py:185 */
    float beta1_power;
    float beta2_power;
    float alpha;               /* lr_t used by the most recent step (output) */
} dccn_adam_state;

typedef struct dccn_adam_hparams {   /* host struct, passed by value */
    float lr0, decay_steps, decay_rate;    /* 1e-3, 500, 0.98 */
    float beta1, beta2, eps;               /* 0.9, 0.999, 1e-8 */
} dccn_adam_hparams;

int dccn_adam_tf_step(float* param, const float* grad, float* m, float* v,
                      const float* reg_coef, const float* reg_gate,
                      dccn_adam_state* state, dccn_adam_hparams hp, long long n,
                      dccn_stream_t stream);

/* ---- the fused receiver step -------------------------------------------------------
 * dev/py/ofdmreceiver_np.py:234 (session.run(train_op...)) and :80 (evaluation run):
 * R0 -> R1 -> R2 -> R3..R6 [-> backward -> R7] as one stream-ordered launch sequence
 * (optionally captured into a hipGraph and replayed).
 *
 * Parameter arena layout (floats), F2 = 2F, m = 2^nbits:
 *   conv_w [kin,F2] | conv_b [F2] | dense_w [S*F2, 2D] | dense_b [2D] | tailp
 * dccn_rx_param_offsets() fills offsets[6] = {conv_w, conv_b, dense_w, dense_b, tail, total}. */
typedef struct dccn_rx_shape {
    int batch;     /* frames (Bf) */
    int S;         /* OFDM symbols per frame (7) */
    int kin;       /* samples per symbol seen by the C-Conv (N+CP, or N when cp=False: the caller crops the cyclic prefix, or
                      hands the step a gen_next descriptor, which then reads the N samples behind the prefix itself) */
    int F;         /* nfilter */
    int D;         /* data cells per frame (frame_size) */
    int nbits;     /* 1..4 */
} dccn_rx_shape;

/* The fused device-side generator: a whole batch of any channel of rayleigh_chan_lte on the N = 64 grid, at either cyclic
 * prefix length of the reference driver (CP = 16 / CP = 4: dccn_gen_static_supported), in ONE launch (the chain of dccn_ofdm_tx_frames + dccn_channel_awgn / _doppler_awgn / _groups_awgn below; csrc/datagen.h
 * gen_static_frames_kernel, gen_doppler_frames_kernel): label bits -> resource grid -> ifft + cyclic prefix -> per frame
 * either static Rayleigh taps and the 'same' FIR, or (Doppler frames) Jakes taps per symbol and the per-symbol FIR with n_taps
 * samples of history (dev/py/util.py:25-29, ofdm.py:328-380, radio.py:352-407, 438-452) -> y, plus the frame-scaled noise of
 * radio.py:513-526 and per-block partial sums of |y|^2 and |noise|^2.  It covers the single-profile channels, static or
 * mobile (every frame a Doppler frame), and the frame-interleaved mixRayleigh / mixAll with or without their Doppler frames
 * (every 3rd / 4th frame): the reference driver's default training channel.  Descriptors without Doppler frames launch the
 * code they launched before that was added.
 * CALLERS MUST ZERO-INITIALISE THE STRUCT (memset / = {0}): fields added later sit in what used to be padding, and all-zero
 * new fields mean the earlier behaviour, bit for bit.  The receiver's input is
 * x = y / sqrt(mean |y|^2 over the batch) + noise: formed by the consumer -- dccn_rx_train_step reads the descriptor as the
 * virtual input of its pipelined normalisation (dccn_rx_buffers.gen_next) -- or materialised by dccn_gen_static_apply.
 * Same Philox streams and draws as the separate launches (a batch is a pure function of (seed, offset)); the ifft runs on
 * 16x16x4 MFMA tiles instead of the 32x32x2 GEMM, so tx / y agree with that path to rounding, not bit for bit.
 * All pointers are device pointers; power_partial / noise_partial hold dccn_gen_static_partials(frames) doubles. */
typedef struct dccn_gen_static {
    int32_t* bits_out;            /* [frames, D, nbits] labels drawn here */
    const int32_t* cell_map;      /* [S*K] >= 0 data-cell index, -1 pilot, -2 empty */
    const float* const_tab;       /* [2^nbits, 2] */
    float pilot_re, pilot_im;
    const float* idft;            /* [2K, 2(K+CP)] real form of ifft + cyclic prefix */
    const float* coeff;           /* [n_taps] tap amplitudes (null when identity) */
    const float* alpha;           /* [n_taps, L] sinc interpolation */
    int n_taps, L, identity;      /* identity: AWGN channel (g = [1]) */
    float Fd;                     /* the single profile's Doppler frequency in Hz (read when doppler_period > 0) */
    const float* snr_db;          /* [frames] */
    float* y;                     /* [frames, S, K+CP, 2] channel output */
    float* noise;                 /* [frames, S, K+CP, 2] noise, already scaled per frame */
    double* power_partial;        /* [partials] */
    double* noise_partial;        /* [partials], nullable */
    float* noise_power_out;       /* device float[1], nullable: `noise_power:0`, written by the consumer that sums noise_partial */
    float* tx_out;                /* [frames, S, K+CP, 2], nullable: the transmitted frames (tests) */
    int frames, S, K, CP, D, nbits;
    unsigned long long seed;
    unsigned offset;
    /* Frame-interleaved static profiles ('mixRayleigh' without Doppler frames, dev/py/radio.py:438-452): frame f runs profile
       f % n_profiles of `profiles` (a HOST array of at most 6, read during the call); n_profiles = 0: the single profile
       (coeff, alpha, n_taps, L, identity) above.  tap_stride: taps per frame in the Philox index of the tap draws (0 = n_taps;
       16 reproduces the draws of dccn_channel_groups_awgn). */
    int n_profiles, tap_stride;
    /* Doppler frames (radio.py:376-407): 0 none; 1 every frame (single-profile mobile channels); p: the frames with
       f % p == 0 (3 for mixRayleigh, 4 for mixAll with `mix`).  Such a frame is a Doppler frame when its profile is not the
       identity and has Fd > 0.1; its phases are Philox stream 3 at index ((f*2 + c)*48 + n)*tap_stride + k (the draws of
       dccn_channel_doppler_awgn with tap_stride = n_taps, of dccn_channel_groups_awgn with 16).  Nonzero: t_sym > 0 and every
       Fd finite, else the descriptor is refused. */
    int doppler_period;
    const struct dccn_gen_profile* profiles;
    /* nullable: H [frames * h_rep, K, 2] = fft(g, K) of every frame's impulse response, h_rep copies per frame (the mixed
       channels report the response per symbol: h_rep = S) -- the values dccn_channel_awgn / _groups_awgn put into `H` */
    /* a Doppler frame writes S DISTINCT responses [f, s, K]: a descriptor with Doppler frames and H_out needs h_rep == S
       (refused otherwise); its static frames keep writing h_rep copies */
    float* H_out;
    int h_rep;
    float t_sym;                  /* seconds per OFDM symbol, (K + CP) / Fs (read when doppler_period > 0) */
} dccn_gen_static;
typedef struct dccn_gen_profile {
    const float* coeff;           /* [n_taps] (null when identity) */
    const float* alpha;           /* [n_taps, L] */
    int n_taps, L, identity;
    float Fd;                     /* this profile's Doppler frequency in Hz (was `reserved`: a float's zero is the int's zero) */
} dccn_gen_profile;
/* 1: shapes the fused launch is instantiated for -- the N = 64 grid of 7 symbols at the long cyclic prefix (7, 64, 16) and at
 * the short one (7, 64, 4); 0 for everything else (such a descriptor is refused with DCCN_ERR_INVALID_ARG, nothing launched) */
int dccn_gen_static_supported(int S, int K, int CP);
int dccn_gen_static_partials(int frames);
int dccn_gen_static_frames(const dccn_gen_static* g, dccn_stream_t stream);
/* x_out [frames, S, K+CP, 2] = y / sqrt(mean |y|^2) + noise; noise_power (nullable) = mean |noise|^2.  Writes exactly
 * frames * S * (K+CP) * 2 floats: a cp=False receiver's [frames, S, K, 2] buffer takes dccn_gen_static_apply_window. */
int dccn_gen_static_apply(const dccn_gen_static* g, float* x_out, float* noise_power, dccn_stream_t stream);
/* The same batch as a cp=False receiver sees it (dev/py/model.py:1236-1240 slices the cyclic prefix off inside the graph):
 * x_out [frames, S, K, 2], x_out[f, s, 0:K] = y[f, s, CP:CP+K] / sqrt(mean |y|^2) + noise[f, s, CP:CP+K].  The mean is still
 * taken over the WHOLE frames, prefix included, so the result is dccn_gen_static_apply's output cropped, bit for bit; noise_power
 * is the same value too.  Refused like dccn_gen_static_apply (DCCN_ERR_INVALID_ARG); inside a chain group DCCN_ERR_UNSUPPORTED
 * (the launch carries no chain table). */
int dccn_gen_static_apply_window(const dccn_gen_static* g, float* x_out, float* noise_power, dccn_stream_t stream);
/* dccn_gen_static_apply followed by dccn_frame_sync (below: window W, out_kin = K+CP or K) as ONE launch, for training loops that
 * align every generated batch: x is formed in LDS, the estimator runs on it and the rotated frame is written once.  x_out
 * [frames, S, out_kin, 2], offset int32 [frames] and noise_power carry the bits of that two-launch sequence on the same
 * descriptor.  H_inout (nullable): the [frames, h_rep, K, 2] responses the generator launch wrote (dccn_gen_static.H_out,
 * h_rep = 1 or S), multiplied in place by exp(+2 pi i k offset / K) per column k -- the response of the frame as aligned.
 * dccn_gen_static_apply_sync_supported (host only) = dccn_gen_static_supported && dccn_frame_sync_supported.
 * Refused with DCCN_ERR_INVALID_ARG before anything is launched: a descriptor dccn_gen_static_apply refuses; W or out_kin that
 * dccn_frame_sync refuses; x_out or offset NULL; x_out off a 16-byte boundary or overlapping g->y / g->noise; H_inout with
 * h_rep neither 1 nor S.  Inside a chain group DCCN_ERR_UNSUPPORTED (the launch carries no chain table). */
int dccn_gen_static_apply_sync_supported(int S, int K, int CP, int W);
int dccn_gen_static_apply_sync(const dccn_gen_static* g, int W, int out_kin, float* x_out, int32_t* offset, float* H_inout,
                               int h_rep, float* noise_power, dccn_stream_t stream);

typedef struct dccn_rx_buffers {
    const float* x;            /* [batch, S, kin, 2] raw input (tx_ofdm) */
    const int32_t* bits;       /* [batch, D, nbits] labels (bits_in) */
    float* params;             /* parameter arena */
    float* grads;              /* gradient arena (train only) */
    float* adam_m;             /* train only */
    float* adam_v;             /* train only */
    float* reg_coef;           /* [total] per-element L2 coefficient (train only) */
    dccn_adam_state* adam;     /* train only */
    float* x_norm;             /* [batch, S, kin, 2]  `input:0` */
    float* fft_out;            /* [batch, S, F, 2]    `receiver/fft_like/fft_out:0` */
    float* z;                  /* [batch, 2D] (nullable for nbits <= 2: the fused dense+tail launch skips it) */
    float* prob;               /* [batch, D, nbits, 2] `output:0` (nullable) */
    float* dz;                 /* [batch, 2D] train only */
    float* dfft;               /* [batch, S, F, 2] train only (nullable when dccn_rx_bwd_fused_supported: the dense dX
                                  tiles then only feed the C-Conv weight gradient in their own epilogue) */
    dccn_metrics* metrics;     /* ce_mean / conf_matrix / linear_ber / log_ber */
    float* tx_power;           /* device float[1] `tx_power:0` (nullable: skip R8) */
    void* workspace;
    size_t workspace_bytes;
    /* Software pipelining of R0 across training steps (both default 0 = every step normalises its own batch first):
       x_next != NULL  the step also normalises x_next into x_norm behind its Adam update (the leading blocks of the
                       optimizer launch; x_norm is dead by then), for the following call;
       x_prenormalised x_norm (and the R8 partial sums in the workspace) already hold this step's batch -- written
                       by the previous call through x_next -- so the step starts at R1.
       x itself is only read by R0: with both set, x and x_next may be the same buffer, refilled between calls.
       The workspace must be the same memory in both calls. */
    const float* x_next;
    int x_prenormalised;
    /* Double-buffered form of the same pipelining (dccn_rx_norm_rides_backward(shape) == 1): with x_norm_next != NULL the
       normalisation of x_next is written to x_norm_next by leading blocks of the BACKWARD launch of this step -- hidden
       behind 30 us of matrix work instead of stretching the optimizer launch -- and the caller passes that buffer as
       x_norm (and norm_slot ^ 1 as norm_slot) in the following call.  norm_slot (0/1) names the R8 partial-sum slot of
       the workspace that belongs to x_norm; x_norm is read until the backward launch ends, hence the second buffer.
       Where that query answers 0, x_next + x_norm_next is refused (DCCN_ERR_INVALID_ARG) before anything is launched. */
    float* x_norm_next;
    int norm_slot;
    /* Large layers (dccn_get_tuning(16), N = 1024): the dense kernel's optimizer update runs in the epilogue of its
       weight-gradient tiles and its gradient is not written to `grads` unless keep_dense_grad > 0.
       keep_dense_grad < 0 (round 5): the caller never reads the dense kernel's gradient (a training loop): the optimizer
       launch that sums its split-K slabs does not store the sum either (the other gradients are still written). */
    int keep_dense_grad;
    /* reg_coef holds ONE value over the whole dense-kernel segment (what the reference's keras l2(0.01) regulariser gives:
       dev/py/model.py:1271-1272): the optimizer then reads that value once instead of streaming a parameter-sized array
       (12 % of the optimizer launch's traffic at N = 1024).  0 = per-element coefficients everywhere (the general form). */
    int reg_uniform_dense;
    /* hipEvent_t (nullable) that the launch reading x_next waits for on `stream`: lets a producer fill x_next on ANOTHER
       stream while the forward and backward launches of this step run (the device-side generator: dl_ofdm_amd/datagen.py
       SideStreamFeeder).  Eager launches only (not inside dccn_rx_graph_create). */
    void* x_next_ready;
    /* Round 5: the next batch comes from the fused generator (host pointer to a descriptor, read during the call only): the
       step issues the generator launch as its FIRST launch and its last launch normalises (y, noise, partials) as if they were
       x_next = y / sqrt(mean |y|^2) + noise (bit-identical to normalising the materialised batch).  x_next, when non-null as
       well, receives that batch (tx_ofdm); the labels go to gen_next->bits_out (the caller's OTHER label slot).  Training
       calls on the single-buffer pipelining only (dccn_rx_norm_rides_backward(shape) == 0); one C call per generated-and-
       trained batch.
       shape.kin == K + CP: the step reads the generator's whole symbols.  shape.kin == K (a cp=False receiver): its last launch
       reads the K samples behind the cyclic prefix of every symbol -- the batch power still that of the whole frames -- which is
       bit-identical to normalising dccn_gen_static_apply_window's output; x_next, when given, is [batch, S, kin, 2] either way.
       Any other kin is refused (DCCN_ERR_INVALID_ARG) before anything is launched. */
    const dccn_gen_static* gen_next;
    /* nullable: the plan's OWN tuning table (dccn_tuning_count() ints, captured with dccn_tuning_snapshot when the plan was
       built): the call plans its launches from it instead of the process-global knobs, so dccn_set_tuning on another thread
       cannot change this plan.  NULL: the globals as they stand when the call begins (copied once: never mid-call). */
    const int* tuning;
} dccn_rx_buffers;

int dccn_rx_param_offsets(const dccn_rx_shape* shape, long long offsets[6]);
int dccn_rx_bwd_fused_supported(const dccn_rx_shape* shape);
/* 1: dccn_rx_train_step (train != 0) / dccn_rx_eval_step run R2..R6 as ONE launch for this shape -- the dense forward
 * with the demodulation tail in its epilogue -- and `z` may be NULL.  (8-QAM / 16-QAM: the tile is staged through LDS and
 * walked a lane or a quad of lanes per cell; which of those steps take the fused launch is tuning knob 13.) */
int dccn_rx_dense_tail_fused(const dccn_rx_shape* shape, int train);
/* 1: a training step given x_next + x_norm_next normalises the next batch on its backward launch (see dccn_rx_buffers) */
int dccn_rx_norm_rides_backward(const dccn_rx_shape* shape);
/* 1: a training step of this shape takes dccn_rx_buffers.gen_next (the next batch formed from the fused generator's
 * (y, noise, partials) by the pipelined R0 on the optimizer launch): single-buffer pipelining, batch <= 1536 frames, one power
 * partial per generator block.  0: generate with dccn_gen_static_frames / _apply (or the launch-per-stage generator) and hand
 * the batch over as x_next.  A step given gen_next for a shape answering 0 is refused BEFORE anything is launched. */
int dccn_rx_gen_next_supported(const dccn_rx_shape* shape);
/* The backward half of the basic receiver's training step as one launch (small layers, see the query above):
 *   dfft = dz . Wd^T                     (dev/py/model.py:1268-1275 backward; written only when dfft != NULL)
 *   dWd  = fft_out^T . dz, dbd = colsum  (k-major tiles, split-K slabs)
 *   dWeff = x_norm^T . dfft              (dev/py/complex.py:183-192 backward; contracted in the epilogue of the tiles
 *                                         that produce dfft, one [2kin,64] partial per tile)
 * reduce != 0: a second and third launch sum the slabs / fold the partials into dw_dense [S*2F, 2D], db_dense [2D]
 * (nullable), dw_conv [kin, 2F] = [Wa|Wb], db_conv [2F] (nullable); reduce == 0 leaves them in the workspace (what the
 * fused training step does: its optimizer launch reduces them).  x_norm [batch,S,kin,2], fft_out [batch,S,F,2],
 * dz [batch,2D], w_dense [S*2F, 2D]. */
size_t dccn_rx_backward_workspace_size(int batch, int S, int kin, int F, int D);
int dccn_rx_backward(const float* x_norm, const float* fft_out, const float* dz, const float* w_dense, float* dfft,
                     float* dw_dense, float* db_dense, float* dw_conv, float* db_conv, int batch, int S, int kin, int F,
                     int D, int reduce, void* workspace, size_t workspace_bytes, dccn_stream_t stream);
size_t dccn_rx_workspace_size(const dccn_rx_shape* shape, int train);
/* eager launch sequences.
 * Large layers (an unsplit dense weight gradient of >= 512 tiles of 128x128, e.g. N = 1024: a 459 MB dense kernel): the training
 * step forks the dense kernel's optimizer update onto a stream the LIBRARY owns (one per device, lowest priority, created on
 * first use) and joins it before its last launch, so that this 3.2 GB stream runs next to the MFMA-bound C-Conv
 * weight-gradient launch.  Nothing changes for the caller: every effect of the step is ordered on `stream` when the call
 * returns, results are bit-identical, and dccn_rx_graph_create captures the fork and the join with the rest. */
int dccn_rx_eval_step(const dccn_rx_shape* shape, const dccn_rx_buffers* buf, dccn_stream_t stream);

/* ---- receive path: IQ frames -> packed bits and LLRs, no labels ---------------------------------------------------------
 * The forward of the receiver with a decision stage instead of the loss: no bits_in, no cross entropy, no confusion counts,
 * no reduction, no metrics (dev/py/test_v1/test_ofdm_cdnn_awgn.py:113-118 fetches `output:0` from `tx_ofdm:0` alone).
 * Outputs for `frames` frames of D data cells with nbits (1..4) bits:
 *   packed uint8 [frames, ceil(D*nbits/8)]  required.  Row f = numpy.packbits(hard[f].reshape(-1)), hard [frames, D, nbits] in
 *          the layout of bits_in (cell, then bit, most significant bit of the symbol first); most significant bit of a byte
 *          first, padding bits of a row's last byte 0.
 *   llr    float [frames, D, nbits]         nullable.  u1 - u0 of the bit pair's two post-leaky-ReLU logits
 *          (dev/py/model.py:1283-1291) = log(p1 / p0) of output:0; positive means bit 1.
 *   prob   float [frames, D, nbits, 2]      nullable.  output:0, as the evaluation step writes it.
 * The hard decision is argmax over the pair of output:0, first index on ties (dev/py/ofdmreceiver_np.py:166), computed with
 * the expressions of the evaluation step's tail: it is bit for bit the decision that step tallies.  Note: where u1 - u0 is
 * positive but so small that exp(-(u1 - u0)) rounds to 1, p1 == p0 and the bit is 0 although llr > 0.
 * Every entry validates its arguments before it launches anything.
 *
 *   dccn_demod_decide            z [frames, D, 2] + tail weights (dccn_tail_param_count floats) -> packed / llr / prob: one launch,
 *                                no workspace, every nbits, any D (rows of packed need no alignment).
 *   dccn_dense_decide_supported  1: dccn_dense_decide_fwd accepts (M, K, N, nbits) with 16-byte aligned x / w (N = 2 D).
 *                                It does NOT say that z may be NULL: that holds for nbits <= 2 only; for nbits 3 / 4 the call
 *                                is two launches and a NULL z is refused with DCCN_ERR_INVALID_ARG.
 * Alignment (checked, DCCN_ERR_INVALID_ARG otherwise): z and prob 8 bytes; llr 8 bytes at nbits = 2, 16 bytes at nbits = 4,
 * 4 bytes otherwise (a cell's values leave as one vector store); packed: none.
 *   dccn_dense_decide_fwd        z = x [M,K] . w [K,N] + bias and the decision.  nbits <= 2: ONE launch, the decision in the
 *                                GEMM's epilogue; z nullable (not materialised then).  nbits >= 3: the GEMM stores z (required),
 *                                the decision kernel follows.  z has the bits dccn_dense_tail_fwd computes for the same operands. */
int dccn_demod_decide(const float* z, const float* tailp, unsigned char* packed, float* llr, float* prob, int frames, int D,
                      int nbits, dccn_stream_t stream);
int dccn_dense_decide_supported(int M, int K, int N, int nbits);
int dccn_dense_decide_fwd(const float* x, const float* w, const float* bias, float* z, const float* tailp,
                          unsigned char* packed, float* llr, float* prob, int M, int K, int N, int nbits,
                          dccn_stream_t stream);
/* The basic receiver's receive step: R0 -> C-Conv forward -> dense + decision.  Three launches where dccn_rx_receive_fused
 * answers 1 (BPSK / QPSK wherever the evaluation step fuses its tail, up to 1536 frames), one more otherwise.  x_norm and
 * fft_out are bitwise what dccn_rx_eval_step writes for the same x and params.  A buffer set that misses the alignment above, or
 * lacks z where it is needed, is refused (DCCN_ERR_INVALID_ARG) before anything is launched. */
typedef struct dccn_rx_receive_buffers {
    const float* x;            /* [batch, S, kin, 2] */
    const float* params;       /* the receiver's arena (dccn_rx_param_offsets) */
    float* x_norm;             /* [batch, S, kin, 2] */
    float* fft_out;            /* [batch, S, F, 2] */
    float* z;                  /* [batch, 2D]; nullable where dccn_rx_receive_fused answers 1 (not written then unless given) */
    unsigned char* packed;
    float* llr;                /* nullable */
    float* prob;               /* nullable */
    void* workspace;
    size_t workspace_bytes;    /* >= dccn_rx_receive_workspace_size */
    const int* tuning;         /* nullable: a plan's own knob table (dccn_tuning_snapshot), as dccn_rx_buffers.tuning */
} dccn_rx_receive_buffers;
size_t dccn_rx_receive_workspace_size(const dccn_rx_shape* shape);
/* 1: the step runs the dense forward and the decision as ONE launch for this shape under the current knobs: z may be NULL */
int dccn_rx_receive_fused(const dccn_rx_shape* shape);
int dccn_rx_receive_step(const dccn_rx_shape* shape, const dccn_rx_receive_buffers* buf, dccn_stream_t stream);
int dccn_rx_train_step(const dccn_rx_shape* shape, const dccn_rx_buffers* buf,
                       dccn_adam_hparams hp, dccn_stream_t stream);
/* R0 (+R8 partial sums) of buf->x into buf->x_norm, as the first launch of a step does it: primes the pipelined
   mode (x_prenormalised) before its first call.  Workspace = the training step's. */
int dccn_rx_normalise(const dccn_rx_shape* shape, const dccn_rx_buffers* buf, dccn_stream_t stream);
/* hipGraph-captured replay of the same sequences */
typedef struct dccn_rx_graph dccn_rx_graph;
/* mode: bit0 = train (else eval), bit1 = run the dense weight-gradient branch on a forked stream */
int dccn_rx_graph_create(const dccn_rx_shape* shape, const dccn_rx_buffers* buf, int mode,
                         dccn_adam_hparams hp, dccn_stream_t stream, dccn_rx_graph** out);
int dccn_rx_graph_launch(dccn_rx_graph* g, dccn_stream_t stream);
int dccn_rx_graph_destroy(dccn_rx_graph* g);

/* ---- measurement helpers (HIP events on the caller's stream) ------------------------ */
typedef struct dccn_timer dccn_timer;
int dccn_timer_create(dccn_timer** out);
int dccn_timer_start(dccn_timer* t, dccn_stream_t stream);
int dccn_timer_stop(dccn_timer* t, dccn_stream_t stream);
int dccn_timer_elapsed_ms(dccn_timer* t, float* ms);     /* synchronises on the stop event */
int dccn_timer_destroy(dccn_timer* t);
int dccn_stream_synchronize(dccn_stream_t stream);

/* ---- per-step monitors of the equaliser harness (dev/py/ofdmreceiver_np_mp.py:245, 325-333: `chan_rms`; :411-425: the
 * per-epoch means of ce_mean, berlin, tx_power, noise power and chan_rms) in ONE launch -------------------------------
 * chan_rms = mean((LN(chan) - LN(chest))^2), LN = LayerNormalization(axis=1, center=False, scale=False, eps 1e-3) over the
 * OFDM-symbol axis of the [B, S, K, 2] views.  chan is [B, S, K, 2] (chan_per_symbol = 1) or one row per frame [B, K, 2]
 * (static channels: its LN is 0, as in the reference).  acc5 (nullable) += {metrics->ce_mean, metrics->berlin, *tx_power,
 * *noise_power, chan_rms}; rms_out (nullable) = chan_rms.  The workspace (dccn_eq_monitor_workspace_size bytes) must be
 * ZERO before the first call and belongs to the calls of one stream; each call leaves it ready for the next. */
size_t dccn_eq_monitor_workspace_size(int B, int S, int K);
int dccn_eq_monitor_accumulate(const float* chest, const float* chan, int chan_per_symbol, int B, int S, int K,
                               const dccn_metrics* metrics, const float* tx_power, const float* noise_power, float* acc5,
                               float* rms_out, void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* ---- step timeline: in-situ start / end of the launches of dccn_rx_train_step / dccn_rx_eval_step ----------------------
 * Replaces nothing in the reference (TF1 has `RunMetadata` step stats for this: dev/py/ofdmreceiver_np.py:234 runs the
 * step without them); it exists so that a step time can be decomposed into per-launch durations and the gaps between
 * launches on whatever box the step runs on (bench.py `step.boundaries`).
 * `buf` is DEVICE memory of dccn_step_trace_bytes(ring_steps) bytes, zeroed by the caller: a ring of `ring_steps` steps x
 * `launches` slots x `blocks` workgroups x `words` 64-bit words (dccn_step_trace_geometry).  While enabled, every step call
 * takes the next ring entry and thread 0 of each workgroup of its instrumented launches writes
 *   {s_memrealtime at entry (100 MHz), s_memtime at entry (shader cycles), the same two at exit}
 * into [step % ring][slot][blockIdx.x].  Slots: 1 C-Conv forward, 2 dense forward (+ tail), 3 tail (own launch),
 * 4 backward, 5 C-Conv weight gradient (own launch), 6 optimizer; 0 and 7 are never written.  buf = NULL disables (the
 * default: a disabled mark is one scalar compare per workgroup).  Process-wide switch, meant for one measuring thread.
 *   Blocks.  Every workgroup with blockIdx.x < `blocks` and blockIdx.y == blockIdx.z == 0 marks, the workgroups that carry
 *     the tail's slab reduction behind a weight-gradient grid included; the words of a block index at or above the launch's
 *     grid stay as the caller zeroed them.  A split-K launch (z = the k range) therefore leaves gridDim.x stamps, those of
 *     its first k range.  Where a plan issues two launches under one slot on the same stream (the dense weight gradient,
 *     then dX, when they cannot share a grid) the later launch overwrites the block indices the two have in common.
 *   Not instrumented (their time shows as the gap in front of the next slot): R0 and the generator of the next batch in
 *     front of slot 1; the tail's slab reduction where it is a launch of its own (every evaluation step, and training
 *     steps whose dense update runs on the second stream, knob 25) and that update itself; the fold launch behind a C-Conv
 *     weight gradient whose operands are not vector-legal (slot 5 then holds the GEMM alone).
 *   Captured steps are never instrumented: while dccn_rx_graph_create / dccn_eq_graph_create capture, a step takes no ring
 *     entry, counts no step and bakes no pointer into the graph, so replays write nothing whether a trace is enabled at
 *     capture time, at replay time or never.  Only the receiver's training and evaluation steps are traced at all:
 *     dccn_rx_receive_step, the equaliser steps and the stand-alone operators never write.
 *   dccn_step_trace_enable returns DCCN_ERR_WORKSPACE for ring_steps <= 0 or bytes < dccn_step_trace_bytes(ring_steps) (with
 *     a non-null buf) and changes nothing: a trace already in force stays in force, its counter included.  A step call
 *     that is refused (any status but DCCN_OK from its plan) takes no entry and counts nothing. */
size_t dccn_step_trace_bytes(int ring_steps);
int dccn_step_trace_enable(unsigned long long* buf, size_t bytes, int ring_steps);
long long dccn_step_trace_steps(void);                 /* step calls recorded since the last enable */
void dccn_step_trace_geometry(int* launches, int* blocks, int* words);

/* ==== channel-equaliser stage: dev/py/model.py:349-478 =====================
 * The stage's dense / C-Conv layers use dccn_dense_* / dccn_cconv_gemm_* above; these are the
 * remaining operators.  All tensors fp32, IQ pairs interleaved on the last axis. */

/* model.py:363  tf.contrib.layers.layer_norm(center=False, scale=False, begin_norm_axis=1):
 * per-row (sample) y = x*inv + (-mean*inv), inv = rsqrt(var + eps), biased variance over `cols`.
 * mean, inv [rows] nullable (inv is what dccn_layer_norm_bwd needs). */
int dccn_layer_norm_fwd(const float* x, float* y, float* mean, float* inv, int rows, int cols, float eps,
                        dccn_stream_t stream);
int dccn_layer_norm_bwd(const float* dy, const float* y, const float* inv, float* dx, int rows, int cols,
                        dccn_stream_t stream);

/* model.py:421-426  activation=tf.nn.tanh of the channel-estimate dense layer; bwd: dx = dy*(1-y^2). */
int dccn_tanh_fwd(const float* x, float* y, long long n, dccn_stream_t stream);
int dccn_tanh_bwd(const float* dy, const float* y, float* dx, long long n, dccn_stream_t stream);

/* model.py:431-438  eq = y*conj(h)/|h| and corr = eq*conj(eq) over [n_pairs,2] (corr nullable).
 * bwd: cotangents d_eq / d_corr (either nullable) -> dy / dh (either nullable). */
int dccn_equalize_fwd(const float* y, const float* h, float* eq, float* corr, long long n_pairs,
                      dccn_stream_t stream);
int dccn_equalize_bwd(const float* y, const float* h, const float* d_eq, const float* d_corr, float* dy,
                      float* dh, long long n_pairs, dccn_stream_t stream);

/* model.py:465-475  pilot "SNR" monitor: eq [frames,S,K,2], carriers: device int32[P] -> snr_db [frames]
 * = log10(clip(mean/var of |pilot cell|^2, 1e-3, 1e4)). */
int dccn_pilot_snr(const float* eq, const int* carriers, float* snr_db, int frames, int S, int K, int P,
                   dccn_stream_t stream);

/* model.py:428  layers_conv2d_complex(chest, 1, (kL,kW), padding='same') on a one-channel L x W
 * complex image, lowered to a dense layer: expand w [kL,kW,2] (=[Wa|Wb] per tap, the TF kernel
 * [kL,kW,1,1,2]) and bias [2] (nullable) into T [L*W*2, L*W*2] and bias_eff [L*W*2] (nullable);
 * run dccn_dense_fwd/bwd with them; reduce dT / dbias_eff back onto dw [kL,kW,2] / dbias [2]
 * (dbias, dbias_eff nullable). */
int dccn_cconv2d_same_expand(const float* w, const float* bias, float* T, float* bias_eff, int L, int W,
                             int kL, int kW, dccn_stream_t stream);
int dccn_cconv2d_same_reduce(const float* dT, const float* dbias_eff, float* dw, float* dbias, int L, int W,
                             int kL, int kW, dccn_stream_t stream);

/* ---- the fused equaliser transfer-learning step ------------------------------------------------------
 * dev/py/ofdmreceiver_np_mp.py:283-330,414 (session.run(train_op...)) and :87 (evaluation run) as ONE
 * pre-planned launch sequence: R0 normalise -> equalizer_ofdm -> frozen basic receiver -> loss/BER ->
 * backward to the Equalizer/ variables only -> TF Adam on the equaliser arena.  cp = 0: the first dense layer and
 * the receiver read the K samples behind the cyclic prefix (model.py:364-366, 1236-1240).
 * Equaliser parameter arena, TF creation order (floats):
 *   dense k[2n_sc (cp=1) or 2K (cp=0), 2K] b | conv3d k[K,2K] b | dense_1 k[S*K*2,2*pilot_size] b | dense_2 | dense_3 |
 *   dense_4 | conv3d_1 k[S,K,2] b[2] | conv3d_2 k[K,2K] b | conv3d_3 | dense_5 k[4K,2n_sc] b
 * (offsets[0..19] = start of each tensor, offsets[20] = total).  rx_params: the frozen receiver in the
 * dccn_rx_param_offsets layout with kin = K + CP (cp=1) or K (cp=0). */
typedef struct dccn_eq_shape {
    int batch, S, K, CP, cp;      /* frames, OFDM symbols per frame, nfft, cyclic prefix, FLAGS.cp */
    int F, D, nbits;              /* receiver: nfilter, data cells per frame, bits per cell */
    int pilot_size, P;            /* pilot cells per frame (model.py:359), pilot carriers per symbol */
} dccn_eq_shape;

struct dccn_eq_monitor;
/* Every step that takes a dccn_eq_buffers (eager, grouped, or captured by dccn_eq_graph_create) checks all of it first: a
 * call that is refused (any status but DCCN_OK for something the caller passed in) is refused before anything is launched. */
typedef struct dccn_eq_buffers {
    const float* x;               /* [batch,S,n_sc,2] raw `tx_ofdm` */
    const int32_t* bits;          /* [batch,D,nbits] */
    float* eq_params;             /* equaliser arena (updated by the train step) */
    float* eq_grads;              /* train: gradient arena (data term; L2 enters in the optimizer) */
    float* adam_m;
    float* adam_v;
    const float* reg_coef;        /* nullable, see dccn_adam_tf_step (gate = 1) */
    dccn_adam_state* adam;
    const float* rx_params;       /* frozen receiver arena */
    float* out_eq;                /* [batch,S,n_sc,2] equalised receiver input (model.py:463) */
    float* chest;                 /* [batch,S,K,2] channel estimate (model.py:477) */
    float* snr_db;                /* [batch] nullable (model.py:465-475) */
    const int* pilot_carriers;    /* device int32[P], nullable with snr_db */
    float* prob;                  /* [batch,D,nbits,2] nullable */
    dccn_metrics* metrics;
    float* tx_power;              /* device float[1], nullable */
    void* workspace;
    size_t workspace_bytes;
    int reg_uniform;              /* 1: reg_coef holds ONE value over each dense kernel / bias tensor (keras l2(0.01) on every dense
                                     layer, model.py:371-462) and is not consulted for the C-Conv tensors' segments other than
                                     element-wise: the optimizer launch reads one coefficient per dense tensor instead of
                                     streaming a parameter-sized array.  0: per-element coefficients everywhere. */
    const float* rx_folded;       /* nullable: dccn_eq_rx_fold(rx_params) -- the frozen receiver's C-Conv and dense layer as one
                                     matrix.  When given, few-row batches (<= 96 frames) run ONE GEMM where the step ran the two
                                     layers (and one on the way back); must be rebuilt whenever rx_params change. */
    /* Pipelined input normalisation (training, round 4; same idea as dccn_rx_buffers.x_next): the step's first launch -- the
       batch normalisation of `input:0` -- depends on nothing but x, so the PREVIOUS step can run it for this batch on leading
       workgroups of its optimizer launch.
       x_next != NULL   this step also normalises x_next (same shape as x) into the workspace; honoured when
                        dccn_eq_norm_rides(shape) is 1, otherwise ignored
       x_prenormalised  1: the workspace already holds the normalisation of x (and its R8 partial sums in slot norm_slot),
                        written by the previous call through x_next on the SAME workspace: the step starts at the layer norm
       norm_slot        0/1: the R8 partial-sum slot of THIS batch; x_next's sums go to the other one, so consecutive
                        pipelined calls alternate it.  Results are bit-identical to un-pipelined calls. */
    const float* x_next;
    int x_prenormalised;
    int norm_slot;
    /* Round 5: the next batch as the fused generator left it (host pointer to its descriptor, read during the call / at graph
       capture): instead of x_next the optimizer launch normalises y / sqrt(mean |y|^2) + noise formed in registers from
       (y, noise, power_partial) -- the values dccn_gen_static_apply would write, so results keep their bits -- and, when
       noise_partial and noise_power_out are set, finishes the noise-power monitor.  The CALLER issues dccn_gen_static_frames
       for that batch on the same stream before this call (the step itself launches nothing for it: the call stays
       graph-capturable, the generator's per-batch arguments stay outside the graph).  Honoured like x_next. */
    const dccn_gen_static* x_next_virtual;
    const int* tuning;            /* nullable: the plan's own tuning table, as dccn_rx_buffers.tuning */
    /* Round 6: 1 = the step ALSO produces the batch x_next_virtual describes (the descriptor fully armed: bits_out, snr_db,
       offset, seed, H_out ...): the generator's workgroups ride on the step's pilot-bottleneck backward launch (15 us of VALU
       work beside MFMA tiles and HBM streams instead of a launch of its own in front of the step; a launch of its own when the
       plan has no such launch).  The caller no longer issues dccn_gen_static_frames for that batch.  Same draws, same bits.
       A descriptor with Doppler frames does not ride: its generator is the step's own FIRST launch (also for a chain group,
       one launch for all chains).  The bottleneck backward launch keeps the static generator as its only rider: the Doppler
       body needs 54.9 KB of LDS beside that kernel's 10.6 KB and is several times the launch's longest work item.
       A descriptor at the short cyclic prefix (CP = 4) does not ride either, with or without Doppler frames: the rider is the
       (7, 64, 16) instantiation only, so its generator takes the same route -- the step's own first launch.  Same draws,
       same bits as a launch issued by the caller. */
    int gen_next_rides;
    /* Round 6, nullable: the training loop's per-step monitors (dccn_eq_monitor_accumulate: chan_rms of THIS step's channel
       estimate against `chan`, and {ce_mean, berlin, tx_power, noise_power, chan_rms} added onto acc5) as part of the step's
       optimizer launch instead of a launch of their own behind the step.  chest / metrics / tx_power must be the step's own.
       Same additions of the same values: the accumulators keep their bits. */
    const struct dccn_eq_monitor* monitor;
} dccn_eq_buffers;
/* 1: dccn_eq_train_step honours dccn_eq_buffers.x_next for this shape */
int dccn_eq_norm_rides(const dccn_eq_shape* shape);

/* The frozen receiver's linear part folded into one matrix: out [S*2n_sc*2D + 2D] floats = Mf [S*2n_sc, 2D] then bf [2D], with
 * z = out_eq_flat . Mf + bf  ==  dense(C-Conv(out_eq)) of dev/py/model.py:1246-1275 (rows of cyclic-prefix samples are zero
 * when cp = 0).  Valid as long as rx_params do not change (they are frozen: ofdmreceiver_np_mp.py:330 trains Equalizer/ only). */
size_t dccn_eq_rx_folded_floats(const dccn_eq_shape* shape);
int dccn_eq_rx_fold(const dccn_eq_shape* shape, const float* rx_params, float* out, dccn_stream_t stream);

/* offsets[i] = first float of tensor i, offsets[20] = ARENA size.  Every tensor starts on a 16-byte boundary: the arena has
 * up to three floats of PADDING behind a tensor whose element count is not a multiple of four (conv3d_1's two-float bias),
 * so offsets[i+1] - offsets[i] is NOT the tensor's size and offsets[20] is not the parameter count -- take sizes from the
 * shapes above.  The padding floats of eq_params, eq_grads, adam_m, adam_v and reg_coef must be ZERO when the arenas are
 * created (zero gradient and zero Adam state keep them zero): the optimizer launch and the merged element-wise jobs stream
 * over whole arena segments, padding included. */
int dccn_eq_param_offsets(const dccn_eq_shape* shape, long long* offsets /* [21] */);
size_t dccn_eq_workspace_size(const dccn_eq_shape* shape, int train);
/* Where a named intermediate of the fused step lives inside the caller's workspace (the step never reuses a buffer within a
 * call, so every one of them holds what its stage left there when the call returns -- the counterpart of fetching a named
 * tensor of the reference's graph, dev/py/model.py:349-478 by line):
 *   forward   "x_norm" input:0 [B,S,n_sc,2] | "ln" :363 | "t1" :371 dense [B*S,2K] | "y" :378-386 [B,S,K,2] | "d1" :394 [B,2P] |
 *             "d2" :402 | "d3" :408 | "d4" :421 (after tanh) [B,S*K*2] | "T" / "be" the :428 kernel expanded to a dense layer
 *             [SK2,SK2] / [SK2] | "eq" :435 | "corr" :438 | "cat" :456 [B*S,K,4] | "fft" / "z" receiver (unless folded) | "dz"
 *   backward  "dout" d loss / d equalized [B,S,n_sc,2] | "deqc" / "dcorc" gradients of the two :439-449 C-Conv outputs |
 *             "deq" / "dcorr" | "dy" (from the equalise stage only) | "dh" | "dd4" (through the tanh) | "dd3" | "dd2" |
 *             "dflat" (total gradient of y: "dy" + the pilot branch) | "dt1" | "dT" / "dbe"
 * Returns DCCN_OK and (*byte_offset, *count floats), or DCCN_ERR_INVALID_ARG for an unknown name / a training-only tensor of
 * an evaluation workspace.  Which buffers a given launch plan leaves un-written (e.g. "dcat" when the concat's gradient is
 * split in the GEMM's store) is the plan's business: compare only what the plan's description says it materialises. */
int dccn_eq_workspace_tensor(const dccn_eq_shape* shape, int train, const char* name, size_t* byte_offset, size_t* count);
int dccn_eq_eval_step(const dccn_eq_shape* shape, const dccn_eq_buffers* buf, dccn_stream_t stream);
int dccn_eq_train_step(const dccn_eq_shape* shape, const dccn_eq_buffers* buf, dccn_adam_hparams hp,
                       dccn_stream_t stream);
/* The chain's receive step (see "receive path" above): the equaliser forward exactly as dccn_eq_eval_step runs it -- out_eq,
 * chest (and snr_db) are written as that step writes them -- and the frozen receiver with the decision stage in place of the
 * tail: buf->bits, buf->metrics, buf->prob and buf->tx_power may be NULL and are not touched.  Workspace: the evaluation
 * step's.  Several chains per launch sequence: dccn_eq_receive_step_grouped ("chain groups" below).  llr / prob that miss the
 * alignment of the decision stage (see "receive path" above) are refused (DCCN_ERR_INVALID_ARG) before anything is launched. */
typedef struct dccn_receive_out {
    unsigned char* packed;     /* [batch, ceil(D*nbits/8)] */
    float* llr;                /* [batch, D, nbits], nullable */
    float* prob;               /* [batch, D, nbits, 2], nullable */
} dccn_receive_out;
int dccn_eq_receive_step(const dccn_eq_shape* shape, const dccn_eq_buffers* buf, const dccn_receive_out* out,
                         dccn_stream_t stream);
/* ---- chain groups: several independent equaliser training chains carried by ONE launch sequence ------------------------
 * The reference driver trains one (receiver -> equaliser) chain per modulation and per cp / longcp variant, each as an OS process
 * of its own (dev/py/run_local_ofdm.py:61-118, locals.py:28-38; the loop is ofdmreceiver_np_mp.py:394-466).  A 73-frame
 * equaliser step is a chain of ~21 dependent launches that keeps a few percent of an MI355X busy; here n_chains (<=
 * dccn_chain_group_max() = 8) such chains of the SAME shape share every launch: the chain index is a grid dimension and
 * every kernel adds that chain's arena offset to its pointer arguments.  The chains may differ in modulation (nbits): the
 * demodulation tail of the frozen receiver -- the only stage whose kernels depend on it -- is launched once per distinct nbits.
 *
 * Layout contract (checked; DCCN_ERR_INVALID_ARG otherwise): for every pointer field f of dccn_eq_buffers (and of the
 * dccn_gen_static behind x_next_virtual), bufs[g]->f - bufs[0]->f is the SAME byte offset off[g] for all fields, a multiple of
 * 256: each chain keeps ALL its device buffers in one arena with chain 0's internal layout (dl_ofdm_amd/equalizer.py
 * ChainArena).  `prob` must be NULL; rx_folded must be given.  Every chain computes exactly what dccn_eq_train_step would
 * compute for it alone: same kernels, same blocks, same summation orders -- bitwise equal parameters, Adam slots and
 * metrics (tests/test_gpu_chain_groups.py).  n_chains == 1 is dccn_eq_train_step.
 * dccn_eq_group_supported: 1 exactly for the shapes whose grouped step is accepted under the current knobs, given 16-byte aligned
 * buffers: the step consists of group-capable launches only (<= 96 frames: the few-row plan with the pilot bottleneck as one
 * launch per direction and the receiver folded).  Elsewhere a grouped call returns DCCN_ERR_UNSUPPORTED before anything is
 * launched. */
int dccn_chain_group_max(void);
int dccn_eq_group_supported(const dccn_eq_shape* shape);
int dccn_eq_train_step_grouped(int n_chains, const dccn_eq_shape* const* shapes, const dccn_eq_buffers* const* bufs,
                               dccn_adam_hparams hp, dccn_stream_t stream);
/* dccn_eq_receive_step for the chains of a group -- a host that serves several links, each with its own trained chain and
 * modulation, issues ONE launch sequence per round of frames: every launch of the forward carries the chain index, the decision
 * stage is launched once per distinct nbits on the chains of that modulation (its row stride ceil(D*nbits/8) and its kernels
 * depend on it).  Chain g's packed / llr / prob, out_eq, chest and snr_db are bit for bit what dccn_eq_receive_step writes for
 * chain g alone (tests/test_gpu_group_receive.py).
 * Contract as dccn_eq_train_step_grouped: the shapes agree in everything but nbits; every pointer field of bufs[g] that the
 * forward-only step uses (x, eq_params, rx_params, rx_folded, out_eq, chest, snr_db, pilot_carriers, workspace) and every
 * pointer field of outs[g] (packed, llr, prob) lies at ONE byte offset, a multiple of 256, from chain 0's; a nullable field is
 * NULL for all chains or for none; rx_folded must be given; x_prenormalised must be 0.  A violation returns
 * DCCN_ERR_INVALID_ARG, nothing launched.  Each chain's packed keeps its own row length; a caller that wants one arena layout
 * for every modulation sets packed / llr / prob aside for nbits = 4.  n_chains == 1 is dccn_eq_receive_step.
 * dccn_eq_receive_group_supported (host only, launches nothing): 1 exactly for the shapes whose grouped receive step is accepted
 * under the current knobs, given aligned buffers -- the forward of a training group without its optimizer launch (<= 96 frames,
 * single-pass normalisation, the pilot bottleneck as one launch, the receiver folded).  Elsewhere the grouped call returns
 * DCCN_ERR_UNSUPPORTED before anything is launched.  Grouped evaluation is not offered. */
int dccn_eq_receive_group_supported(const dccn_eq_shape* shape);
int dccn_eq_receive_step_grouped(int n_chains, const dccn_eq_shape* const* shapes, const dccn_eq_buffers* const* bufs,
                                 const dccn_receive_out* const* outs, dccn_stream_t stream);
/* the fused generator launch (dccn_gen_static_frames) / the launch that materialises x (dccn_gen_static_apply) for every chain of
 * a group: per-chain seed, offset and nbits, same layout contract on the descriptors' pointers (x_out / noise_power included) */
int dccn_gen_static_frames_grouped(int n_chains, const dccn_gen_static* const* g, dccn_stream_t stream);
int dccn_gen_static_apply_grouped(int n_chains, const dccn_gen_static* const* g, float* const* x_out, float* const* noise_power,
                                  dccn_stream_t stream);
/* dccn_eq_monitor_accumulate for every chain of a group (arguments as that function's, one struct per chain) */
typedef struct dccn_eq_monitor {
    const float* chest; const float* chan;
    int chan_per_symbol, B, S, K;
    const dccn_metrics* metrics;
    const float* tx_power; const float* noise_power;
    float* acc5; float* rms_out;
    void* workspace; size_t workspace_bytes;
} dccn_eq_monitor;
int dccn_eq_monitor_accumulate_grouped(int n_chains, const dccn_eq_monitor* const* m, dccn_stream_t stream);

/* mode bit0: train.  The handle is a dccn_rx_graph: launch / destroy it with dccn_rx_graph_launch /
 * dccn_rx_graph_destroy. */
int dccn_eq_graph_create(const dccn_eq_shape* shape, const dccn_eq_buffers* buf, int mode, dccn_adam_hparams hp,
                         dccn_stream_t stream, dccn_rx_graph** out);

/* ==== device-side input generator ================================================
 * What the reference computes per batch on the host with NumPy, written straight into device buffers.
 * Random streams: Philox4x32-10, counter = (index lo, index hi, stream, offset), key = seed; a batch is
 * a pure function of (seed, offset).  Streams: 0 label bits, 1 channel taps, 2 noise. */

/* test hook: out[4*i..4*i+3] = Philox words of counter (i, stream, offset) */
int dccn_philox_fill(uint32_t* out, long long n, unsigned stream, unsigned offset, unsigned long long seed,
                     dccn_stream_t stream_handle);

/* dev/py/util.py:25-29 bit_source + dev/py/ofdm.py:328-380 ofdm_tx_frame_np.
 * bits_in [frames,D,nbits] nullable (null: draw the labels and store them to bits_out, nullable otherwise);
 * cell_map int32[S*K]: >= 0 data-cell index, -1 pilot, -2 empty; const_tab [2^nbits,2] (MSB-first index);
 * idft [2K, 2(K+CP)]: real form of ifft + cyclic prefix; grid_ws [frames,S,K,2] scratch;
 * tx [frames,S,K+CP,2] time-domain frames. */
int dccn_ofdm_tx_frames(const int32_t* bits_in, int32_t* bits_out, const int32_t* cell_map, const float* const_tab,
                        float pilot_re, float pilot_im, const float* idft, float* grid_ws, float* tx, int frames,
                        int S, int K, int CP, int D, int nbits, unsigned long long seed, unsigned offset,
                        dccn_stream_t stream);

/* dev/py/radio.py:352-372 (static Rayleigh taps, 'same' FIR over the frame) + :513-526 AWGN_channel_np.
 * tx [frames,T,2]; taps_in [frames,n_taps,2] standard normals, nullable (null: draw); coeff [n_taps];
 * alpha [n_taps,L] (L <= 64, n_taps <= 16); identity != 0: pass-through channel (AWGN only);
 * snr_db [frames]; noise_in [frames,T,2] standard normals, nullable (null: draw);
 * out [frames,T,2] = y/sqrt(mean|y|^2) + noise; H [frames,nfft,2] nullable = fft(impulse response, nfft);
 * noise_power device float[1] nullable. */
size_t dccn_channel_awgn_workspace_size(int frames, int T, int L);
int dccn_channel_awgn(const float* tx, const float* taps_in, const float* coeff, const float* alpha, int n_taps,
                      int L, int identity, const float* snr_db, const float* noise_in, float* out, float* H, int nfft,
                      float* noise_power, int frames, int T, unsigned long long seed, unsigned offset,
                      void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* dev/py/radio.py:376-407 mobile (Doppler) variant: per OFDM symbol the taps follow Jakes' sum of 48
 * sinusoids (maximum Doppler Fd [Hz], symbol period t_sym = n_sc / Fs [s]) and each symbol is filtered with its own
 * impulse response over [n_taps samples of history | the symbol].  theta_in [frames,2,48,n_taps] uniform phases,
 * nullable (null: draw, stream 3).  H [frames,S,nfft,2] nullable.  Other arguments as dccn_channel_awgn; T = S*n_sc. */
size_t dccn_channel_doppler_awgn_workspace_size(int frames, int T, int L, int S);
int dccn_channel_doppler_awgn(const float* tx, const float* theta_in, const float* coeff, const float* alpha,
                              int n_taps, int L, float Fd, float t_sym, int S, int n_sc, const float* snr_db,
                              const float* noise_in, float* out, float* H, int nfft, float* noise_power, int frames,
                              unsigned long long seed, unsigned offset, void* workspace, size_t workspace_bytes,
                              dccn_stream_t stream);

/* Frame-interleaved channels (dev/py/radio.py:438-470 'mixRayleigh' / 'mixAll'): every frame belongs to one group =
 * (profile, static | Doppler); a group lists its frame indices.  taps_in [frames,16,2] / theta_in [frames,2,48,16]
 * (padded to 16 taps; the Philox tap index also uses stride 16 here), H [frames,S,nfft,2] (static frames repeat
 * their response per symbol, as the reference does).  Fd > 0 selects the Doppler model for the group. */
typedef struct dccn_channel_group {
    const int* frames;      /* device int32[n_frames] */
    int n_frames;
    const float* coeff;     /* device [n_taps] */
    const float* alpha;     /* device [n_taps, L] */
    int n_taps, L;
    int identity;           /* pass-through slot ('mixAll' frame % 5 == 0) */
    float Fd;               /* maximum Doppler [Hz]; 0 = static taps */
} dccn_channel_group;
size_t dccn_channel_groups_awgn_workspace_size(int frames, int T, int S);
int dccn_channel_groups_awgn(const float* tx, const dccn_channel_group* groups /* host array */, int n_groups,
                             const float* taps_in, const float* theta_in, float t_sym, int S, int n_sc,
                             const float* snr_db, const float* noise_in, float* out, float* H, int nfft,
                             float* noise_power, int frames, unsigned long long seed, unsigned offset,
                             void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* ==== per-frame timing alignment from the cyclic prefix =========================
 * The receive path (dccn_rx_receive_step, dccn_eq_receive_step) takes frames that sit on the FFT window; this stage puts
 * them there.  A frame is T = S*(K+CP) complex samples y[n], taken as CIRCULAR (indices mod T, as a torch.roll of the frame
 * treats it).  With N = K+CP:
 *     p[n] = y[n] * conj(y[n+K])                 e[n] = (|y[n]|^2 + |y[n+K]|^2) / 2
 *     Gamma(t) = sum_{s<S} sum_{n<CP} p[s*N + t + n]          Phi(t) likewise over e
 *     Lambda(t) = |Gamma(t)| - Phi(t)            (<= 0: the rho = 1 form of the ML cyclic-prefix estimator)
 *     offset = the smallest t in [-W, W] with the largest Lambda(t)            aligned[n] = y[(n + offset) mod T]
 * x [frames,S,K+CP,2]; offset int32[frames]; metric [frames, 2W+1] nullable = Lambda(-W .. W);
 * x_out nullable (offsets only), [frames,S,out_kin,2]: out_kin == K+CP the aligned frame, out_kin == K its samples behind each
 * symbol's prefix (x_out[f,s,0:K] = aligned_f[s, CP:CP+K], the input of a receiver built with cp = False).
 * One launch, no workspace, no atomics; every sum runs in a fixed order, so two runs give the same bits.  x is read once and
 * x_out written once.
 * dccn_frame_sync_supported (host only): 1 exactly where dccn_frame_sync accepts the shape: S >= 1, 1 <= W <= CP,
 * 2W + CP <= 64 (one lane per lag), T even (16-byte frame rows), four frames and their lag sums within 64 KB of LDS.
 * Refused with DCCN_ERR_INVALID_ARG before anything is launched: an unsupported shape; frames <= 0; x or offset NULL; x, x_out
 * or metric off a 16-byte boundary; out_kin neither K+CP nor K (nor K with S*K odd: those rows are no multiple of 16 bytes);
 * x_out overlapping x. */
int dccn_frame_sync_supported(int S, int K, int CP, int W);
int dccn_frame_sync(const float* x, int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                    float* metric, dccn_stream_t stream);
/* The same launch with the carrier-frequency offset (CFO) estimated from the angle the timing metric throws away, and taken out
 * of the frame on its way to x_out.  A frame y[n] = s[n] exp(+2 pi i eps n / K) has p[n] = |s[n]|^2 exp(-2 pi i eps) on its
 * prefix, so (van de Beek's ML estimate of the fractional offset)
 *     cfo = -atan2(Im Gamma(offset), Re Gamma(offset)) / (2 pi)       [subcarrier spacings; 0 where Gamma = 0]
 *     out[n] = y[(n + offset) mod T] * exp(-2 pi i cfo n / K)         n = 0 .. T-1, the position in the ALIGNED frame
 * offset and metric are dccn_frame_sync's, bit for bit; cfo float32[frames]; x_out as above (out_kin == K stores the same
 * out[n], only the K samples behind each symbol's prefix).  Unambiguous for |eps| < 1/2.  The frame is taken as circular: the
 * |offset| samples that wrap carry a phase step of 2 pi eps T / K against their neighbours.  A frame of NaN / Inf samples does
 * not fault: its offset stays inside [-W, W] and its cfo is whatever atan2f returns.  One launch, no workspace, no atomics, the
 * sums and the phase in a fixed order (two runs give the same bits).
 * Refused with DCCN_ERR_INVALID_ARG before anything is launched wherever dccn_frame_sync refuses, and for cfo NULL; inside a
 * chain group DCCN_ERR_UNSUPPORTED (the launch carries no chain table; several links per launch: dccn_frame_sync_grouped below). */
int dccn_frame_sync_cfo(const float* x, int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                        float* cfo, float* metric, dccn_stream_t stream);
/* The same estimator on frames that still sit inside ONE CONTIGUOUS CAPTURE cap [n_samples, 2] (what a front end hands over):
 * frame f nominally starts at sample b_f = first + f*stride, nothing is circular, and the samples the alignment brings in are the
 * frame's neighbours in the air.  With c = the capture indexed linearly, T = S*N:
 *     p[n] = c[n] * conj(c[n+K])                 e[n] = (|c[n]|^2 + |c[n+K]|^2) / 2
 *     Gamma_f(t) = sum_{s<S} sum_{n<CP} p[b_f + s*N + t + n]        Phi_f likewise        Lambda = |Gamma| - Phi
 *     offset[f] = the smallest t in [-W, W] with the largest Lambda_f(t)
 *     cfo[f] = -atan2(Im Gamma_f(offset), Re Gamma_f(offset)) / (2 pi)                    (only when cfo != NULL)
 *     out[f][n] = c[b_f + offset[f] + n] * exp(-2 pi i cfo[f] n / K),  n = 0 .. T-1       (no factor when cfo == NULL: the capture's
 *                                                                                          own bits)
 * Frame f touches exactly the samples [b_f - W, b_f + T + W); nothing outside [0, n_samples) is read.  b_f - W may be odd (any
 * first >= W, any stride >= T): a window that starts on an odd sample is read with 16-byte loads of the even-aligned pairs inside
 * it and one 8-byte load at each end.  x_out, out_kin, offset, metric as dccn_frame_sync.  On a capture whose frames sit in slots
 * [last W samples | frame | first W samples] (stride T + 2W, first W) the results are dccn_frame_sync's / dccn_frame_sync_cfo's bit
 * for bit: the sums and their order are the same code.  One launch, no workspace, no atomics; two runs give the same bits.
 * dccn_capture_sync_supported (host only): dccn_frame_sync_supported and four windows of T + 2W + 2 samples and their lag sums
 * within 64 KB of LDS.
 * Refused with DCCN_ERR_INVALID_ARG before anything is launched: an unsupported shape; frames <= 0; cap or offset NULL; cap, x_out
 * or metric off a 16-byte boundary; out_kin neither K+CP nor K (nor K with S*K odd); stride < T; first < W;
 * first + (frames-1)*stride + T + W > n_samples; x_out overlapping cap.  Inside a chain group DCCN_ERR_UNSUPPORTED. */
int dccn_capture_sync_supported(int S, int K, int CP, int W);
int dccn_capture_sync(const float* cap, long long n_samples, long long first, long long stride, int frames, int S, int K, int CP,
                      int W, int out_kin, float* x_out, int32_t* offset, float* cfo /* nullable */, float* metric /* nullable */,
                      dccn_stream_t stream);
/* dccn_capture_sync with `first` read from DEVICE memory (first_dev, int64[1]: what dccn_capture_acquire left there), so that
 * acquisition, cut and receive run as one launch sequence without a host round trip.  The kernel clamps the value it reads into
 * [lo, lo + T - 1]; everything else -- the sums, their order, the stores -- is dccn_capture_sync's own code (the kernel is a
 * second instantiation of the same body, dccn_capture_sync's instantiation is untouched): with first_dev holding `first` the
 * two calls write the same bits.
 * Refused with DCCN_ERR_INVALID_ARG before anything is launched wherever dccn_capture_sync refuses first = lo + T - 1, and for
 * first_dev NULL or off an 8-byte boundary, lo < W, lo + T - 1 + (frames-1)*stride + T + W > n_samples: every window lies inside
 * the capture for EVERY value the kernel can clamp to, so a wrong first_dev cannot read outside it.  Inside a chain group
 * DCCN_ERR_UNSUPPORTED. */
int dccn_capture_sync_at(const float* cap, long long n_samples, const long long* first_dev, long long lo, long long stride,
                         int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset,
                         float* cfo /* nullable */, float* metric /* nullable */, dccn_stream_t stream);

/* ==== coarse acquisition inside a contiguous capture ============================
 * dccn_capture_sync needs `first` to within W samples.  This stage finds it: the sample in [lo, lo + T) at which a frame starts,
 * from J >= 1 frames that follow back to back (stride T).  c = the capture indexed linearly, N = K+CP, T = S*N, p and e as above.
 * Stage A, symbol timing and carrier offset over a whole symbol period (the estimator above with J*S symbols, every lag of a period):
 *     P[m] = sum_{u<J*S} p[lo + m + u*N]   (u ascending)        E[m] likewise over e                m in [0, N+CP-1)
 *     Gamma(r) = sum_{n<CP} P[r + n]       (n ascending)        Phi(r) likewise over E              Lambda(r) = |Gamma(r)| - Phi(r)
 *     r^ = the smallest r in [0, N) with the largest Lambda(r)          eps^ = -atan2(Im Gamma(r^), Re Gamma(r^)) / (2 pi)
 * Stage B, the frame phase from the pilot symbols.  pilot_sc int32[n_pilot] (device): the frame's pilot cells as flat
 * symbol*K + carrier indices, sorted (the carrier is the DFT bin, the generator's numbering); the pilot symbols are the symbols
 * that hold at least two pilot cells, k_0 < k_1 < ... the pilot carriers of pilot symbol s.  For q in [0, S):
 *     Y_{j,q,s}[k] = sum_{n<K} c[lo + r^ + (q+s)*N + j*T + CP + n] * exp(-2 pi i (k + eps^) n / K)                   (n ascending)
 *     D_j(q) = sum_{pilot symbols s, ascending} | sum_{i ascending} Y_{j,q,s}[k_i] * conj(Y_{j,q,s}[k_{i+1}]) |
 *     D(q) = sum_{j<J, ascending} D_j(q)        q^ = the smallest q with the largest D(q)        first = lo + r^ + q^*N  in [lo, lo+T)
 * (equal pilot values on adjacent pilot carriers multiply coherently; the product is invariant to a residual timing offset
 * and to the symbol's common phase).  The twiddle phase is taken in turns, ((k n mod K) + eps^ n) / K with k n mod K an exact
 * integer.  Frames are assumed back to back at stride T during acquisition.  J = 1 with BPSK data can tie exactly (a data symbol
 * whose adjacent cells happen to agree); a batch's worth of frames (J = 16) is the intended setting.
 * first_out int64[1], cfo_out float32[1] (eps^, subcarrier spacings), sym_metric [N] nullable = Lambda(0 .. N-1), phase_metric
 * [S] nullable = D(0 .. S-1): all device memory, written on the stream; nothing is read back.  Three launches (P, E per lag;
 * Lambda, r^, eps^ and D_j(q), one block per (q, j); D, q^ and first), no host synchronisation, no atomics, every sum in the
 * order stated: two runs give the same bits.  Every read lies in [lo, lo + (J+1)*T).  pilot_sc entries outside [0, S*K) are
 * ignored; whatever the array holds, nothing outside the capture is read.
 * dccn_capture_acquire_supported (host only): 1 <= S <= 64, K >= 2, 1 <= CP <= K, K+CP <= 1024 (a block's LDS holds P, E of
 * N+CP-1 lags and one symbol), 2 <= n_pilot <= 256 (one thread per pilot carrier of a symbol), 1 <= J <= 256.
 * dccn_capture_acquire_workspace_size: bytes of device workspace (P, E, D_j(q), r^), 0 for an unsupported shape.
 * Refused with DCCN_ERR_INVALID_ARG before anything is launched: an unsupported shape; cap, pilot_sc, first_out, cfo_out or
 * workspace NULL; cap or workspace off a 16-byte boundary, first_out off an 8-byte one, pilot_sc, cfo_out, sym_metric or
 * phase_metric off a 4-byte one; lo < 0; lo + (J+2)*T > n_samples (conservative: it covers every read of both stages).  A
 * workspace smaller than the size query's answer: DCCN_ERR_WORKSPACE.  Inside a chain group DCCN_ERR_UNSUPPORTED (several links
 * per launch: the grouped entries below, which take their own link table). */
int dccn_capture_acquire_supported(int S, int K, int CP, int n_pilot, int J);
size_t dccn_capture_acquire_workspace_size(int S, int K, int CP, int n_pilot, int J);
int dccn_capture_acquire(const float* cap, long long n_samples, long long lo, int J, int S, int K, int CP, const int* pilot_sc,
                         int n_pilot, long long* first_out, float* cfo_out, float* sym_metric /* nullable */,
                         float* phase_metric /* nullable */, void* workspace, size_t workspace_bytes, dccn_stream_t stream);

/* ==== the receive front end for several links: alignment, capture cut and acquisition as shared launches ====
 * dccn_eq_receive_step_grouped carries up to dccn_chain_group_max() links through one launch sequence; these entries do the same
 * for what runs in front of it.  Each runs the solo entry's kernel body for n_links links in ONE launch (acquisition: its three
 * launches), the link index on a grid dimension and a link's blocks laid out as the solo launch lays them out: link i's outputs
 * are bit for bit what the solo entry writes for link i's arguments, and n_links == 1 writes what the solo entry writes.
 * A capture comes from a front end and does not live in a chain's arena, so the links travel as a table of per-link descriptors
 * (a HOST array of n_links entries, copied by value into the kernel arguments), not as arena offsets.
 *   common to the call: frames, S, K, CP, W, out_kin (J, n_pilot for acquisition);
 *   per link: every pointer, the capture's length, first or first_dev + lo, stride, pilot_sc, the workspace.
 * dccn_frame_sync_grouped:      link i as dccn_frame_sync(x, ..., x_out, offset, metric), or dccn_frame_sync_cfo where cfo is given.
 * dccn_capture_sync_grouped:    link i as dccn_capture_sync(cap, n_samples, first, stride, ...) where first_dev == NULL, as
 *                               dccn_capture_sync_at(cap, n_samples, first_dev, lo, stride, ...) otherwise (first_dev is read, never
 *                               written; the value is clamped into [lo, lo + T - 1]).  Known and acquired starts mix in one call.
 * dccn_capture_acquire_grouped: link i as dccn_capture_acquire(cap, n_samples, lo, J, ..., pilot_sc, ..., workspace, workspace_bytes).
 * Two links may read the same capture (or frames, or pilot_sc).  x_out, cfo and metric (sym_metric and phase_metric) are each NULL
 * for every link or for none; with cfo given the CFO instantiation runs.
 * Plan first, then issue: every link is checked by the solo entry's own rules, and the call adds: n_links outside
 * 1 .. dccn_chain_group_max(); links NULL; an output given for some links only; any output range of one link (x_out, offset,
 * cfo, metric; first_out, cfo_out, sym_metric, phase_metric, workspace) overlapping an output range or an input (x, cap,
 * first_dev, pilot_sc) of ANOTHER link -- all DCCN_ERR_INVALID_ARG; a short acquisition workspace on any link DCCN_ERR_WORKSPACE.
 * A refused call launches nothing and writes nothing for any link.  Inside a chain group DCCN_ERR_UNSUPPORTED, as the solo
 * entries: the link table is the call's own, not the group's chain table.  No atomics, no workspace beyond each link's own, every
 * sum in the solo entry's order: two runs give the same bits. */
typedef struct dccn_frame_link {
    const float* x;            /* [frames,S,K+CP,2] */
    float* x_out;              /* nullable (for all links or none) */
    int32_t* offset;           /* [frames] */
    float* cfo;                /* nullable (all or none): [frames] */
    float* metric;             /* nullable (all or none): [frames, 2W+1] */
} dccn_frame_link;
typedef struct dccn_capture_link {
    const float* cap;          /* [n_samples,2] */
    long long n_samples;
    long long first;           /* used when first_dev == NULL */
    const long long* first_dev;/* nullable: device int64[1], clamped into [lo, lo + T - 1] */
    long long lo;              /* read with first_dev only */
    long long stride;
    float* x_out;              /* nullable (all or none) */
    int32_t* offset;           /* [frames] */
    float* cfo;                /* nullable (all or none) */
    float* metric;             /* nullable (all or none) */
} dccn_capture_link;
typedef struct dccn_acquire_link {
    const float* cap;          /* [n_samples,2] */
    long long n_samples;
    long long lo;
    const int* pilot_sc;       /* [n_pilot] */
    long long* first_out;      /* [1] */
    float* cfo_out;            /* [1] */
    float* sym_metric;         /* nullable (all or none): [K+CP] */
    float* phase_metric;       /* nullable (all or none): [S] */
    void* workspace;           /* dccn_capture_acquire_workspace_size bytes, the link's own */
    size_t workspace_bytes;
} dccn_acquire_link;
int dccn_frame_sync_grouped(int n_links, const dccn_frame_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                            dccn_stream_t stream);
int dccn_capture_sync_grouped(int n_links, const dccn_capture_link* links, int frames, int S, int K, int CP, int W, int out_kin,
                              dccn_stream_t stream);
int dccn_capture_acquire_grouped(int n_links, const dccn_acquire_link* links, int J, int S, int K, int CP, int n_pilot,
                                 dccn_stream_t stream);

/* ==== one carrier offset per capture, pooled over its frames ====================
 * dccn_capture_sync estimates the carrier-frequency offset once per frame, from that frame's own S*CP prefix products.  A capture
 * comes from one front end with one oscillator, so its frames share one offset.  With b_f, offset[f] (theta_f below), Gamma_f,
 * Lambda_f and metric dccn_capture_sync's, bit for bit:
 *     Gamma = sum_{f < frames} Gamma_f(theta_f)                          (the plain sum: |Gamma_f| weights a frame by its prefix
 *                                                                         energy, the ML combination for a common offset)
 *     cfo   = 0 - atan2(Im Gamma, Re Gamma) / (2 pi)                     (ONE value per call, cfo_out float32[1]; +0 where Gamma = 0)
 *     out[f][n] = c[b_f + theta_f + n] * exp(-2 pi i cfo n / K),  n = 0 .. T-1     (the phase counted inside the frame, as above)
 * Timing stays per frame.  ORDER OF THE SUM (real and imaginary parts separately, fp32): 64 partial sums, partial l adding
 * Gamma_l, Gamma_{l+64}, Gamma_{l+128}, ... in ascending order onto +0; then a butterfly over the partials, d = 1, 2, 4, 8, 16,
 * 32: partial l becomes partial l + partial (l xor d), every l at once; partial 0 is Gamma.  A Gamma_f passes through at most
 * ceil(frames/64) - 1 + 6 rounded additions.  The order depends on `frames` alone, not on a grid, the link count or the entry.
 * Three launches on the stream (the estimate, storing theta_f and Gamma_f; the sum, one wave per link; the cut, which reads
 * offset[f] and cfo back from device memory, clamps the offset into [-W, W] before it indexes and so touches nothing outside
 * [b_f - W, b_f + T + W)).  No block waits for another, no atomics, no host round trip; two runs give the same bits.  With
 * frames == 1, cfo_out[0] and x_out are dccn_capture_sync's (cfo given) bit for bit.
 * workspace: caller-owned device memory, 16-byte aligned, dccn_capture_sync_pooled_workspace_size(frames) bytes (Gamma_f as
 * float2 [frames]; 0 for frames <= 0); it holds nothing between calls.
 * dccn_capture_sync_pooled: first_dev == NULL follows dccn_capture_sync's rules for `first` (lo is ignored); otherwise
 * dccn_capture_sync_at's for first_dev and lo (`first` is ignored).  x_out and cfo_out are required.  Accepted exactly where
 * dccn_capture_sync_supported says so.  Refused with DCCN_ERR_INVALID_ARG before anything is launched wherever that entry refuses,
 * and for x_out, cfo_out or workspace NULL, cfo_out off a 4-byte boundary, workspace off a 16-byte one; a workspace smaller than
 * the size query's answer: DCCN_ERR_WORKSPACE.  Inside a chain group DCCN_ERR_UNSUPPORTED.
 * dccn_capture_sync_pooled_grouped: the same three launches for n_links links (the link index on a grid dimension), each with its
 * own workspace; link i's outputs are bit for bit the solo call's, n_links == 1 is the solo call.  The rules of the grouped entries
 * above apply: metric for every link or for none; no output range of one link (x_out, offset, cfo, metric, workspace) may overlap
 * an output or an input (cap, first_dev) of another; a refused call launches nothing and writes nothing for any link. */
typedef struct dccn_pooled_link {
    const float* cap;          /* [n_samples,2] */
    long long n_samples;
    long long first;           /* used when first_dev == NULL */
    const long long* first_dev;/* nullable: device int64[1], clamped into [lo, lo + T - 1] */
    long long lo;              /* read with first_dev only */
    long long stride;
    float* x_out;              /* [frames,S,out_kin,2] */
    int32_t* offset;           /* [frames] */
    float* cfo;                /* [1]: the capture's estimate */
    float* metric;             /* nullable (all or none) */
    void* workspace;           /* dccn_capture_sync_pooled_workspace_size bytes, the link's own */
    size_t workspace_bytes;
} dccn_pooled_link;
size_t dccn_capture_sync_pooled_workspace_size(int frames);
int dccn_capture_sync_pooled(const float* cap, long long n_samples, long long first, const long long* first_dev /* nullable */,
                             long long lo, long long stride, int frames, int S, int K, int CP, int W, int out_kin, float* x_out,
                             int32_t* offset, float* cfo_out, float* metric /* nullable */, void* workspace,
                             size_t workspace_bytes, dccn_stream_t stream);
int dccn_capture_sync_pooled_grouped(int n_links, const dccn_pooled_link* links, int frames, int S, int K, int CP, int W,
                                     int out_kin, dccn_stream_t stream);

/* ==== carrier offsets beyond half a subcarrier spacing ==========================
 * The prefix correlation gives the offset modulo one subcarrier spacing.  An offset eps = m + f (m whole, |f| < 1/2) moves the
 * pilots from the bins k_i to k_i + m; they are boosted, their comb is broken by the DC gap and guard carriers surround the
 * band, so stage B's metric evaluated at shifted bins has one clear maximum over (symbol position q, integer shift m).
 * dccn_capture_acquire_wide: stage A as dccn_capture_acquire (r^, and eps^ = the fraction).  Stage B over both:
 *     Y_{j,q,s}[k] as above (twiddle turns ((k n mod K) + eps^ n) / K, n ascending)
 *     D_j(q,m) = sum_{pilot symbols s, ascending} | sum_{i ascending} Y_{j,q,s}[(k_i+m) mod K] * conj(Y_{j,q,s}[(k_{i+1}+m) mod K]) |
 *     D(q,m) = sum_{j<J, ascending} D_j(q,m)      m in [-M, M]
 *     (q^, m^) = the first maximum of D in row-major order of [S, 2M+1]
 *     first = lo + r^ + q^*N        cfo_out = eps^ (the fraction)        cfo_int_out = m^ (int32[1])
 * The total offset is m^ + eps^.  phase_metric (nullable) is [S, 2M+1].  M is the search span in subcarrier spacings,
 * 0 <= M <= K/2 - 1 (the 2M+1 shifts of a carrier are distinct bins); no tighter cap: the block's LDS (the narrow block's plus
 * Y of all K bins, K marks and 2M+1 sums) stays under 64 KB for every shape dccn_capture_acquire accepts.  The shift is
 * circular in K: the model is a pure rotation, and on the reference grid (K = 64, 14 guard carriers around the band) M <= 7 keeps the
 * occupied carriers inside [0, K); beyond that the search wraps, which a real channel filter does not.
 * At M == 0, first_out, cfo_out, sym_metric and phase_metric are dccn_capture_acquire's, bit for bit; at any M, sym_metric and
 * cfo_out are, and so is column m = 0 of phase_metric (the same sums in the same order).
 * Three launches: dccn_capture_acquire's first as it is; Lambda, r^, eps^ and D_j(q,m), one block per (q, j) -- per pilot symbol
 * every bin some (pilot, m) pair reads is computed once, one thread per bin, then one thread per m forms the modulus; D, (q^, m^),
 * first and m^, one block.  No atomics, no host round trip, the sums in the order stated: two runs give the same bits.  The
 * samples read are dccn_capture_acquire's; pilot_sc is untrusted as there, every bin taken mod K.
 * dccn_capture_acquire_wide_workspace_size: the narrow layout with D_j(q,m) [S, 2M+1, J]; 0 for an unsupported shape.
 * Refused before anything is launched: wherever dccn_capture_acquire refuses; M < 0 or M > K/2 - 1; cfo_int_out NULL or off a
 * 4-byte boundary -- DCCN_ERR_INVALID_ARG; a short workspace DCCN_ERR_WORKSPACE; inside a chain group DCCN_ERR_UNSUPPORTED. */
int dccn_capture_acquire_wide_supported(int S, int K, int CP, int n_pilot, int J, int M);
size_t dccn_capture_acquire_wide_workspace_size(int S, int K, int CP, int n_pilot, int J, int M);
int dccn_capture_acquire_wide(const float* cap, long long n_samples, long long lo, int J, int S, int K, int CP, const int* pilot_sc,
                              int n_pilot, int M, long long* first_out, float* cfo_out, int32_t* cfo_int_out,
                              float* sym_metric /* nullable */, float* phase_metric /* nullable */, void* workspace,
                              size_t workspace_bytes, dccn_stream_t stream);
/* The cut with the whole offset taken out.  cfo_int_dev int32[1] and cfo_frac_dev float32[1] are device memory, what
 * dccn_capture_acquire_wide left in cfo_int_out and cfo_out.  The fraction the prefix gives (eps_f per frame; the pooled eps for
 * the pooled entry) is unwrapped against them:
 *     ref = (float)m^ + eps^_acq        I = rint(ref - eps_f), kept inside [-K/2, K/2] (0 where the difference is NaN)
 *     cfo[f] = (float)I + eps_f
 *     out[f][n] = c[b_f + offset[f] + n] * exp(-2 pi i ((I n mod K) + eps_f n) / K)
 * The whole turns of I n / K drop out exactly ((I n mod K) is an integer), so the phase carries the roundings of the narrow
 * derotation however large I is; cfo * n is never formed with the total.  A frame whose own fraction lands on the other side
 * of +-1/2 from acquisition's still gets the right total (2.49 read as -0.49 gives I = 3).  A wild device value costs a wrong
 * derotation, nothing else.
 * dccn_capture_sync_wide: dccn_capture_sync_at with cfo given, plus the two inputs; offset and metric are that call's bits, and
 * with m^ = 0, eps^_acq = 0 so are cfo and x_out.  One launch.  Refused wherever dccn_capture_sync_at refuses, and for cfo,
 * cfo_int_dev or cfo_frac_dev NULL or the latter two off a 4-byte boundary.
 * dccn_capture_sync_pooled_wide: dccn_capture_sync_pooled plus the two inputs; first / first_dev / lo as there.  Its estimate and
 * sum launches as they are (the capture's fraction goes to a workspace slot), then a cut that unwraps it; cfo_out[0] is the
 * total.  With m^ = 0, eps^_acq = 0 every output is dccn_capture_sync_pooled's, bit for bit.  workspace:
 * dccn_capture_sync_pooled_wide_workspace_size(frames) bytes (16 more than the pooled call's).  Refused wherever
 * dccn_capture_sync_pooled refuses, and for the two inputs as above; a short workspace DCCN_ERR_WORKSPACE.
 * Both: a refused call launches nothing; inside a chain group DCCN_ERR_UNSUPPORTED; two runs give the same bits. */
int dccn_capture_sync_wide(const float* cap, long long n_samples, const long long* first_dev, long long lo, long long stride,
                           int frames, int S, int K, int CP, int W, int out_kin, float* x_out, int32_t* offset, float* cfo,
                           float* metric /* nullable */, const int32_t* cfo_int_dev, const float* cfo_frac_dev,
                           dccn_stream_t stream);
size_t dccn_capture_sync_pooled_wide_workspace_size(int frames);
int dccn_capture_sync_pooled_wide(const float* cap, long long n_samples, long long first, const long long* first_dev /* nullable */,
                                  long long lo, long long stride, int frames, int S, int K, int CP, int W, int out_kin,
                                  float* x_out, int32_t* offset, float* cfo_out, float* metric /* nullable */,
                                  const int32_t* cfo_int_dev, const float* cfo_frac_dev, void* workspace, size_t workspace_bytes,
                                  dccn_stream_t stream);

/* ==== 16-bit integer I/Q captures, converted inside the launches =================
 * A front end (an ADC, an SDR driver) delivers interleaved 16-bit integer I/Q ("sc16"), not float32.  These entries take the
 * capture as it arrives: cap int16 [n_samples, 2], contiguous, (I, Q) interleaved, native byte order, the base on a 16-byte boundary.
 * The value of sample n is
 *     ( (float)I[n] * scale, (float)Q[n] * scale )
 * -- the int16 -> fp32 conversion is exact and each component gets ONE fp32 multiply, rounded to nearest.  scale is a finite,
 * positive host value (2^-15 maps full scale onto [-1, 1)).  The receiver and the chain normalise their input by batch moments, so
 * scale moves no decision; it sets the magnitude of the metrics and keeps the samples out of the denormals.
 * THE CONTRACT: every output of an sc16 entry equals, bit for bit, what the float32 entry writes when it is given the converted
 * capture c[n] = the value above (frames, offset, metric, per-frame and pooled cfo; first_out, cfo_out, sym_metric, phase_metric).
 * Only the loads differ: a window is read four samples per 16-byte load, its head and tail with 8- or 4-byte loads (no lane reads a
 * sample outside [b_f - W, b_f + T + W): nothing at or beyond cap + 4*n_samples bytes is touched, whatever n_samples mod 4 is),
 * and lands in LDS where the float32 loader puts it; acquisition reads one 4-byte sample per load.  Everything behind the load is
 * the float32 entry's code, the kernels are new instantiations and the float32 kernels are untouched.  No conversion launch, no
 * float copy of the capture, half the capture bytes per launch.
 * dccn_capture_sync_sc16:        first_dev == NULL: dccn_capture_sync (lo is ignored); otherwise dccn_capture_sync_at, `first`
 *                                ignored, the value read clamped into [lo, lo + T - 1].  One launch.
 * dccn_capture_sync_pooled_sc16: dccn_capture_sync_pooled (first / first_dev / lo as there); three launches, the same workspace.
 * dccn_capture_acquire_sc16:     dccn_capture_acquire; three launches, the same workspace.
 * dccn_capture_sync_supported, dccn_capture_acquire_supported, dccn_capture_acquire_workspace_size and
 * dccn_capture_sync_pooled_workspace_size answer for both formats.
 * Plan first, then launch: refused before anything is launched (nothing is written) wherever the float32 entry refuses, with the
 * capture's extent taken as 4*n_samples bytes (so an x_out that starts at cap + 4*n_samples is accepted), and for a scale that is
 * not finite or not > 0 -- DCCN_ERR_INVALID_ARG; a short workspace DCCN_ERR_WORKSPACE; inside a chain group DCCN_ERR_UNSUPPORTED.
 * float32 only: the wide entries (dccn_capture_acquire_wide, dccn_capture_sync_wide, dccn_capture_sync_pooled_wide) and every
 * grouped entry. */
int dccn_capture_sync_sc16(const int16_t* cap, long long n_samples, float scale, long long first,
                           const long long* first_dev /* nullable */, long long lo, long long stride, int frames, int S, int K, int CP,
                           int W, int out_kin, float* x_out, int32_t* offset, float* cfo /* nullable */, float* metric /* nullable */,
                           dccn_stream_t stream);
int dccn_capture_sync_pooled_sc16(const int16_t* cap, long long n_samples, float scale, long long first,
                                  const long long* first_dev /* nullable */, long long lo, long long stride, int frames, int S, int K,
                                  int CP, int W, int out_kin, float* x_out, int32_t* offset, float* cfo_out,
                                  float* metric /* nullable */, void* workspace, size_t workspace_bytes, dccn_stream_t stream);
int dccn_capture_acquire_sc16(const int16_t* cap, long long n_samples, float scale, long long lo, int J, int S, int K, int CP,
                              const int* pilot_sc, int n_pilot, long long* first_out, float* cfo_out,
                              float* sym_metric /* nullable */, float* phase_metric /* nullable */, void* workspace,
                              size_t workspace_bytes, dccn_stream_t stream);

/* ==== host utility: CRC32C (Castagnoli), the checksum of TensorFlow's tensor-bundle checkpoints =========
 * (tf.train.Saver files the reference writes at dev/py/ofdmreceiver_np.py:271).
 * Returns the CRC of (previous data ++ data) given the CRC of the previous data (0 to start).  Host code. */
uint32_t dccn_crc32c(uint32_t crc, const void* data, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* DCCN_H_ */

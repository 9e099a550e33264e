// libdccn.so -- device-side generator, classical receivers, in-graph AWGN branch (see abi_impl.h for how the library is cut into units)
#include "abi_impl.h"
#include "link_group.h"

using namespace dccn;

extern "C" {

// ---- device-side input generator ------------------------------------------------------------------
int dccn_philox_fill(uint32_t* out, long long n, unsigned stream, unsigned offset, unsigned long long seed,
                     dccn_stream_t stream_handle) {
    if (!out || n <= 0) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(philox_fill_kernel, dim3((unsigned)ceil_div_ll(n, 256)), dim3(256), 0,
                       (hipStream_t)stream_handle, out, n, stream, offset, seed);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_ofdm_tx_frames(const int32_t* bits_in, int32_t* bits_out, const int32_t* cell_map, const float* const_tab,
                        float pilot_re, float pilot_im, const float* idft, float* grid_ws, float* tx, int frames,
                        int S, int K, int CP, int D, int nbits, unsigned long long seed, unsigned offset,
                        dccn_stream_t stream) {
    if (!cell_map || !const_tab || !idft || !grid_ws || !tx || frames <= 0 || S <= 0 || K <= 0 || CP < 0 || D <= 0 ||
        nbits < 1 || nbits > 4)
        return DCCN_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const long long n_cells = (long long)frames * S * K;
    hipLaunchKernelGGL(tx_grid_kernel, dim3((unsigned)ceil_div_ll(n_cells, 256)), dim3(256), 0, s, bits_in, bits_out,
                       cell_map, (const float2*)const_tab, make_float2(pilot_re, pilot_im), (float2*)grid_ws, n_cells,
                       S * K, D, nbits, offset, seed);
    DCCN_LAUNCH_CHECK();
    return dense_fwd_impl(grid_ws, idft, nullptr, tx, frames * S, 2 * K, 2 * (K + CP), s);
}
static int chan_blocks_x(int T) { return ceil_div(T, 256); }
// persistent FIR grid: all items when they are few, else eight blocks per CU; never more than the partial slots
static int fir_blocks(int items, int cap) {
    int b = items < 8 * kCUs ? items : 8 * kCUs;
    if (b > cap) b = cap;
    return b < 1 ? 1 : b;
}
// static-channel FIR: whole frames per block (bx items each) so that a frame's taps are set up once in the launch
struct FirPlan {
    int blocks, ipb;
};
static FirPlan fir_plan(int items, int bx, int cap) {
    const int b0 = fir_blocks(items, cap);
    FirPlan p;
    p.ipb = ceil_div(ceil_div(items, b0), bx) * bx;
    p.blocks = ceil_div(items, p.ipb);
    return p;
}
// workspace of the channel stage, one layout for the three entry points (gstride = complex taps per frame: L, S * L, 64 * S)
// g: the frames' tap responses; y: FIR output, before the noise; partial: signal-power partials of the FIR blocks (kChanPartials
// slots); npartial: noise-power partials, one per AWGN block (bx per frame)
struct ChanWs { float *g, *y; double *partial, *npartial; int bx; };
static ChanWs chan_carve(Carver& c, int frames, int T, int gstride) {
    ChanWs w;
    w.bx = chan_blocks_x(T);
    w.g = c.take<float>((size_t)frames * gstride * 2);
    w.y = c.take<float>((size_t)frames * T * 2);
    w.partial = c.take<double>((size_t)kChanPartials);
    w.npartial = c.take<double>((size_t)frames * w.bx);
    c.take<float>(4);       // (four floats no launch uses: part of the size the callers allocate)
    return w;
}
// enabled (nobody wants the frequency response and the taps are drawn here): the FIR blocks draw the taps themselves
static TapGen tap_gen_of(bool enabled, const float* coeff, const float* alpha, int n_taps, int identity, int tap_stride,
                         unsigned offset, unsigned long long seed) {
    TapGen tg;
    memset(&tg, 0, sizeof(tg));
    tg.enabled = enabled ? 1 : 0;
    tg.coeff = coeff; tg.alpha = alpha; tg.n_taps = n_taps; tg.identity = identity; tg.tap_stride = tap_stride;
    tg.offset = offset; tg.seed = seed;
    return tg;
}
size_t dccn_channel_awgn_workspace_size(int frames, int T, int L) {
    if (frames <= 0 || T <= 0 || L <= 0) return 0;
    return carved_bytes([&](Carver& c) { chan_carve(c, frames, T, L); });
}
// the stage's tail: AWGN at the power the `n_partial` FIR partials sum to, then the noise power when the caller wants it
static int chan_awgn_tail(const ChanWs& w, int n_partial, const float* snr_db, const float* noise_in, float* out, float* noise_power,
                          int frames, int T, unsigned long long seed, unsigned offset, hipStream_t s) {
    const double total = (double)frames * (double)T;
    hipLaunchKernelGGL(awgn_kernel, dim3(w.bx, frames), dim3(256), 0, s, (const float2*)w.y, (const double*)w.partial, n_partial,
                       total, snr_db, noise_in, (float2*)out, noise_power ? w.npartial : nullptr, T, offset, seed);
    DCCN_LAUNCH_CHECK();
    if (noise_power) {
        hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, (const double*)w.npartial, frames * w.bx, total,
                           noise_power);
        DCCN_LAUNCH_CHECK();
    }
    return DCCN_OK;
}
int dccn_channel_awgn(const float* tx, const float* taps_in, const float* coeff, const float* alpha, int n_taps,
                      int L, int identity, const float* snr_db, const float* noise_in, float* out, float* H, int nfft,
                      float* noise_power, int frames, int T, unsigned long long seed, unsigned offset,
                      void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    if (!tx || !snr_db || !out || frames <= 0 || frames > 65535 || T <= 0 || L <= 0 || L > 64) return DCCN_ERR_INVALID_ARG;
    if (!identity && (!coeff || !alpha || n_taps <= 0 || n_taps > 16)) return DCCN_ERR_INVALID_ARG;
    if (H && nfft <= 0) return DCCN_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < dccn_channel_awgn_workspace_size(frames, T, L)) return DCCN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Carver c(workspace, workspace_bytes);
    const ChanWs w = chan_carve(c, frames, T, L);
    float *g = w.g, *y = w.y; double* partial = w.partial; const int bx = w.bx;
    const TapGen tg = tap_gen_of(H == nullptr && taps_in == nullptr, coeff, alpha, n_taps, identity, n_taps, offset, seed);
    if (!tg.enabled) {
        hipLaunchKernelGGL(channel_taps_kernel, dim3(frames), dim3(64), 0, s, taps_in, coeff, alpha, (float2*)g, (float2*)H,
                           n_taps, L, nfft, identity, offset, seed, (const int*)nullptr, n_taps, L, 1);
        DCCN_LAUNCH_CHECK();
    }
    const FirPlan fp = fir_plan(frames * bx, bx, kChanPartials);
    const int nfb = fp.blocks;
    hipLaunchKernelGGL(fir_same_kernel, dim3(nfb), dim3(256), 0, s, (const float2*)tx, (const float2*)g,
                       (float2*)y, partial, T, L, (const int*)nullptr, L, frames, 0, tg, fp.ipb);
    DCCN_LAUNCH_CHECK();
    return chan_awgn_tail(w, nfb, snr_db, noise_in, out, noise_power, frames, T, seed, offset, s);
}

// ---- fused static-channel generator (datagen.h gen_static_frames_kernel) ----------------------------------------------
static_assert(sizeof(dccn_gen_static) == 200 && sizeof(dccn_rx_buffers) == 208 && sizeof(dccn_eq_buffers) == 208 &&
              sizeof(dccn_eq_monitor) == 88, "ctypes mirrors in dl_ofdm_amd/_lib.py");
int dccn_gen_static_supported(int S, int K, int CP) {
    return gen_static_shape_ok(S, K, CP) ? 1 : 0;
}
int dccn_gen_static_partials(int frames) { return frames > 0 ? ceil_div(frames, kGenFramesPerBlock) : 0; }
int dccn_gen_static_frames(const dccn_gen_static* g, dccn_stream_t stream) { return gen_static_launch(g, (hipStream_t)stream); }
// x = y / sqrt(mean |y|^2) + noise into x_out: the whole frames, or (window) the batch of a cp=False receiver, the K samples
// behind the cyclic prefix of every symbol.  noise_power is served when the generator launch left noise partials.
static int gen_static_apply_launch(const dccn_gen_static* g, float* x_out, float* noise_power, bool window, hipStream_t s) {
    if (!gen_static_ok(g) || !x_out || !aligned16(x_out)) return DCCN_ERR_INVALID_ARG;
    const int T = g->S * (g->K + g->CP);
    long long n4;                             // float4s of x_out
    if (window) {
        // (gen_static_ok: K = 64 and CP = 16 or 4, so a symbol, its window and the window's offset are whole float4s)
        if ((2 * g->K) % 4 != 0 || (2 * g->CP) % 4 != 0) return DCCN_ERR_INVALID_ARG;
        DCCN_NO_CHAINS();                     // (that launch carries no chain table: inside a group it would serve chain 0 only)
        n4 = (long long)g->frames * g->S * (2 * g->K / 4);
    } else {
        if (((long long)g->frames * T * 2) % 4 != 0) return DCCN_ERR_INVALID_ARG;
        n4 = (long long)g->frames * T * 2 / 4;
    }
    const int np = dccn_gen_static_partials(g->frames);
    long long blocks = ceil_div_ll(n4, 256);
    if (blocks > 4 * kCUs) blocks = 4 * kCUs;
    const float4 *y = reinterpret_cast<const float4*>(g->y), *noise = reinterpret_cast<const float4*>(g->noise);
    const double total = (double)g->frames * (double)T;
    const bool want_np = noise_power && g->noise_partial;
    const double* npart = want_np ? g->noise_partial : nullptr;
    float* npow = want_np ? noise_power : nullptr;
    if (window)
        hipLaunchKernelGGL(gen_static_apply_window_kernel, dim3((unsigned)blocks), dim3(256), 0, s, y, noise, (const double*)g->power_partial,
                           np, total, reinterpret_cast<float4*>(x_out), n4, 2 * g->K / 4, 2 * (g->K + g->CP) / 4, 2 * g->CP / 4, npart,
                           np, npow);
    else
        DCCN_LAUNCH_CHAINS_Z(gen_static_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, s, y, noise, (const double*)g->power_partial,
                             np, total, reinterpret_cast<float4*>(x_out), n4, npart, np, npow);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_gen_static_apply(const dccn_gen_static* g, float* x_out, float* noise_power, dccn_stream_t stream) {
    return gen_static_apply_launch(g, x_out, noise_power, false, (hipStream_t)stream);
}
int dccn_gen_static_apply_window(const dccn_gen_static* g, float* x_out, float* noise_power, dccn_stream_t stream) {
    return gen_static_apply_launch(g, x_out, noise_power, true, (hipStream_t)stream);
}

// apply + frame alignment as one launch (datagen.h gen_apply_sync_kernel).  Everything the call decides, before its one launch:
// a refused call launches nothing.
struct GenApplySyncPlan {
    GenApplySyncArgs args;
    unsigned blocks;
    size_t lds;
};
static int gen_apply_sync_plan(const dccn_gen_static* g, int W, int out_kin, float* x_out, int32_t* offset, float* H_inout, int h_rep,
                               float* noise_power, GenApplySyncPlan* plan) {
    if (!gen_static_ok(g) || !frame_sync_shape_ok(g->S, g->K, g->CP, W)) return DCCN_ERR_INVALID_ARG;
    if (!x_out || !aligned16(x_out) || !offset) return DCCN_ERR_INVALID_ARG;
    if (out_kin != g->K + g->CP && out_kin != g->K) return DCCN_ERR_INVALID_ARG;
    if (out_kin == g->K && (g->S * g->K) % 2 != 0) return DCCN_ERR_INVALID_ARG;      // (cropped rows leave as 16-byte stores too)
    if (H_inout && ((h_rep != 1 && h_rep != g->S) || reinterpret_cast<uintptr_t>(H_inout) % 8 != 0)) return DCCN_ERR_INVALID_ARG;
    const int T = g->S * (g->K + g->CP);
    const size_t in_bytes = (size_t)g->frames * T * 8, out_bytes = (size_t)g->frames * g->S * out_kin * 8;
    if (ranges_overlap(g->y, in_bytes, x_out, out_bytes) || ranges_overlap(g->noise, in_bytes, x_out, out_bytes))
        return DCCN_ERR_INVALID_ARG;
    const int np = dccn_gen_static_partials(g->frames);
    const bool want_np = noise_power && g->noise_partial;
    GenApplySyncArgs& a = plan->args;
    a.y = reinterpret_cast<const float4*>(g->y); a.noise = reinterpret_cast<const float4*>(g->noise);
    a.ppart = g->power_partial; a.npart = np; a.total = (double)g->frames * (double)T;
    a.x_out = x_out; a.offset = offset; a.H = reinterpret_cast<float2*>(H_inout); a.h_rep = H_inout ? h_rep : 0;
    a.npart_noise = want_np ? g->noise_partial : nullptr; a.n_noise = np; a.npow_out = want_np ? noise_power : nullptr;
    a.frames = g->frames; a.S = g->S; a.K = g->K; a.CP = g->CP; a.W = W; a.crop = out_kin == g->K ? 1 : 0;
    plan->blocks = (unsigned)ceil_div(g->frames, kSyncWaves);
    plan->lds = kSyncWaves * frame_sync_lds_per_frame(T);
    return DCCN_OK;
}
int dccn_gen_static_apply_sync_supported(int S, int K, int CP, int W) {
    return (gen_static_shape_ok(S, K, CP) && frame_sync_shape_ok(S, K, CP, W)) ? 1 : 0;
}
int dccn_gen_static_apply_sync(const dccn_gen_static* g, int W, int out_kin, float* x_out, int32_t* offset, float* H_inout, int h_rep,
                               float* noise_power, dccn_stream_t stream) {
    GenApplySyncPlan plan;
    DCCN_TRY(gen_apply_sync_plan(g, W, out_kin, x_out, offset, H_inout, h_rep, noise_power, &plan));
    DCCN_NO_CHAINS();                         // (the launch carries no chain table: inside a group it would serve chain 0 only)
    DCCN_TRY(set_max_dynamic_smem((const void*)gen_apply_sync_kernel, plan.lds));
    hipLaunchKernelGGL(gen_apply_sync_kernel, dim3(plan.blocks), dim3(kSyncWaves * kSyncLanes), plan.lds, (hipStream_t)stream, plan.args);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

size_t dccn_channel_doppler_awgn_workspace_size(int frames, int T, int L, int S) {
    if (frames <= 0 || T <= 0 || L <= 0 || S <= 0) return 0;
    return dccn_channel_awgn_workspace_size(frames, T, L * S);
}
int dccn_channel_doppler_awgn(const float* tx, const float* theta_in, const float* coeff, const float* alpha,
                              int n_taps, int L, float Fd, float t_sym, int S, int n_sc, const float* snr_db,
                              const float* noise_in, float* out, float* H, int nfft, float* noise_power, int frames,
                              unsigned long long seed, unsigned offset, void* workspace, size_t workspace_bytes,
                              dccn_stream_t stream) {
    if (!tx || !coeff || !alpha || !snr_db || !out || frames <= 0 || frames > 65535 || S <= 0 || S > 16 || n_sc <= 0 ||
        L <= 0 || L > 64 || n_taps <= 0 || n_taps > 16 || (H && nfft <= 0))
        return DCCN_ERR_INVALID_ARG;
    const int T = S * n_sc;
    if (!workspace || workspace_bytes < dccn_channel_doppler_awgn_workspace_size(frames, T, L, S))
        return DCCN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Carver c(workspace, workspace_bytes);
    const ChanWs w = chan_carve(c, frames, T, S * L);
    float *g = w.g, *y = w.y; double* partial = w.partial; const int bx = w.bx;
    hipLaunchKernelGGL(doppler_taps_kernel, dim3(frames), dim3(64), 0, s, theta_in, coeff, alpha, (float2*)g, (float2*)H,
                       n_taps, L, nfft, S, Fd, t_sym, offset, seed, (const int*)nullptr, n_taps, S * L);
    DCCN_LAUNCH_CHECK();
    const int nfb = fir_blocks(frames * bx, kChanPartials);
    hipLaunchKernelGGL(fir_doppler_kernel, dim3(nfb), dim3(256), 0, s, (const float2*)tx, (const float2*)g,
                       (float2*)y, partial, T, L, n_sc, n_taps, (const int*)nullptr, S * L, frames, 0);
    DCCN_LAUNCH_CHECK();
    return chan_awgn_tail(w, nfb, snr_db, noise_in, out, noise_power, frames, T, seed, offset, s);
}

size_t dccn_channel_groups_awgn_workspace_size(int frames, int T, int S) {
    if (frames <= 0 || T <= 0 || S <= 0) return 0;
    return dccn_channel_awgn_workspace_size(frames, T, 64 * S);
}
int dccn_channel_groups_awgn(const float* tx, const dccn_channel_group* groups, int n_groups, const float* taps_in,
                             const float* theta_in, float t_sym, int S, int n_sc, const float* snr_db,
                             const float* noise_in, float* out, float* H, int nfft, float* noise_power, int frames,
                             unsigned long long seed, unsigned offset, void* workspace, size_t workspace_bytes,
                             dccn_stream_t stream) {
    if (!tx || !groups || n_groups <= 0 || !snr_db || !out || frames <= 0 || frames > 65535 || S <= 0 || S > 16 ||
        n_sc <= 0 || (H && nfft <= 0))
        return DCCN_ERR_INVALID_ARG;
    const int T = S * n_sc;
    int covered = 0;
    for (int i = 0; i < n_groups; ++i) {
        const dccn_channel_group& g = groups[i];
        if (g.n_frames < 0 || (g.n_frames > 0 && !g.frames && n_groups > 1)) return DCCN_ERR_INVALID_ARG;
        if (!g.identity && (!g.coeff || !g.alpha || g.n_taps <= 0 || g.n_taps > 16 || g.L <= 0 || g.L > 64))
            return DCCN_ERR_INVALID_ARG;
        covered += g.n_frames;
    }
    if (covered != frames) return DCCN_ERR_INVALID_ARG;        // every frame belongs to exactly one group
    if (!workspace || workspace_bytes < dccn_channel_groups_awgn_workspace_size(frames, T, S)) return DCCN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    Carver c(workspace, workspace_bytes);
    const int gstride = 64 * S;
    const ChanWs w = chan_carve(c, frames, T, gstride);
    float *g = w.g, *y = w.y; double* partial = w.partial; const int bx = w.bx;
    int live = 0;
    for (int i = 0; i < n_groups; ++i) live += groups[i].n_frames > 0 ? 1 : 0;
    const int pcap = kChanPartials / (live > 0 ? live : 1);       // partial slots per group launch
    int pbase = 0;
    for (int i = 0; i < n_groups; ++i) {
        const dccn_channel_group& q = groups[i];
        if (q.n_frames == 0) continue;
        if (q.identity || q.Fd <= 0.f) {
            const int L = q.identity ? 1 : q.L;
            const TapGen tg = tap_gen_of(H == nullptr && taps_in == nullptr, q.coeff, q.alpha, q.n_taps, q.identity, 16, offset, seed);
            if (!tg.enabled) {
                hipLaunchKernelGGL(channel_taps_kernel, dim3(q.n_frames), dim3(64), 0, s, taps_in, q.coeff, q.alpha, (float2*)g,
                                   (float2*)H, q.n_taps, L, nfft, q.identity, offset, seed, q.frames, 16, gstride, S);
                DCCN_LAUNCH_CHECK();
            }
            const FirPlan fp = fir_plan(q.n_frames * bx, bx, pcap);
            const int nfb = fp.blocks;
            hipLaunchKernelGGL(fir_same_kernel, dim3(nfb), dim3(256), 0, s, (const float2*)tx, (const float2*)g,
                               (float2*)y, partial, T, L, q.frames, gstride, q.n_frames, pbase, tg, fp.ipb);
            DCCN_LAUNCH_CHECK();
            pbase += nfb;
        } else {
            hipLaunchKernelGGL(doppler_taps_kernel, dim3(q.n_frames), dim3(64), 0, s, theta_in, q.coeff, q.alpha, (float2*)g,
                               (float2*)H, q.n_taps, q.L, nfft, S, q.Fd, t_sym, offset, seed, q.frames, 16, gstride);
            DCCN_LAUNCH_CHECK();
            const int nfb = fir_blocks(q.n_frames * bx, pcap);
            hipLaunchKernelGGL(fir_doppler_kernel, dim3(nfb), dim3(256), 0, s, (const float2*)tx,
                               (const float2*)g, (float2*)y, partial, T, q.L, n_sc, q.n_taps, q.frames, gstride, q.n_frames, pbase);
            DCCN_LAUNCH_CHECK();
            pbase += nfb;
        }
    }
    return chan_awgn_tail(w, pbase, snr_db, noise_in, out, noise_power, frames, T, seed, offset, s);
}

// ---- classical pilot-aided receivers (classical.h) -----------------------------------------------------------------
// gain: per-block sums of dccn_classical_gain (dccn_classical_estimate modes 1 / 3 read them); errors: per-block bit errors of
// dccn_classical_detect
struct ClassicalWs { double* gain; long long* errors; };
static ClassicalWs classical_carve(Carver& c) {
    double* gain = c.take<double>((size_t)kClassicalPartials * 4);
    return ClassicalWs{gain, c.take<long long>((size_t)kClassicalPartials)};
}
size_t dccn_classical_workspace_size(void) { return carved_bytes([](Carver& c) { classical_carve(c); }); }
static int classical_blocks(long long items) {
    long long b = items < 2 * kCUs ? items : 2 * kCUs;
    if (b > kClassicalPartials) b = kClassicalPartials;
    return (int)(b < 1 ? 1 : b);
}
int dccn_dense_fwd_ld(const float* x, int ldx, const float* w, const float* bias, float* y, int M, int K, int N,
                      dccn_stream_t stream) {
    if (ldx < K) return DCCN_ERR_INVALID_ARG;
    return dense_fwd_impl(x, w, bias, y, M, K, N, (hipStream_t)stream, ldx);
}
int dccn_classical_pilot_ls(const float* Y, const int* pil, float* gp, int n, int SK, int P, float pv_re, float pv_im,
                            dccn_stream_t stream) {
    if (!Y || !pil || !gp || n <= 0 || SK <= 0 || P <= 0 || (pv_re == 0.f && pv_im == 0.f)) return DCCN_ERR_INVALID_ARG;
    hipLaunchKernelGGL(classical_pilot_ls_kernel, dim3((unsigned)ceil_div_ll((long long)n * P, 256)), dim3(256), 0,
                       (hipStream_t)stream, (const float2*)Y, pil, gp, n, SK, P, make_float2(pv_re, pv_im));
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_classical_gain(const float* Y, const float* H, const float* Gls, const int* pil, int n, int SK, int P, float pv_re,
                        float pv_im, double* sums4, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    if (!Y || !Gls || !pil || n <= 0 || SK <= 0 || P <= 0) return DCCN_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < dccn_classical_workspace_size()) return DCCN_ERR_WORKSPACE;
    Carver c(workspace, workspace_bytes);
    double* partial = classical_carve(c).gain;
    const int nblk = classical_blocks(n);       // (dccn_classical_estimate modes 1 / 3 read these partials: dccn.h order contract)
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(classical_gain_kernel, dim3(nblk), dim3(256), 0, s, (const float2*)Y, (const float2*)H, Gls, pil, partial,
                       n, SK, P, make_float2(pv_re, pv_im));
    DCCN_LAUNCH_CHECK();
    if (sums4) {
        hipLaunchKernelGGL(classical_finish_kernel, dim3(1), dim3(256), 0, s, (const long long*)nullptr, 0, (const double*)partial,
                           nblk, (long long*)nullptr, sums4);
        DCCN_LAUNCH_CHECK();
    }
    return DCCN_OK;
}
int dccn_classical_estimate(const float* Gls, const float* H, float* G, int n, int S, int K, int mode, float c_var,
                            void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    if (!Gls || !G || n <= 0 || S <= 0 || S > 32 || K <= 0 || mode < CE_LS || mode > CE_FRAME_MEAN) return DCCN_ERR_INVALID_ARG;
    if ((mode == CE_LMMSE || mode == CE_PERFECT) && !H) return DCCN_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < dccn_classical_workspace_size()) return DCCN_ERR_WORKSPACE;
    Carver c(workspace, workspace_bytes);
    double* partial = classical_carve(c).gain;
    hipLaunchKernelGGL(classical_estimate_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, Gls, (const float2*)H,
                       (const double*)partial, classical_blocks(n), (float2*)G, n, S, K, mode, c_var);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}
int dccn_classical_detect(const float* Y, const float* G, const int* dat, const float* table, const int* labels,
                          const int32_t* bits, int32_t* det, long long* errors, int n, int SK, int D, int m, int nbits,
                          int g_row, int g_mod, void* workspace, size_t workspace_bytes, dccn_stream_t stream) {
    if (!Y || !G || !dat || !table || !labels || !bits || !errors || n <= 0 || SK <= 0 || D <= 0 || m <= 0 || nbits < 1 ||
        nbits > 8 || g_row <= 0)
        return DCCN_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < dccn_classical_workspace_size()) return DCCN_ERR_WORKSPACE;
    Carver c(workspace, workspace_bytes);
    long long* ep = classical_carve(c).errors;
    const int nblk = classical_blocks(ceil_div_ll((long long)n * D, 256));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(classical_detect_kernel, dim3(nblk), dim3(256), 0, s, (const float2*)Y, (const float2*)G, dat,
                       (const float2*)table, labels, bits, det, ep, n, SK, D, m, nbits, g_row, g_mod);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(classical_finish_kernel, dim3(1), dim3(256), 0, s, (const long long*)ep, nblk, (const double*)nullptr, 0,
                       errors, (double*)nullptr);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// ---- classical receive: the label-free detector of the receive path as one launch (classical_receive.h) -----------------
static_assert(sizeof(dccn_classical_receive_args) == 160, "dccn.h states the size; dl_ofdm_amd/_lib.py mirrors the layout");
int dccn_classical_receive_supported(int S, int K, int CP, int P, int D, int E, int nbits) {
    if (S < 1 || S > kClsRxRows || K < 16 || K % 16 != 0 || K > 4096 || CP < 0 || CP > 4096 || (K + CP) % 2 != 0) return 0;
    if (P < 1 || P > (1 << 16) || D < 1 || D > (1 << 24) || E < 1 || E > (1 << 24) || nbits < 1 || nbits > 4) return 0;
    return clsrx_lds_floats(S, K, P) * sizeof(float) <= kClsRxMaxLds ? 1 : 0;
}
static bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
// One link of a classical receive call, judged by the rules dccn.h states -> its entry of the launch's table and the shape.  Both
// entries judge a link here, so a link the grouped call accepts is one the solo call accepts.
static int clsrx_link_plan(const dccn_classical_link& a, int frames, int S, int K, int CP, int P, int D, int E, ClsRxLink* l,
                           ClsRxShape* sh) {
    if (!dccn_classical_receive_supported(S, K, CP, P, D, E, a.nbits)) return DCCN_ERR_INVALID_ARG;
    if (frames < 1 || frames > (1 << 24) || a.win < 0 || a.win > CP || a.m != (1 << a.nbits)) return DCCN_ERR_INVALID_ARG;
    if (a.mode != CE_LS && a.mode != CE_ALMMSE) return DCCN_ERR_INVALID_ARG;
    if (!isfinite(a.noise_var) || a.noise_var < 0.f) return DCCN_ERR_INVALID_ARG;
    const float pd = a.pv_re * a.pv_re + a.pv_im * a.pv_im;
    if (!isfinite(pd) || !(pd > 0.f)) return DCCN_ERR_INVALID_ARG;
    if (!a.dft || !a.w || !a.pil || !a.dat || !a.empty || !a.table || !a.labels || !a.x || !a.packed) return DCCN_ERR_INVALID_ARG;
    if (!aligned16(a.x) || !aligned_to(a.dft, 4) || !aligned_to(a.w, 4) || !aligned_to(a.pil, 4) || !aligned_to(a.dat, 4) ||
        !aligned_to(a.empty, 4) || !aligned_to(a.table, 8) || !aligned_to(a.labels, 4) || !aligned_to(a.llr, 4) ||
        !aligned_to(a.chest, 8) || !aligned_to(a.y_freq, 8) || !aligned_to(a.noise, 4))
        return DCCN_ERR_INVALID_ARG;
    *sh = ClsRxShape{frames, S, K, CP, P, D, E, kClsRxRows / S};
    *l = ClsRxLink{a.nbits, a.win, a.mode, (D * a.nbits + 7) / 8, a.noise_var, make_float2(a.pv_re, a.pv_im), a.dft, a.w, a.pil,
                   a.dat, a.empty, (const float2*)a.table, a.labels, a.x, a.packed, a.llr, (float2*)a.chest, (float2*)a.y_freq,
                   a.noise};
    return DCCN_OK;
}
// the launch geometry of a shape: a link's tiles on x (the grouped launch: the links on y)
static dim3 clsrx_grid(const ClsRxShape& sh, int n_links) { return dim3((unsigned)ceil_div(sh.frames, sh.fpb), (unsigned)n_links); }
static size_t clsrx_lds(const ClsRxShape& sh) { return clsrx_lds_floats(sh.S, sh.K, sh.P) * sizeof(float); }

int dccn_classical_receive(const dccn_classical_receive_args* a, dccn_stream_t stream) {
    if (!a) return DCCN_ERR_INVALID_ARG;
    const dccn_classical_link link{a->nbits, a->m, a->mode, a->win, a->noise_var, a->pv_re, a->pv_im, a->dft, a->w, a->pil, a->dat,
                                   a->empty, a->table, a->labels, a->x, a->packed, a->llr, a->chest, a->y_freq, a->noise};
    ClsRxParams p;
    DCCN_TRY(clsrx_link_plan(link, a->frames, a->S, a->K, a->CP, a->P, a->D, a->E, &p.l, &p.s));
    DCCN_NO_CHAINS();
    const size_t lds = clsrx_lds(p.s);
    const dim3 grid = clsrx_grid(p.s, 1), block(kClsRxThreads);
    hipStream_t s = (hipStream_t)stream;
    switch (a->nbits) {
        case 1: hipLaunchKernelGGL(classical_receive_kernel<1>, grid, block, lds, s, p); break;
        case 2: hipLaunchKernelGGL(classical_receive_kernel<2>, grid, block, lds, s, p); break;
        case 3: hipLaunchKernelGGL(classical_receive_kernel<3>, grid, block, lds, s, p); break;
        default: hipLaunchKernelGGL(classical_receive_kernel<4>, grid, block, lds, s, p); break;
    }
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// Several links in ONE launch: everything decided before it, so a refused call launches nothing.
static_assert(sizeof(dccn_classical_link) == 136, "dccn.h states the size; dl_ofdm_amd/_lib.py mirrors the layout");
int dccn_classical_receive_grouped(int n_links, const dccn_classical_link* links, int frames, int S, int K, int CP, int P, int D,
                                   int E, dccn_stream_t stream) {
    ClsRxGroupArgs g{};
    DCCN_TRY(group_plan(n_links, links, [&](int i, const dccn_classical_link& a, LinkRanges* r) -> int {
        DCCN_TRY(clsrx_link_plan(a, frames, S, K, CP, P, D, E, &g.link[i], &g.s));
        const size_t n = (size_t)frames, SK = (size_t)S * K;
        r->out(a.packed, n * g.link[i].RB);
        r->out(a.llr, n * D * a.nbits * 4);
        r->out(a.chest, n * SK * 8);
        r->out(a.y_freq, n * SK * 8);
        r->out(a.noise, n * 4);
        r->in(a.x, n * S * (K + CP) * 8);
        r->in(a.dft, (size_t)4 * K * K * 4);
        r->in(a.w, (size_t)P * SK * 4);
        r->in(a.pil, (size_t)P * 4);
        r->in(a.dat, (size_t)D * 4);
        r->in(a.empty, (size_t)E * 4);
        r->in(a.table, (size_t)a.m * 8);
        r->in(a.labels, (size_t)a.m * a.nbits * 4);
        return DCCN_OK;
    }, &dccn_classical_link::llr, &dccn_classical_link::chest, &dccn_classical_link::y_freq, &dccn_classical_link::noise));
    DCCN_NO_CHAINS();                         // (the link table is the call's own, not the group's chain table)
    hipLaunchKernelGGL(classical_receive_grouped_kernel, clsrx_grid(g.s, n_links), dim3(kClsRxThreads), clsrx_lds(g.s),
                       (hipStream_t)stream, g);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

// ---- in-graph AWGN monitor branch (`iq_tx:0`, `iq_rx:0`, `noise_power:0`) -----------------------------------
// clipped / xn: the clipped and the re-normalised signal; norm / clip: the two operators' own workspaces; partial: noise-power
// partials, gx per frame; scratch_pw: complex_clip's power output is `tx_power:0`, served elsewhere
struct IngraphWs { float *clipped, *xn; void *norm, *clip; size_t n_norm, n_clip; double* partial; int gx; float* scratch_pw; };
static IngraphWs ingraph_carve(Carver& c, int frames, int pairs_per_frame) {
    const size_t n_pairs = (size_t)frames * pairs_per_frame;
    IngraphWs w;
    w.clipped = c.take<float>(n_pairs * 2);
    w.xn = c.take<float>(n_pairs * 2);
    w.n_norm = norm_ws_bytes(frames, 2 * pairs_per_frame);
    w.norm = c.take<char>(w.n_norm);
    w.n_clip = dccn_clip_power_workspace_size((long long)n_pairs);
    w.clip = c.take<char>(w.n_clip);
    w.gx = ceil_div(pairs_per_frame, 256);
    w.partial = c.take<double>((size_t)frames * w.gx);
    w.scratch_pw = c.take<float>(64);
    return w;
}
size_t dccn_ingraph_awgn_workspace_size(int frames, int pairs_per_frame) {
    if (frames <= 0 || pairs_per_frame <= 0) return 0;
    return carved_bytes([&](Carver& c) { ingraph_carve(c, frames, pairs_per_frame); });
}
int dccn_ingraph_awgn(const float* x_norm, const float* snr_db, float* tx_signal, uint16_t* iq_tx_f16,
                      uint16_t* iq_rx_f16, float* noise_power, int frames, int pairs_per_frame, float peak,
                      unsigned long long seed, unsigned offset, void* workspace, size_t workspace_bytes,
                      dccn_stream_t stream) {
    if (!x_norm || !snr_db || !noise_power || frames <= 0 || pairs_per_frame <= 0) return DCCN_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < dccn_ingraph_awgn_workspace_size(frames, pairs_per_frame)) return DCCN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const long long n_pairs = (long long)frames * pairs_per_frame;
    Carver c(workspace, workspace_bytes);
    const IngraphWs w = ingraph_carve(c, frames, pairs_per_frame);
    float* xn = w.xn; double* partial = w.partial; const int gx = w.gx;
    float* clip_dst = tx_signal ? tx_signal : w.clipped;
    DCCN_TRY(dccn_clip_power(x_norm, clip_dst, w.scratch_pw, n_pairs, peak, w.clip, w.n_clip, stream));
    dccn_adam_hparams hp;
    memset(&hp, 0, sizeof(hp));
    DCCN_TRY(norm_impl(clip_dst, xn, nullptr, nullptr, false, nullptr, frames, 2 * pairs_per_frame, 1e-8f, peak, nullptr, hp,
                       w.norm, w.n_norm, s));
    hipLaunchKernelGGL(ingraph_awgn_kernel, dim3(gx, frames), dim3(256), 0, s, (const float2*)clip_dst, (const float2*)xn,
                       snr_db, reinterpret_cast<__half2*>(iq_tx_f16), reinterpret_cast<__half2*>(iq_rx_f16), partial,
                       pairs_per_frame, offset, seed);
    DCCN_LAUNCH_CHECK();
    hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, frames * gx, (double)n_pairs,
                       noise_power);
    DCCN_LAUNCH_CHECK();
    return DCCN_OK;
}

}  // extern "C"

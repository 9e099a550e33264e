// Per-frame timing alignment from the cyclic prefix, with or without the carrier-frequency offset taken out.
//
// A frame is T = S * (K + CP) complex samples y[n].  With N = K + CP:
//     p[n] = y[n] * conj(y[n + K])                  e[n] = (|y[n]|^2 + |y[n + K]|^2) / 2
//     Gamma(t) = sum_{s < S} sum_{n < CP} p[s N + t + n]      Phi(t) likewise over e
//     Lambda(t) = |Gamma(t)| - Phi(t)               (<= 0: the rho = 1 form of the ML cyclic-prefix estimator)
//     offset = the smallest t in [-W, W] with the largest Lambda(t);  aligned[n] = y[n + offset]
// A frame s[n] exp(+2 pi i eps n / K) has p = |s|^2 exp(-2 pi i eps), so the angle of Gamma(offset) is the ML estimate of eps (in
// subcarrier spacings, unambiguous for |eps| < 1/2):
//     cfo = -atan2(Im Gamma(offset), Re Gamma(offset)) / (2 pi);  out[n] = aligned[n] exp(-2 pi i cfo n / K),  n = 0 .. T-1
//
// One wave per frame, four frames per 256-thread block; no atomics, every sum in a fixed order (two runs give the same bits).
// The frame is read once (16-byte loads) into the wave's own LDS region, every later step reads LDS, and the frame leaves with
// 16-byte stores: the traffic of the copy the launch stands in for.  The sums, their order, the stores and the derotation are
// stated once (sync_estimate, sync_store, sync_cfo_store); a kernel of this file is a choice along five axes:
//
//   index mapping  where a sample of the frame sits in the wave's LDS region.  SyncCircular: the frame is given on its own and
//                  taken as circular (indices mod T) -- frame_sync_body, gen_apply_sync_kernel (datagen.h).  SyncLinear: the
//                  frame still sits inside one contiguous capture c[n]; frame f nominally starts at b = start + f * stride, its
//                  window [b - W, b + T + W) is indexed linearly (nothing wraps: the samples around the frame are its neighbours
//                  in the air) and out[n] = c[b + offset + n] -- capture_sync_body, capture_pool_cut_kernel.
//   source         the capture's sample format (capture_source.h): CapOfArgs, the float32 capture a link names, or CapSc16, 16-bit
//                  integer I/Q and a scale.  The window loader has one form per format; the sc16 form leaves in LDS, slot for slot,
//                  what the float32 form leaves there for the converted capture, and everything behind the load is the same code.
//   start          capture_start: a link's `first`, or, where first_dev is given, the value read there (what acquisition left on
//                  the device) kept inside [lo, lo + T - 1], the range the host checked every window against.
//   finish         SyncFinish, what follows the estimate: the offset alone; the frame's own cfo taken out; Gamma_f stored for the
//                  pooled sum (one cfo per capture: estimate, capture_pool_reduce_kernel, capture_pool_cut_kernel); or the whole
//                  offset taken out where it exceeds half a spacing (the fraction unwrapped against acquisition's (m^, eps^)).
//   links          one link or up to kMaxChains per launch: the kernels are templates over their argument block (LinkGroup: a
//                  by-value table, the link index on blockIdx.y; OneLink: one link and its source).
//
// The instantiations that exist (the sync unit; gen_apply_sync_kernel is datagen.h's):
//   kernel                                  argument block         entry points
//   frame_sync_kernel, frame_sync_cfo_kernel                       dccn_frame_sync, dccn_frame_sync_cfo
//   frame_sync_grouped_kernel<CFO>          FrameSyncGroupArgs     dccn_frame_sync_grouped
//   capture_sync_kernel<kOffset|kFrameCfo>  CaptureSyncSoloArgs    dccn_capture_sync, dccn_capture_sync_at
//   capture_sync_kernel<kOffset|kFrameCfo>  CaptureSyncGroupArgs   dccn_capture_sync_grouped
//   capture_sync_kernel<kOffset|kFrameCfo>  CaptureSyncSc16Args    dccn_capture_sync_sc16
//   capture_sync_kernel<kWide>              CaptureSyncWideArgs    dccn_capture_sync_wide
//   capture_pool_estimate_kernel            PooledGroupArgs        dccn_capture_sync_pooled(_grouped), dccn_capture_sync_pooled_wide
//   capture_pool_estimate_kernel            PooledSc16Args         dccn_capture_sync_pooled_sc16
//   capture_pool_reduce_kernel              PooledGroupArgs        every pooled entry (it reads no capture)
//   capture_pool_cut_kernel<false>          PooledGroupArgs        dccn_capture_sync_pooled(_grouped)
//   capture_pool_cut_kernel<false>          PooledSc16Args         dccn_capture_sync_pooled_sc16
//   capture_pool_cut_kernel<true>           PooledWideArgs         dccn_capture_sync_pooled_wide
#pragma once
#include "capture_source.h"
#include "common.h"

namespace dccn {

constexpr int kSyncWaves = 4;               // frames per block
constexpr int kSyncLanes = 64;              // one lane per j in [-W, W + CP): 2 W + CP <= 64
constexpr size_t kSyncLdsMax = 64 * 1024;   // a block's LDS (set_max_dynamic_smem raises the kernel's limit past 48 KB)

// LDS of one frame: T complex samples, then (P.re, P.im, E, -) per j
__host__ __device__ static inline size_t frame_sync_lds_per_frame(int T) { return (size_t)T * 8 + (size_t)kSyncLanes * 16; }

static inline bool frame_sync_shape_ok(int S, int K, int CP, int W) {
    if (S < 1 || K < 1 || CP < 1 || W < 1 || W > CP || 2 * W + CP > kSyncLanes) return false;
    const long long T = (long long)S * ((long long)K + CP);
    if (T % 2 != 0 || T > (1 << 20)) return false;
    return kSyncWaves * frame_sync_lds_per_frame((int)T) <= kSyncLdsMax;
}

// The index mapping: slot(j) is the LDS slot of sample j of the nominal frame, j in [-W, W + CP); ahead(slot, d) the slot of the
// sample d in [0, T) further on.
struct SyncCircular {       // the region holds the frame's T samples and indices wrap (W <= CP < T)
    int T;
    __device__ __forceinline__ int slot(const int j) const { return (j + T) % T; }
    __device__ __forceinline__ int ahead(const int slot, const int d) const { return (slot + d) % T; }
};
struct SyncLinear {         // the region holds the window's T + 2 W samples, sample -W in slot 0; nothing wraps
    int W;
    __device__ __forceinline__ int slot(const int j) const { return j + W; }
    __device__ __forceinline__ int ahead(const int slot, const int d) const { return slot + d; }
};

struct FrameSyncArgs {
    const float* x;     // [frames, T, 2]
    float* x_out;       // nullable: [frames, S, out_kin, 2]
    int32_t* offset;    // [frames]
    float* metric;      // nullable: [frames, 2 W + 1]
    int frames, S, K, CP, W;
    int crop;           // 1: x_out rows are the K samples behind each symbol's prefix (out_kin == K)
};

// Steps 2-4 on a frame that sits in the wave's LDS region (y: its samples, placed as `at` says; pe: the kSyncLanes (P, E) slots
// behind them): the frame's offset, the same value in every lane.  The block's barriers are inside: every wave of the block calls
// this, live or not.  Shared by the frame_sync kernels, the capture kernels and gen_apply_sync_kernel (datagen.h): one statement
// of the sums and their order.  gamma_out (nullable): Gamma at the returned offset, the winning lane's sums handed to every lane.
template <class At>
__device__ __forceinline__ int sync_estimate(const At at, const float2* y, float4* pe, const int lane, const bool live, const int S,
                                             const int K, const int CP, const int W, float* metric_row, float2* gamma_out) {
    const int N = K + CP;
    __syncthreads();                                    // (the frame is complete in LDS)

    // 2. P[j], E[j] for j = lane - W in [-W, W + CP): the S symbols in order
    if (live && lane < 2 * W + CP) {
        float pr = 0.f, pi = 0.f, e = 0.f;
        int n = at.slot(lane - W);
        for (int s = 0; s < S; ++s) {
            const float2 u = y[n], v = y[at.ahead(n, K)];
            pr += u.x * v.x + u.y * v.y;
            pi += u.y * v.x - u.x * v.y;
            e += 0.5f * ((u.x * u.x + u.y * u.y) + (v.x * v.x + v.y * v.y));
            n = at.ahead(n, N);
        }
        pe[lane] = make_float4(pr, pi, e, 0.f);
    }
    __syncthreads();

    // 3. one lane per candidate t = lane - W: its CP terms in order
    float lam = -INFINITY;
    float2 gam = make_float2(0.f, 0.f);
    if (live && lane <= 2 * W) {
        float gr = 0.f, gi = 0.f, phi = 0.f;
        for (int n = 0; n < CP; ++n) {
            const float4 t = pe[lane + n];
            gr += t.x;
            gi += t.y;
            phi += t.z;
        }
        lam = sqrtf(gr * gr + gi * gi) - phi;
        if (metric_row) metric_row[lane] = lam;
        if (gamma_out) gam = make_float2(gr, gi);
    }

    // 4. the wave's maximum, the smallest candidate on ties (every lane takes part; lanes past 2 W hold -inf)
    int best = lane;
    for (int d = 1; d < kSyncLanes; d <<= 1) {
        const float ol = __shfl_xor(lam, d);
        const int ob = __shfl_xor(best, d);
        if (ol > lam || (ol == lam && ob < best)) {
            lam = ol;
            best = ob;
        }
    }
    // lane 0's view, for every lane; kept inside the candidates whatever the samples were (NaN compares false everywhere)
    best = __shfl(best, 0);
    best = best < 0 ? 0 : (best > 2 * W ? 2 * W : best);
    if (gamma_out) *gamma_out = make_float2(__shfl(gam.x, best), __shfl(gam.y, best));
    return best - W;
}
// the circular frame (the frame_sync kernels and gen_apply_sync_kernel)
__device__ __forceinline__ int frame_sync_estimate(const float2* y, float4* pe, const int lane, const bool live, const int S,
                                                   const int K, const int CP, const int W, float* metric_row,
                                                   float2* gamma_out = nullptr) {
    return sync_estimate(SyncCircular{S * (K + CP)}, y, pe, lane, live, S, K, CP, W, metric_row, gamma_out);
}

// Step 5: the frame from its sample theta on, from LDS to dst (the frame's [S, K + CP, 2] rows, or crop: its [S, K, 2] rows behind
// each symbol's prefix): two complex samples per 16-byte store, each read at its own (shifted) place
template <class At>
__device__ __forceinline__ void sync_store(const At at, const float2* y, float* dst_, const int theta, const int lane, const int S,
                                           const int K, const int CP, const int crop) {
    const int N = K + CP, T = S * N;
    const int rot = at.slot(theta);
    float4* dst = reinterpret_cast<float4*>(dst_);
    if (crop) {
        const int M = S * K;
        for (int i = lane; i < M / 2; i += kSyncLanes) {
            const int m0 = 2 * i, m1 = 2 * i + 1;
            const float2 u = y[at.ahead(rot, (m0 / K) * N + CP + m0 % K)];
            const float2 v = y[at.ahead(rot, (m1 / K) * N + CP + m1 % K)];
            dst[i] = make_float4(u.x, u.y, v.x, v.y);
        }
    } else {
        for (int i = lane; i < T / 2; i += kSyncLanes) {
            const float2 u = y[at.ahead(rot, 2 * i)], v = y[at.ahead(rot, 2 * i + 1)];
            dst[i] = make_float4(u.x, u.y, v.x, v.y);
        }
    }
}
__device__ __forceinline__ void frame_sync_store(const float2* y, float* dst_, const int theta, const int lane, const int S,
                                                 const int K, const int CP, const int crop) {
    sync_store(SyncCircular{S * (K + CP)}, y, dst_, theta, lane, S, K, CP, crop);
}

// Step 5 of the CFO variant: sample n of the ALIGNED frame leaves as aligned[n] * exp(-2 pi i cfo n / K).  The phase is taken in
// turns: cfo * n and the division by K are its only two roundings (|turns| < 4.4), turns - rint(turns) is exact, and sincospif
// reduces no further.  Same places, same stores as frame_sync_store.
__device__ __forceinline__ float2 frame_cfo_derotate(const float2 u, const float cfo, const int n, const float fK) {
    const float turns = cfo * (float)n / fK;
    float sn, cs;
    sincospif(2.0f * (turns - rintf(turns)), &sn, &cs);
    return make_float2(u.x * cs + u.y * sn, u.y * cs - u.x * sn);
}
// The wide finish: the offset is I + cfo with I a whole number of spacings, 0 <= ipos < K its residue mod K.  I n / K turns are
// whole but for (ipos n mod K) / K, an exact integer over K, so the phase keeps the roundings above however large I is; with
// ipos = 0 the turns are the expression above, bit for bit (0 + a = a).  ipos n stays below K T < 2^22: four frames of T samples
// fit a block's LDS (frame_sync_shape_ok), so T <= 1920.
__device__ __forceinline__ float2 frame_cfo_derotate_wide(const float2 u, const unsigned ipos, const float cfo, const int n,
                                                          const int K, const float fK) {
    const float turns = ((float)(ipos * (unsigned)n % (unsigned)K) + cfo * (float)n) / fK;
    float sn, cs;
    sincospif(2.0f * (turns - rintf(turns)), &sn, &cs);
    return make_float2(u.x * cs + u.y * sn, u.y * cs - u.x * sn);
}
template <class At, bool WIDE = false>
__device__ __forceinline__ void sync_cfo_store(const At at, const float2* y, float* dst_, const int theta, const float cfo,
                                               const int lane, const int S, const int K, const int CP, const int crop,
                                               const unsigned ipos = 0) {
    const int N = K + CP, T = S * N;
    const int rot = at.slot(theta);
    const float fK = (float)K;
    float4* dst = reinterpret_cast<float4*>(dst_);
    const int M = crop ? S * K : T;
    for (int i = lane; i < M / 2; i += kSyncLanes) {
        const int m0 = 2 * i, m1 = 2 * i + 1;
        const int n0 = crop ? (m0 / K) * N + CP + m0 % K : m0, n1 = crop ? (m1 / K) * N + CP + m1 % K : m1;
        float2 u, v;
        if constexpr (WIDE) {
            u = frame_cfo_derotate_wide(y[at.ahead(rot, n0)], ipos, cfo, n0, K, fK);
            v = frame_cfo_derotate_wide(y[at.ahead(rot, n1)], ipos, cfo, n1, K, fK);
        } else {
            u = frame_cfo_derotate(y[at.ahead(rot, n0)], cfo, n0, fK);
            v = frame_cfo_derotate(y[at.ahead(rot, n1)], cfo, n1, fK);
        }
        dst[i] = make_float4(u.x, u.y, v.x, v.y);
    }
}

// The estimate read off a correlation sum, in subcarrier spacings (0 - a: +0 where the angle is 0)
__device__ __forceinline__ float cfo_of_gamma(const float2 gamma) { return 0.f - atan2f(gamma.y, gamma.x) / 6.283185307179586f; }

// What follows the estimate, stated once: the offset, the CFO variant's estimate, and the frame on its way out.
template <bool CFO, class At>
__device__ __forceinline__ void sync_finish(const At at, const float2* y, const long long f, const int theta, const float2 gamma,
                                            const int lane, float* x_out, int32_t* offset, float* cfo_out, const int S, const int K,
                                            const int CP, const int crop) {
    if (lane == 0) offset[f] = theta;
    float* const dst = x_out + (size_t)f * S * (crop ? K : K + CP) * 2;
    if constexpr (CFO) {
        const float cfo = cfo_of_gamma(gamma);
        if (lane == 0) cfo_out[f] = cfo;
        if (x_out) sync_cfo_store(at, y, dst, theta, cfo, lane, S, K, CP, crop);
    } else {
        if (x_out) sync_store(at, y, dst, theta, lane, S, K, CP, crop);
    }
}

// The prefix's fraction unwrapped against what acquisition left on the device (dccn_capture_acquire_wide: m^ and eps^_acq):
//     ref = (float)m^ + eps^_acq       I = rint(ref - frac), kept inside [-K/2, K/2] (a NaN difference: 0)
// so a wild device value costs a wrong derotation and nothing else.  ipos = I mod K in [0, K).
struct CfoWide {
    const int32_t* cfo_int;     // [1]
    const float* cfo_frac;      // [1]
};
__device__ __forceinline__ int cfo_unwrap(const float frac, const CfoWide w, const int K, unsigned* ipos) {
    const float lim = (float)(K / 2);
    const float d = rintf(((float)w.cfo_int[0] + w.cfo_frac[0]) - frac);
    const int I = d > lim ? K / 2 : (d < -lim ? -(K / 2) : (d == d ? (int)d : 0));
    *ipos = (unsigned)((I % K + K) % K);
    return I;
}
// sync_finish of the wide variant: cfo_out[f] holds the total, the frame leaves with the whole offset taken out
template <class At>
__device__ __forceinline__ void sync_finish_wide(const At at, const float2* y, const long long f, const int theta, const float2 gamma,
                                                 const int lane, float* x_out, int32_t* offset, float* cfo_out, const int S,
                                                 const int K, const int CP, const int crop, const CfoWide w) {
    if (lane == 0) offset[f] = theta;
    const float frac = cfo_of_gamma(gamma);
    unsigned ipos;
    const int I = cfo_unwrap(frac, w, K, &ipos);
    if (lane == 0) cfo_out[f] = (float)I + frac;
    if (x_out)
        sync_cfo_store<At, true>(at, y, x_out + (size_t)f * S * (crop ? K : K + CP) * 2, theta, frac, lane, S, K, CP, crop, ipos);
}

// The launch on frames given on their own, stated once; CFO selects the variant (cfo_out [frames] is written by that variant only).
template <bool CFO>
__device__ __forceinline__ void frame_sync_body(const FrameSyncArgs& a, float* cfo_out) {
    extern __shared__ float4 sync_lds[];
    const int lane = threadIdx.x & (kSyncLanes - 1), wave = threadIdx.x / kSyncLanes;
    const int T = a.S * (a.K + a.CP), W = a.W;
    const long long f = (long long)blockIdx.x * kSyncWaves + wave;
    const bool live = f < a.frames;          // (a ragged last block: the wave still meets the block's barriers)
    float4* const region = sync_lds + (size_t)wave * (frame_sync_lds_per_frame(T) / 16);
    float2* const y = reinterpret_cast<float2*>(region);
    float4* const pe = region + T / 2;

    // 1. the frame, once, into LDS
    if (live) {
        const float4* src = reinterpret_cast<const float4*>(a.x + (size_t)f * T * 2);
        for (int i = lane; i < T / 2; i += kSyncLanes) region[i] = src[i];
    }
    float2 gamma = make_float2(0.f, 0.f);
    const int theta = frame_sync_estimate(y, pe, lane, live, a.S, a.K, a.CP, W,
                                          (live && a.metric) ? a.metric + (size_t)f * (2 * W + 1) : nullptr, CFO ? &gamma : nullptr);
    if (!live) return;
    sync_finish<CFO>(SyncCircular{T}, y, f, theta, gamma, lane, a.x_out, a.offset, cfo_out, a.S, a.K, a.CP, a.crop);
}

static __global__ void __launch_bounds__(kSyncWaves * kSyncLanes) frame_sync_kernel(const FrameSyncArgs a) {
    frame_sync_body<false>(a, nullptr);
}

struct FrameSyncCfoArgs {
    FrameSyncArgs s;
    float* cfo;         // [frames]
};
static __global__ void __launch_bounds__(kSyncWaves * kSyncLanes) frame_sync_cfo_kernel(const FrameSyncCfoArgs a) {
    frame_sync_body<true>(a.s, a.cfo);
}

// Several links per launch (dccn_frame_sync_grouped): each link has its own frames and outputs; frames, the shape, W and out_kin
// are the call's.  The table travels by value in the kernel arguments and is indexed by blockIdx.y, a block-uniform value (scalar
// loads, as ChainOffs is read); blockIdx.x stays what the body takes it for, so a link's blocks are the solo launch's.
struct FrameSyncLink {
    const float* x;
    float* x_out;
    int32_t* offset;
    float* metric;
    float* cfo;
};
struct FrameSyncGroupArgs {
    FrameSyncLink link[kMaxChains];
    int frames, S, K, CP, W, crop;
};
template <bool CFO>
static __global__ void __launch_bounds__(kSyncWaves * kSyncLanes) frame_sync_grouped_kernel(const FrameSyncGroupArgs g) {
    const FrameSyncLink& l = g.link[blockIdx.y];
    frame_sync_body<CFO>(FrameSyncArgs{l.x, l.x_out, l.offset, l.metric, g.frames, g.S, g.K, g.CP, g.W, g.crop}, l.cfo);
}

// ---- frames cut from a contiguous capture ---------------------------------------------------------------------------------------
// Frame f's window is the samples [b - W, b + T + W) of the capture, b = start + f * stride; it is all the wave reads.  The
// capture's base is 16-byte aligned, so EVEN samples are: the wave's region starts at the even sample a0 = (b - W) & ~1 and holds
// pairs (a0 + 2 i, a0 + 2 i + 1), one 16-byte load each.  A window that starts on an odd sample has its first sample in the
// upper half of pair 0, and then (T + 2 W is even) its last sample in the lower half of the last pair: those two pairs are read
// with one 8-byte load of the half that belongs to the window, so no lane reads a sample outside it -- the neighbour may lie
// past either end of the capture.  The window then sits in the region from slot sh = (b - W) & 1 on; one spare pair per frame.
__host__ __device__ static inline size_t capture_sync_lds_per_frame(int T, int W) {
    return (size_t)(T + 2 * W + 2) * 8 + (size_t)kSyncLanes * 16;
}

static inline bool capture_sync_shape_ok(int S, int K, int CP, int W) {
    if (!frame_sync_shape_ok(S, K, CP, W)) return false;
    return kSyncWaves * capture_sync_lds_per_frame(S * (K + CP), W) <= kSyncLdsMax;
}

// What a launch's links share, and what one link of a capture cut is.
struct SyncShape {
    int frames, S, K, CP, W;
    int crop;                   // 1: x_out rows are the K samples behind each symbol's prefix (out_kin == K)
};
struct CaptureSyncLink {
    const float* cap;           // [n_samples, 2]; not read where the argument block names another source
    long long first, stride;    // frame f nominally starts at sample start + f * stride
    const long long* first_dev; // nullable [1]: the start is read here and kept inside [lo, lo + T - 1]
    long long lo;
    float* x_out;               // nullable: [frames, S, out_kin, 2]
    int32_t* offset;            // [frames]
    float* metric;              // nullable: [frames, 2 W + 1]
    float* cfo;                 // per-frame finishes: [frames]; pooled: [1], the capture's estimate
};
// Where frame 0 nominally starts: `first`, or what the device holds kept inside the range the host checked every window against,
// so a wrong value cannot read outside the capture.  first_dev is the same for every thread of a block.
__device__ __forceinline__ long long capture_start(const CaptureSyncLink& l, const int T) {
    if (!l.first_dev) return l.first;
    const long long hi = l.lo + T - 1;
    const long long got = l.first_dev[0];
    return got < l.lo ? l.lo : (got > hi ? hi : got);
}

// The argument blocks the capture kernels are templates over: at(y) the link of grid row y, source() where its samples come from.
template <class Link>
struct LinkGroup {              // up to kMaxChains links, each naming its own float32 capture
    Link link[kMaxChains];
    SyncShape shape;
    __device__ __forceinline__ const Link& at(const unsigned y) const { return link[y]; }
    __device__ __forceinline__ CapOfArgs source() const { return CapOfArgs{}; }
};
template <class Link, class Src>
struct OneLink {                // one link and its source
    Link link;
    Src src;
    SyncShape shape;
    __device__ __forceinline__ const Link& at(const unsigned) const { return link; }
    __device__ __forceinline__ Src source() const { return src; }
};

// The samples [start, start + len) of the capture (len even) into a wave's region, as stated above: the region's pair i holds the
// samples (a0 + 2 i, a0 + 2 i + 1), a0 = start & ~1, so sample `start` sits in slot start & 1.
__device__ __forceinline__ void capture_window_load(float4* region, const float* cap, const long long start, const int len,
                                                    const int lane) {
    const int sh = (int)(start & 1);
    const float2* const src2 = reinterpret_cast<const float2*>(cap) + (start - sh);
    const float4* const src4 = reinterpret_cast<const float4*>(src2);
    const int pairs = (len + 2 * sh) / 2;            // sh = 1: one more pair, the first and the last half inside
    for (int i = lane; i < pairs; i += kSyncLanes) {
        float4 v;
        if (sh && i == 0) {
            const float2 h = src2[1];
            v = make_float4(0.f, 0.f, h.x, h.y);
        } else if (sh && i == pairs - 1) {
            const float2 h = src2[2 * i];
            v = make_float4(h.x, h.y, 0.f, 0.f);
        } else {
            v = src4[i];
        }
        region[i] = v;
    }
}

__device__ __forceinline__ void capture_window_load(float4* region, const CapF32 src, const long long start, const int len,
                                                    const int lane) {
    capture_window_load(region, reinterpret_cast<const float*>(src), start, len, lane);
}
// The sc16 form: the same samples into the same slots.  A sample is 4 bytes, so the capture's 16-byte units are QUADS of samples:
// with r = start & 3 the window is the samples [r, r + len) counted from quad 0's first sample, a quad that lies inside it is one
// 16-byte load (four samples: the region's pairs 2 j - h and 2 j + 1 - h, h = r >> 1 -- the region starts at the even sample
// start & ~1, which is sample 2 h of quad 0), and the quads the window's head and tail cut through are read pair by pair: an
// 8-byte load where both samples belong to the window, a 4-byte load of the one that does (the other half of the region's pair is
// written as 0, as the float32 loader writes it), nothing where neither does.  No lane reads a sample outside the window: the 16
// bytes of its last quad may reach past the capture's end, and are then not read whole.
__device__ __forceinline__ void capture_window_load(float4* region, const CapSc16 src, const long long start, const int len,
                                                    const int lane) {
    const int r = (int)(start & 3), h = r >> 1, end = r + len;
    const uint32_t* const s1 = reinterpret_cast<const uint32_t*>(src.cap) + (start - r);
    const uint2* const s2 = reinterpret_cast<const uint2*>(s1);
    const uint4* const s4 = reinterpret_cast<const uint4*>(s1);
    const int quads = (end + 3) / 4;
    for (int j = lane; j < quads; j += kSyncLanes) {
        const int s = 4 * j;
        if (s >= r && s + 4 <= end) {
            const uint4 w = s4[j];
            const float2 a = CapSc16::value(w.x, src.scale), b = CapSc16::value(w.y, src.scale);
            const float2 c = CapSc16::value(w.z, src.scale), d = CapSc16::value(w.w, src.scale);
            region[2 * j - h] = make_float4(a.x, a.y, b.x, b.y);
            region[2 * j + 1 - h] = make_float4(c.x, c.y, d.x, d.y);
        } else {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int s0 = s + 2 * p;
                const bool in0 = s0 >= r && s0 < end, in1 = s0 + 1 >= r && s0 + 1 < end;
                if (!in0 && !in1) continue;
                float2 u = make_float2(0.f, 0.f), v = make_float2(0.f, 0.f);
                if (in0 && in1) {
                    const uint2 w = s2[2 * j + p];
                    u = CapSc16::value(w.x, src.scale);
                    v = CapSc16::value(w.y, src.scale);
                } else if (in0) {
                    u = CapSc16::value(s1[s0], src.scale);
                } else {
                    v = CapSc16::value(s1[s0 + 1], src.scale);
                }
                region[2 * j + p - h] = make_float4(u.x, u.y, v.x, v.y);
            }
        }
    }
}

// What follows the estimate of a capture's frame.
enum class SyncFinish {
    kOffset,        // offset[f]; the aligned frame leaves as it is
    kFrameCfo,      // and cfo[f], the frame's own estimate, taken out of the frame
    kPool,          // offset[f] and Gamma_f(offset[f]) to gamma_ws[f]; no frame is written (the pooled call's estimate pass)
    kWide,          // kFrameCfo with the fraction unwrapped against `wide`: cfo[f] holds the total, which is taken out
};

// The launch, stated once: link l's frames of shape g from the source src.  gamma_ws: kPool's store; wide: kWide's device inputs.
template <SyncFinish FIN, class Src>
__device__ __forceinline__ void capture_sync_body(const CaptureSyncLink& l, const SyncShape& g, const Src src,
                                                  float2* gamma_ws = nullptr, const CfoWide wide = CfoWide{nullptr, nullptr}) {
    extern __shared__ float4 sync_lds[];
    const int lane = threadIdx.x & (kSyncLanes - 1), wave = threadIdx.x / kSyncLanes;
    const int T = g.S * (g.K + g.CP), W = g.W;
    const long long first = capture_start(l, T);
    const long long f = (long long)blockIdx.x * kSyncWaves + wave;
    const bool live = f < g.frames;          // (a ragged last block: the wave still meets the block's barriers)
    const size_t per = capture_sync_lds_per_frame(T, W) / 16;
    float4* const region = sync_lds + (size_t)wave * per;
    float4* const pe = region + (per - kSyncLanes);
    const long long start = live ? first + f * l.stride - W : 0;            // the window's first sample
    const int sh = (int)(start & 1);
    const float2* const y = reinterpret_cast<const float2*>(region) + sh;    // slot 0 = sample start

    // 1. the window, once, into LDS
    if (live) capture_window_load(region, src.of(l), start, T + 2 * W, lane);
    const SyncLinear at{W};
    float2 gamma = make_float2(0.f, 0.f);
    const int theta = sync_estimate(at, y, pe, lane, live, g.S, g.K, g.CP, W,
                                    (live && l.metric) ? l.metric + (size_t)f * (2 * W + 1) : nullptr,
                                    FIN != SyncFinish::kOffset ? &gamma : nullptr);
    if (!live) return;
    if constexpr (FIN == SyncFinish::kPool) {
        if (lane == 0) {
            l.offset[f] = theta;
            gamma_ws[f] = gamma;
        }
    } else if constexpr (FIN == SyncFinish::kWide) {
        sync_finish_wide(at, y, f, theta, gamma, lane, l.x_out, l.offset, l.cfo, g.S, g.K, g.CP, g.crop, wide);
    } else {
        sync_finish<FIN == SyncFinish::kFrameCfo>(at, y, f, theta, gamma, lane, l.x_out, l.offset, l.cfo, g.S, g.K, g.CP, g.crop);
    }
}

// The per-frame cut over its argument block: one kernel text serves a host start and a device one, one link and several, both
// sample formats.  The float32 solo calls have a one-link block of their own: as the one-link case of the group block (8 links by
// value, 600 bytes of kernel arguments) the call measured 0.3 - 0.6 us longer on the host (profiles/capture_front_once.md).
using CaptureSyncGroupArgs = LinkGroup<CaptureSyncLink>;
using CaptureSyncSoloArgs = OneLink<CaptureSyncLink, CapOfArgs>;
using CaptureSyncSc16Args = OneLink<CaptureSyncLink, CapSc16>;
struct CaptureSyncWideArgs : CaptureSyncSoloArgs {
    CfoWide wide;
};
template <SyncFinish FIN, class Args>
static __global__ void __launch_bounds__(kSyncWaves * kSyncLanes) capture_sync_kernel(const Args g) {
    static_assert(FIN != SyncFinish::kPool, "the pooled estimate is capture_pool_estimate_kernel");
    if constexpr (FIN == SyncFinish::kWide)
        capture_sync_body<FIN>(g.at(blockIdx.y), g.shape, g.source(), nullptr, g.wide);
    else
        capture_sync_body<FIN>(g.at(blockIdx.y), g.shape, g.source());
}

// ---- one carrier offset per capture, pooled over its frames -----------------------------------------------------------------------
// A capture comes from one front end with one oscillator: its frames share one offset, so the estimate is taken from
//     Gamma = sum_{f < frames} Gamma_f(offset[f]),    cfo = 0 - atan2(Im Gamma, Re Gamma) / (2 pi)
// and every frame is derotated with that one value.  No frame can leave before every frame's Gamma_f is known, so the call is
// three launches on the stream, each complete before the next starts (no block waits for another, no atomics, no host round trip):
//   estimate  capture_sync_body<kPool>: the per-frame estimate, offset[f] and Gamma_f(offset[f]) stored (workspace: float2 [frames])
//   reduce    one wave per link.  THE ORDER OF THE SUM: lane l adds Gamma_l, Gamma_{l+64}, Gamma_{l+128}, ... in ascending
//             order onto +0; then a butterfly over the 64 lanes, d = 1, 2, 4, 8, 16, 32: every lane adds the value of lane
//             (l xor d) to its own (both partners add the same two numbers, so all lanes hold the same bits).  Real and
//             imaginary parts are summed separately.  The order depends on `frames` alone -- not on a grid, the link count or
//             whether the call is grouped.  A Gamma_f passes through at most ceil(frames / 64) - 1 + 6 rounded additions.
//   cut       one wave per frame, four per block: offset[f] is read back and CLAMPED into [-W, W] before it indexes (the frame
//             [b_f + offset, b_f + offset + T) then lies inside the window [b_f - W, b_f + T + W) the host checked), the frame is
//             loaded as the window is (aligned 16-byte pairs, one 8-byte half at each end when it starts on an odd sample) and
//             leaves through sync_cfo_store with the capture's cfo: the derotation and the 16-byte stores of the per-frame path.
//             WIDE: the reduce left the capture's FRACTION in link.s.cfo (a workspace slot every block reads); it is unwrapped
//             in front of the store and frame 0's wave writes the total to total_out.
// The solo entry is the grouped one with one link: the link index rides on blockIdx.y (reduce: blockIdx.x).
__host__ __device__ static inline size_t capture_cut_lds_per_frame(int T) { return (size_t)(T + 2) * 8; }
constexpr int kPoolAhead = 16;              // the reduce launch's loads in flight per lane

struct PooledLink {
    CaptureSyncLink s;          // s.cfo: [1], the capture's estimate
    float2* gamma;              // [frames]: Gamma_f(offset[f])
};
struct PooledGroupArgs : LinkGroup<PooledLink> {};     // (a type of its own: capture_pool_reduce_kernel keeps its symbol)
using PooledSc16Args = OneLink<PooledLink, CapSc16>;
struct PooledWideArgs : OneLink<PooledLink, CapOfArgs> {
    CfoWide wide;
    float* total_out;           // [1]
};

template <class Args>
static __global__ void __launch_bounds__(kSyncWaves * kSyncLanes) capture_pool_estimate_kernel(const Args g) {
    const PooledLink& l = g.at(blockIdx.y);
    capture_sync_body<SyncFinish::kPool>(l.s, g.shape, g.source(), l.gamma);
}

static __global__ void __launch_bounds__(kSyncLanes) capture_pool_reduce_kernel(const PooledGroupArgs g) {
    const PooledLink& l = g.link[blockIdx.x];
    const int lane = threadIdx.x;
    const int frames = g.shape.frames;
    float gr = 0.f, gi = 0.f;
    // the lane's terms, kPoolAhead loads in flight at a time (their latency is all this launch waits for); added in the stated order
    for (int f0 = lane; f0 < frames; f0 += kSyncLanes * kPoolAhead) {
        float2 t[kPoolAhead];
#pragma unroll
        for (int u = 0; u < kPoolAhead; ++u) {
            const int f = f0 + u * kSyncLanes;
            t[u] = f < frames ? l.gamma[f] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < kPoolAhead; ++u) {
            if (f0 + u * kSyncLanes < frames) {
                gr += t[u].x;
                gi += t[u].y;
            }
        }
    }
    for (int d = 1; d < kSyncLanes; d <<= 1) {
        gr += __shfl_xor(gr, d);
        gi += __shfl_xor(gi, d);
    }
    if (lane == 0) l.s.cfo[0] = cfo_of_gamma(make_float2(gr, gi));
}

template <bool WIDE, class Args>
static __global__ void __launch_bounds__(kSyncWaves * kSyncLanes) capture_pool_cut_kernel(const Args a) {
    extern __shared__ float4 sync_lds[];
    const PooledLink& l = a.at(blockIdx.y);
    const SyncShape& g = a.shape;
    const int lane = threadIdx.x & (kSyncLanes - 1), wave = threadIdx.x / kSyncLanes;
    const int T = g.S * (g.K + g.CP), W = g.W;
    const long long f = (long long)blockIdx.x * kSyncWaves + wave;
    const bool live = f < g.frames;
    float4* const region = sync_lds + (size_t)wave * (capture_cut_lds_per_frame(T) / 16);
    long long start = 0;
    if (live) {
        const int got = l.s.offset[f];
        start = capture_start(l.s, T) + f * l.s.stride + (got < -W ? -W : (got > W ? W : got));
    }
    const float2* const y = reinterpret_cast<const float2*>(region) + (int)(start & 1);      // slot 0 = sample start
    if (live) capture_window_load(region, a.source().of(l.s), start, T, lane);
    __syncthreads();                                    // (the frame is complete in LDS)
    if (!live) return;
    const float cfo = l.s.cfo[0];
    unsigned ipos = 0;
    if constexpr (WIDE) {
        const int I = cfo_unwrap(cfo, a.wide, g.K, &ipos);
        if (f == 0 && lane == 0) a.total_out[0] = (float)I + cfo;
    }
    sync_cfo_store<SyncLinear, WIDE>(SyncLinear{0}, y, l.s.x_out + (size_t)f * g.S * (g.crop ? g.K : g.K + g.CP) * 2, 0, cfo, lane,
                                     g.S, g.K, g.CP, g.crop, ipos);
}

}  // namespace dccn

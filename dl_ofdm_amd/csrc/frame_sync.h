// Per-frame timing alignment from the cyclic prefix (dccn_frame_sync), and its variant that also estimates
// and removes the carrier-frequency offset (dccn_frame_sync_cfo).
//
// A frame is T = S * (K + CP) complex samples y[n], taken as circular (indices mod T).  With N = K + CP:
//     p[n] = y[n] * conj(y[n + K])                  e[n] = (|y[n]|^2 + |y[n + K]|^2) / 2
//     Gamma(t) = sum_{s < S} sum_{n < CP} p[s N + t + n]      Phi(t) likewise over e
//     Lambda(t) = |Gamma(t)| - Phi(t)               (<= 0: the rho = 1 form of the ML cyclic-prefix estimator)
//     offset = the smallest t in [-W, W] with the largest Lambda(t);  aligned[n] = y[(n + offset) mod T]
// CFO variant: a frame s[n] exp(+2 pi i eps n / K) has p = |s|^2 exp(-2 pi i eps), so the angle of Gamma(offset) is the ML estimate
// of eps (in subcarrier spacings, unambiguous for |eps| < 1/2):
//     cfo = -atan2(Im Gamma(offset), Re Gamma(offset)) / (2 pi);  out[n] = aligned[n] exp(-2 pi i cfo n / K),  n = 0 .. T-1
//
// One wave per frame, four frames per 256-thread block; no atomics, no workspace, every sum in a fixed order (two runs give
// the same bits).  The frame is read once (16-byte loads) into the wave's own LDS region, every later step reads LDS, and the
// rotated frame leaves with 16-byte stores: the traffic of the copy the launch stands in for.
#pragma once
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

struct FrameSyncArgs {
    const float* x;     // [frames, T, 2]
    float* x_out;       // nullable: [frames, S, out_kin, 2]
    int32_t* offset;    // [frames]
    float* metric;      // nullable: [frames, 2 W + 1]
    int frames, S, K, CP, W;
    int crop;           // 1: x_out rows are the K samples behind each symbol's prefix (out_kin == K)
};

// Steps 2-4 on a frame that sits in the wave's LDS region (y: its T samples, pe: the kSyncLanes (P, E) slots behind them):
// the frame's offset, the same value in every lane.  The block's barriers are inside: every wave of the block calls this, live or
// not.  Shared by the frame_sync kernels and gen_apply_sync_kernel (datagen.h): one statement of the sums and their order.
// gamma_out (nullable): Gamma at the returned offset, the winning lane's sums handed to every lane.
__device__ __forceinline__ int frame_sync_estimate(const float2* y, float4* pe, const int lane, const bool live, const int S,
                                                   const int K, const int CP, const int W, float* metric_row,
                                                   float2* gamma_out = nullptr) {
    const int N = K + CP, T = S * N;
    __syncthreads();                                    // (the frame is complete in LDS)

    // 2. P[j], E[j] for j = lane - W in [-W, W + CP): the S symbols in order
    if (live && lane < 2 * W + CP) {
        float pr = 0.f, pi = 0.f, e = 0.f;
        int n = (lane - W + T) % T;                     // (W <= CP < T)
        for (int s = 0; s < S; ++s) {
            const float2 u = y[n], v = y[(n + K) % T];
            pr += u.x * v.x + u.y * v.y;
            pi += u.y * v.x - u.x * v.y;
            e += 0.5f * ((u.x * u.x + u.y * u.y) + (v.x * v.x + v.y * v.y));
            n = (n + N) % T;
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

// Step 5: the frame rotated by theta, from LDS to dst (the frame's [S, K + CP, 2] rows, or crop: its [S, K, 2] rows behind each
// symbol's prefix): two complex samples per 16-byte store, each read at its own (shifted) place
__device__ __forceinline__ void frame_sync_store(const float2* y, float* dst_, const int theta, const int lane, const int S,
                                                 const int K, const int CP, const int crop) {
    const int N = K + CP, T = S * N;
    const int rot = (theta + T) % T;
    float4* dst = reinterpret_cast<float4*>(dst_);
    if (crop) {
        const int M = S * K;
        for (int i = lane; i < M / 2; i += kSyncLanes) {
            const int m0 = 2 * i, m1 = 2 * i + 1;
            const float2 u = y[((m0 / K) * N + CP + m0 % K + rot) % T];
            const float2 v = y[((m1 / K) * N + CP + m1 % K + rot) % T];
            dst[i] = make_float4(u.x, u.y, v.x, v.y);
        }
    } else {
        for (int i = lane; i < T / 2; i += kSyncLanes) {
            const float2 u = y[(2 * i + rot) % T], v = y[(2 * i + 1 + rot) % T];
            dst[i] = make_float4(u.x, u.y, v.x, v.y);
        }
    }
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
__device__ __forceinline__ void frame_cfo_store(const float2* y, float* dst_, const int theta, const float cfo, const int lane,
                                                const int S, const int K, const int CP, const int crop) {
    const int N = K + CP, T = S * N;
    const int rot = (theta + T) % T;
    const float fK = (float)K;
    float4* dst = reinterpret_cast<float4*>(dst_);
    const int M = crop ? S * K : T;
    for (int i = lane; i < M / 2; i += kSyncLanes) {
        const int m0 = 2 * i, m1 = 2 * i + 1;
        const int n0 = crop ? (m0 / K) * N + CP + m0 % K : m0, n1 = crop ? (m1 / K) * N + CP + m1 % K : m1;
        const float2 u = frame_cfo_derotate(y[(n0 + rot) % T], cfo, n0, fK);
        const float2 v = frame_cfo_derotate(y[(n1 + rot) % T], cfo, n1, fK);
        dst[i] = make_float4(u.x, u.y, v.x, v.y);
    }
}

// The launch, stated once; CFO selects the variant (cfo_out [frames] is written by that variant only).
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
    float2 gamma;
    const int theta = frame_sync_estimate(y, pe, lane, live, a.S, a.K, a.CP, W,
                                          (live && a.metric) ? a.metric + (size_t)f * (2 * W + 1) : nullptr, CFO ? &gamma : nullptr);
    if (!live) return;
    if (lane == 0) a.offset[f] = theta;
    float* const dst = a.x_out + (size_t)f * a.S * (a.crop ? a.K : a.K + a.CP) * 2;
    if constexpr (CFO) {
        const float cfo = 0.f - atan2f(gamma.y, gamma.x) / 6.283185307179586f;     // (0 - a: +0 where the angle is 0)
        if (lane == 0) cfo_out[f] = cfo;
        if (a.x_out) frame_cfo_store(y, dst, theta, cfo, lane, a.S, a.K, a.CP, a.crop);
    } else {
        if (a.x_out) frame_sync_store(y, dst, theta, lane, a.S, a.K, a.CP, a.crop);
    }
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

}  // namespace dccn

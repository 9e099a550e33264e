// Coarse acquisition inside a contiguous capture (dccn_capture_acquire): where in [lo, lo + T) the first
// frame starts, found on the device and left there for dccn_capture_sync_at (frame_sync.h).
//
// c = the capture indexed linearly, N = K + CP, T = S N, J frames back to back from the (unknown) start on;
// p[n] = c[n] conj(c[n + K]), e[n] = (|c[n]|^2 + |c[n + K]|^2) / 2 as in frame_sync.h.
//
// Stage A, symbol timing and carrier offset over a whole symbol period (the cyclic-prefix estimator with J S symbols and every
// lag of one period):
//     P[m] = sum_{u < J S} p[lo + m + u N]   (u ascending)          E[m] likewise over e          m in [0, N + CP - 1)
//     Gamma(r) = sum_{n < CP} P[r + n]       (n ascending)          Phi(r) likewise over E        r in [0, N)
//     Lambda(r) = |Gamma(r)| - Phi(r)        r^ = the smallest r with the largest Lambda         eps^ = -atan2(Im, Re Gamma(r^)) / 2 pi
// Stage B, which of the S symbol positions is the frame's first: the pilot symbols (the symbols that hold at least two pilot
// cells; k_0 < k_1 < ... the pilot carriers of pilot symbol s) carry the same value on every pilot carrier, so adjacent pilot
// bins of a pilot symbol multiply coherently whatever the residual timing and the symbol's common phase:
//     Y_{j,q,s}[k] = sum_{n < K} c[lo + r^ + (q + s) N + j T + CP + n] exp(-2 pi i (k + eps^) n / K)       (n ascending)
//     D_j(q) = sum_{pilot symbols s, ascending} | sum_{i ascending} Y_{j,q,s}[k_i] conj(Y_{j,q,s}[k_{i+1}]) |
//     D(q) = sum_{j < J, ascending} D_j(q)       q^ = the smallest q with the largest D(q)       first = lo + r^ + q^ N
// The twiddle's phase is taken in turns: (k n mod K) is an exact integer, ((k n mod K) + eps^ n) / K carries three roundings,
// turns - rint(turns) is exact and sincospif reduces no further.
//
// Three launches, no host synchronisation, no atomics, every sum in the order stated above (two runs give the same bits):
//   1. acq_symbol_sums_kernel: one thread per m, P[m] and E[m] into the workspace;
//   2. acq_phase_kernel: one block per (q, j).  Every block redoes stage A's last step from P, E (N CP additions: cheaper than
//      a launch of its own) so that it knows r^ and eps^, then computes D_j(q) into the workspace; block (0, 0) also writes
//      sym_metric, cfo_out and r^;
//   3. acq_decide_kernel: D(q), phase_metric, q^ and first_out.
// Every read lies in [lo, lo + (J + 1) T): stage A reaches lo + J T + N - 2, stage B lo + (J + 1) T - 2 (r^ <= N - 1,
// q + s <= 2 S - 2).  pilot_sc is device data the host cannot look at: entries outside [0, S K) are ignored, a carrier is always
// taken mod K, and a symbol's run is (first entry, count) within the array, so whatever the array holds nothing is read outside
// it or outside the symbol's K samples.
//
// dccn_capture_acquire_grouped runs the same three launches for up to kMaxChains links at once: each kernel's code is a body over
// one link's AcqArgs, and the grouped kernels (at the end) hand it the entry of a by-value link table.
#pragma once
#include <math.h>

#include "capture_source.h"
#include "common.h"

namespace dccn {

constexpr int kAcqThreads = 256;        // a block of acq_phase_kernel: one thread per pilot carrier of a symbol
constexpr int kAcqSumThreads = 64;      // a block of acq_symbol_sums_kernel
constexpr int kAcqMaxN = 1024;          // K + CP: a block's LDS holds P, E of N + CP - 1 lags and one symbol's K samples (< 48 KB)
constexpr int kAcqMaxPilot = kAcqThreads;
constexpr int kAcqMaxS = 64;            // acq_decide_kernel: one thread per q, one wave
constexpr int kAcqMaxJ = 256;

static inline bool capture_acquire_shape_ok(int S, int K, int CP, int n_pilot, int J) {
    if (S < 1 || S > kAcqMaxS || K < 2 || CP < 1 || CP > K || K + CP > kAcqMaxN) return false;
    return n_pilot >= 2 && n_pilot <= kAcqMaxPilot && J >= 1 && J <= kAcqMaxJ;
}

// The workspace: (P.re, P.im, E, -) of the N + CP - 1 lags; D_j(q) [S, J]; r^.
struct AcqWorkspace {
    size_t pe, partial, rhat, total;
};
static inline AcqWorkspace capture_acquire_layout(int S, int K, int CP, int J) {
    AcqWorkspace w;
    w.pe = 0;
    w.partial = align_up((size_t)(K + 2 * CP - 1) * 16, 256);
    w.rhat = w.partial + align_up((size_t)S * J * 4, 256);
    w.total = w.rhat + 256;
    return w;
}

struct AcqArgs {
    const float* cap;           // [n_samples, 2]
    long long lo;
    const int* pilot_sc;        // [n_pilot]
    float4* pe;                 // workspace
    float* partial;             // workspace [S, J]
    int* rhat;                  // workspace [1]
    long long* first_out;       // [1]
    float* cfo_out;             // [1]
    float* sym_metric;          // nullable [N]
    float* phase_metric;        // nullable [S]
    int S, K, CP, J, n_pilot;
};

// LDS of a block of acq_phase_kernel
__host__ __device__ static inline size_t capture_acquire_lds(int S, int K, int CP, int n_pilot) {
    return (size_t)(K + 2 * CP - 1) * 16 + (size_t)K * 8 + (size_t)n_pilot * 8 + (size_t)n_pilot * 4 + (size_t)S * 8 +
           (size_t)kAcqThreads * 16 + 16;
}

// The three launches, each stated once as a body over one link's AcqArgs: the solo kernels pass their own argument, the grouped
// ones (at the end) the entry of their link table.  A body reads blockIdx.x (and .y, acq_phase_body) as the solo grid lays them
// out; the link index rides on a dimension the body does not look at.  The two bodies that read the capture take it from a capture
// source (capture_source.h: float32, or 16-bit integer I/Q with its scale), one sample per load.
template <class Src>
__device__ __forceinline__ void acq_symbol_sums_body(const AcqArgs& a, const Src src) {
    const int N = a.K + a.CP;
    const int m = blockIdx.x * kAcqSumThreads + threadIdx.x;
    if (m >= N + a.CP - 1) return;
    const auto c = src.of(a) + a.lo + m;
    float pr = 0.f, pi = 0.f, e = 0.f;
#pragma unroll 8                                                           // (loads of eight symbols in flight; the order of the sums stays)
    for (int u = 0; u < a.J * a.S; ++u) {
        const float2 x = c[(size_t)u * N], v = c[(size_t)u * N + a.K];
        pr += x.x * v.x + x.y * v.y;
        pi += x.y * v.x - x.x * v.y;
        e += 0.5f * ((x.x * x.x + x.y * x.y) + (v.x * v.x + v.y * v.y));
    }
    a.pe[m] = make_float4(pr, pi, e, 0.f);
}
static __global__ void __launch_bounds__(kAcqSumThreads) acq_symbol_sums_kernel(const AcqArgs a) {
    acq_symbol_sums_body(a, CapOfArgs{});
}

template <class Src>
__device__ __forceinline__ void acq_phase_body(const AcqArgs& a, const Src src) {
    extern __shared__ float4 acq_lds[];
    const int S = a.S, K = a.K, CP = a.CP, N = K + CP, J = a.J, n_pilot = a.n_pilot;
    const int tid = threadIdx.x;
    const int q = blockIdx.x, j = blockIdx.y;
    const bool writer = q == 0 && j == 0;
    float4* const pe = acq_lds;                                          // [N + CP - 1]
    float4* const red = pe + (N + CP - 1);                               // [kAcqThreads]: (Lambda, r, Gamma.re, Gamma.im)
    float2* const y = reinterpret_cast<float2*>(red + kAcqThreads);      // [K]
    float2* const Y = y + K;                                             // [n_pilot]
    int* const car = reinterpret_cast<int*>(Y + n_pilot);                // [n_pilot]
    int* const run_at = car + n_pilot;                                   // [S]: a symbol's first entry of pilot_sc
    int* const run_n = run_at + S;                                       // [S]: and how many it has

    for (int m = tid; m < N + CP - 1; m += kAcqThreads) pe[m] = a.pe[m];
    for (int i = tid; i < n_pilot; i += kAcqThreads) car[i] = a.pilot_sc[i];
    __syncthreads();
    int at = 0, cells = 0;                                               // thread s < S: symbol s's run of pilot cells
    if (tid < S)
        for (int i = 0; i < n_pilot; ++i) {
            const int sc = car[i];
            if (sc >= tid * K && sc < (tid + 1) * K) {
                if (cells == 0) at = i;
                ++cells;
            }
        }
    __syncthreads();
    if (tid < S) {
        run_at[tid] = at;
        run_n[tid] = cells;
    }
    for (int i = tid; i < n_pilot; i += kAcqThreads) {
        const int sc = car[i];
        car[i] = sc >= 0 ? sc % K : 0;
    }
    __syncthreads();

    // stage A's last step: a thread's lags in ascending order, then the block's maximum, the smallest lag on ties
    float lam = -INFINITY, bgr = 0.f, bgi = 0.f;
    int best = tid;
    for (int r = tid; r < N; r += kAcqThreads) {
        float gr = 0.f, gi = 0.f, phi = 0.f;
        for (int n = 0; n < CP; ++n) {
            const float4 t = pe[r + n];
            gr += t.x;
            gi += t.y;
            phi += t.z;
        }
        const float l = sqrtf(gr * gr + gi * gi) - phi;
        if (writer && a.sym_metric) a.sym_metric[r] = l;
        if (l > lam) {
            lam = l;
            best = r;
            bgr = gr;
            bgi = gi;
        }
    }
    red[tid] = make_float4(lam, __int_as_float(best), bgr, bgi);
    __syncthreads();
    for (int d = kAcqThreads / 2; d > 0; d >>= 1) {
        if (tid < d) {
            const float4 mine = red[tid], other = red[tid + d];
            const int mb = __float_as_int(mine.y), ob = __float_as_int(other.y);
            if (other.x > mine.x || (other.x == mine.x && ob < mb)) red[tid] = other;
        }
        __syncthreads();
    }
    const float4 top = red[0];
    int rhat = __float_as_int(top.y);
    rhat = rhat < 0 ? 0 : (rhat > N - 1 ? N - 1 : rhat);                 // (NaN compares false everywhere: still a lag)
    const float eps = 0.f - atan2f(top.w, top.z) / 6.283185307179586f;
    if (writer && tid == 0) {
        a.cfo_out[0] = eps;
        a.rhat[0] = rhat;
    }

    // stage B: D_j(q), the pilot symbols in ascending order
    const float fK = (float)K;
    float dj = 0.f;
    for (int s = 0; s < S; ++s) {
        const int cnt = run_n[s];
        if (cnt < 2) continue;                                           // (uniform over the block)
        const auto sym = src.of(a) + a.lo + rhat + (long long)(q + s) * N + (long long)j * S * N + CP;
        __syncthreads();                                                 // (the previous symbol's y and Y are done with)
        for (int n = tid; n < K; n += kAcqThreads) y[n] = sym[n];
        __syncthreads();
        if (tid < cnt) {
            const int k = car[run_at[s] + tid];
            float yr = 0.f, yi = 0.f;
            int m = 0;                                                   // k n mod K
            for (int n = 0; n < K; ++n) {
                const float turns = ((float)m + eps * (float)n) / fK;
                float sn, cs;
                sincospif(2.0f * (turns - rintf(turns)), &sn, &cs);
                const float2 u = y[n];
                yr += u.x * cs + u.y * sn;
                yi += u.y * cs - u.x * sn;
                m += k;
                if (m >= K) m -= K;
            }
            Y[tid] = make_float2(yr, yi);
        }
        __syncthreads();
        if (tid == 0) {
            float cr = 0.f, ci = 0.f;
            for (int i = 0; i + 1 < cnt; ++i) {
                const float2 u = Y[i], v = Y[i + 1];
                cr += u.x * v.x + u.y * v.y;
                ci += u.y * v.x - u.x * v.y;
            }
            dj += sqrtf(cr * cr + ci * ci);
        }
    }
    if (tid == 0) a.partial[(size_t)q * J + j] = dj;
}
static __global__ void __launch_bounds__(kAcqThreads) acq_phase_kernel(const AcqArgs a) { acq_phase_body(a, CapOfArgs{}); }

__device__ __forceinline__ void acq_decide_body(const AcqArgs& a) {
    __shared__ float d[kAcqMaxS];
    const int q = threadIdx.x, S = a.S, J = a.J;
    if (q < S) {
        float acc = 0.f;
        for (int j = 0; j < J; ++j) acc += a.partial[(size_t)q * J + j];
        d[q] = acc;
        if (a.phase_metric) a.phase_metric[q] = acc;
    }
    __syncthreads();
    if (q == 0) {
        int qhat = 0;
        for (int i = 1; i < S; ++i)
            if (d[i] > d[qhat]) qhat = i;
        a.first_out[0] = a.lo + a.rhat[0] + (long long)qhat * (a.K + a.CP);
    }
}
static __global__ void __launch_bounds__(kAcqMaxS) acq_decide_kernel(const AcqArgs a) { acq_decide_body(a); }

// ---- carrier offsets beyond half a subcarrier spacing (dccn_capture_acquire_wide) ---------------------------------------------------
// Stage A gives eps^ modulo one spacing.  A whole number m of spacings moves the pilots from the bins k_i to k_i + m, so stage B
// is evaluated at shifted bins and decides the symbol position and the integer together:
//     D_j(q, m) = sum_{pilot symbols s, ascending} | sum_{i ascending} Y_{j,q,s}[(k_i + m) mod K] conj(Y_{j,q,s}[(k_{i+1} + m) mod K]) |
//     D(q, m) = sum_{j < J, ascending} D_j(q, m),  m in [-M, M]       (q^, m^) = the first maximum in row-major order of [S, 2 M + 1]
// Y is the narrow kernel's, term for term: column m = 0 is acq_phase_kernel's D_j(q), bit for bit, and M = 0 is the narrow call.
// Launches: acq_symbol_sums_kernel as it is; acq_phase_wide_kernel, one block per (q, j) -- per pilot symbol the bins that some
// (pilot, m) pair needs are marked, a thread owns one marked bin of the K (a bin that several pairs share is computed once, so at
// most K sums per symbol however wide the span), then one thread per m forms the modulus; acq_decide_wide_kernel, one block.
// The shift is circular in K (0 <= M <= K / 2 - 1, so the 2 M + 1 shifts of a carrier are distinct bins).
constexpr int kAcqWideThreads = 256;    // a block of acq_decide_wide_kernel
constexpr size_t kAcqWideLdsMax = 64 * 1024;

struct AcqWideArgs {
    AcqArgs a;                  // a.partial: workspace [S, 2 M + 1, J]; a.phase_metric: nullable [S, 2 M + 1]
    int32_t* cfo_int_out;       // [1]
    int M;
};

// LDS of a block of acq_phase_wide_kernel: the narrow block's with Y of all K bins, their marks and D_j(q, .) of the 2 M + 1 shifts
__host__ __device__ static inline size_t capture_acquire_wide_lds(int S, int K, int CP, int n_pilot, int M) {
    return (size_t)(K + 2 * CP - 1) * 16 + (size_t)kAcqThreads * 16 + (size_t)K * 8 + (size_t)K * 8 + (size_t)n_pilot * 4 +
           (size_t)S * 8 + (size_t)K * 4 + (size_t)(2 * M + 1) * 4 + 16;
}
static inline bool capture_acquire_wide_shape_ok(int S, int K, int CP, int n_pilot, int J, int M) {
    if (!capture_acquire_shape_ok(S, K, CP, n_pilot, J) || M < 0 || M > K / 2 - 1) return false;
    return capture_acquire_wide_lds(S, K, CP, n_pilot, M) <= kAcqWideLdsMax;
}
// The workspace: the narrow call's with D_j(q, m) [S, 2 M + 1, J] where it has D_j(q) (M = 0: the same bytes).
static inline AcqWorkspace capture_acquire_wide_layout(int S, int K, int CP, int J, int M) {
    AcqWorkspace w;
    w.pe = 0;
    w.partial = align_up((size_t)(K + 2 * CP - 1) * 16, 256);
    w.rhat = w.partial + align_up((size_t)S * (2 * M + 1) * J * 4, 256);
    w.total = w.rhat + 256;
    return w;
}

static __global__ void __launch_bounds__(kAcqThreads) acq_phase_wide_kernel(const AcqWideArgs w) {
    extern __shared__ float4 acq_lds[];
    const AcqArgs& a = w.a;
    const int S = a.S, K = a.K, CP = a.CP, N = K + CP, J = a.J, n_pilot = a.n_pilot, M = w.M, M2 = 2 * M + 1;
    const int tid = threadIdx.x;
    const int q = blockIdx.x, j = blockIdx.y;
    const bool writer = q == 0 && j == 0;
    float4* const pe = acq_lds;                                          // [N + CP - 1]
    float4* const red = pe + (N + CP - 1);                               // [kAcqThreads]: (Lambda, r, Gamma.re, Gamma.im)
    float2* const y = reinterpret_cast<float2*>(red + kAcqThreads);      // [K]
    float2* const Y = y + K;                                             // [K]: bin b of the symbol, where marked
    int* const car = reinterpret_cast<int*>(Y + K);                      // [n_pilot]
    int* const run_at = car + n_pilot;                                   // [S]: a symbol's first entry of pilot_sc
    int* const run_n = run_at + S;                                       // [S]: and how many it has
    int* const need = run_n + S;                                         // [K]: some (pilot, m) pair of this symbol reads bin b
    float* const dacc = reinterpret_cast<float*>(need + K);              // [2 M + 1]: D_j(q, m), each entry its own thread's

    for (int m = tid; m < N + CP - 1; m += kAcqThreads) pe[m] = a.pe[m];
    for (int i = tid; i < n_pilot; i += kAcqThreads) car[i] = a.pilot_sc[i];
    for (int mi = tid; mi < M2; mi += kAcqThreads) dacc[mi] = 0.f;
    __syncthreads();
    int at = 0, cells = 0;                                               // thread s < S: symbol s's run of pilot cells
    if (tid < S)
        for (int i = 0; i < n_pilot; ++i) {
            const int sc = car[i];
            if (sc >= tid * K && sc < (tid + 1) * K) {
                if (cells == 0) at = i;
                ++cells;
            }
        }
    __syncthreads();
    if (tid < S) {
        run_at[tid] = at;
        run_n[tid] = cells;
    }
    for (int i = tid; i < n_pilot; i += kAcqThreads) {
        const int sc = car[i];
        car[i] = sc >= 0 ? sc % K : 0;
    }
    __syncthreads();

    // stage A's last step, as acq_phase_body states it
    float lam = -INFINITY, bgr = 0.f, bgi = 0.f;
    int best = tid;
    for (int r = tid; r < N; r += kAcqThreads) {
        float gr = 0.f, gi = 0.f, phi = 0.f;
        for (int n = 0; n < CP; ++n) {
            const float4 t = pe[r + n];
            gr += t.x;
            gi += t.y;
            phi += t.z;
        }
        const float l = sqrtf(gr * gr + gi * gi) - phi;
        if (writer && a.sym_metric) a.sym_metric[r] = l;
        if (l > lam) {
            lam = l;
            best = r;
            bgr = gr;
            bgi = gi;
        }
    }
    red[tid] = make_float4(lam, __int_as_float(best), bgr, bgi);
    __syncthreads();
    for (int d = kAcqThreads / 2; d > 0; d >>= 1) {
        if (tid < d) {
            const float4 mine = red[tid], other = red[tid + d];
            const int mb = __float_as_int(mine.y), ob = __float_as_int(other.y);
            if (other.x > mine.x || (other.x == mine.x && ob < mb)) red[tid] = other;
        }
        __syncthreads();
    }
    const float4 top = red[0];
    int rhat = __float_as_int(top.y);
    rhat = rhat < 0 ? 0 : (rhat > N - 1 ? N - 1 : rhat);                 // (NaN compares false everywhere: still a lag)
    const float eps = 0.f - atan2f(top.w, top.z) / 6.283185307179586f;
    if (writer && tid == 0) {
        a.cfo_out[0] = eps;
        a.rhat[0] = rhat;
    }

    // stage B: D_j(q, m), the pilot symbols in ascending order
    const float fK = (float)K;
    for (int s = 0; s < S; ++s) {
        const int cnt = run_n[s];
        if (cnt < 2) continue;                                           // (uniform over the block)
        const float2* src = reinterpret_cast<const float2*>(a.cap) + a.lo + rhat + (long long)(q + s) * N +
                            (long long)j * S * N + CP;
        const int* const ks = car + run_at[s];
        __syncthreads();                                                 // (the previous symbol's y, Y and marks are done with)
        for (int n = tid; n < K; n += kAcqThreads) {
            y[n] = src[n];
            need[n] = 0;
        }
        __syncthreads();
        for (int t = tid; t < cnt * M2; t += kAcqThreads) need[(ks[t / M2] + t % M2 - M + K) % K] = 1;   // (every writer stores 1)
        __syncthreads();
        for (int k = tid; k < K; k += kAcqThreads) {
            if (!need[k]) continue;
            float yr = 0.f, yi = 0.f;
            int m = 0;                                                   // k n mod K
            for (int n = 0; n < K; ++n) {
                const float turns = ((float)m + eps * (float)n) / fK;
                float sn, cs;
                sincospif(2.0f * (turns - rintf(turns)), &sn, &cs);
                const float2 u = y[n];
                yr += u.x * cs + u.y * sn;
                yi += u.y * cs - u.x * sn;
                m += k;
                if (m >= K) m -= K;
            }
            Y[k] = make_float2(yr, yi);
        }
        __syncthreads();
        for (int mi = tid; mi < M2; mi += kAcqThreads) {
            float cr = 0.f, ci = 0.f;
            for (int i = 0; i + 1 < cnt; ++i) {
                const float2 u = Y[(ks[i] + mi - M + K) % K], v = Y[(ks[i + 1] + mi - M + K) % K];
                cr += u.x * v.x + u.y * v.y;
                ci += u.y * v.x - u.x * v.y;
            }
            dacc[mi] += sqrtf(cr * cr + ci * ci);
        }
    }
    for (int mi = tid; mi < M2; mi += kAcqThreads) a.partial[((size_t)q * M2 + mi) * J + j] = dacc[mi];
}

// D(q, m), phase_metric, the first maximum in row-major order, first_out and cfo_int_out.  A thread walks its entries e = tid,
// tid + 256, ... in ascending order and keeps the first of its largest; the block then keeps the largest, the smallest e on ties.
static __global__ void __launch_bounds__(kAcqWideThreads) acq_decide_wide_kernel(const AcqWideArgs w) {
    __shared__ float bv[kAcqWideThreads];
    __shared__ int be[kAcqWideThreads];
    const AcqArgs& a = w.a;
    const int tid = threadIdx.x, J = a.J, M2 = 2 * w.M + 1, total = a.S * M2;
    float top = -INFINITY;
    int at = tid < total ? tid : 0;
    for (int e = tid; e < total; e += kAcqWideThreads) {
        float acc = 0.f;
        for (int j = 0; j < J; ++j) acc += a.partial[(size_t)e * J + j];
        if (a.phase_metric) a.phase_metric[e] = acc;
        if (acc > top) {
            top = acc;
            at = e;
        }
    }
    bv[tid] = top;
    be[tid] = at;
    __syncthreads();
    for (int d = kAcqWideThreads / 2; d > 0; d >>= 1) {
        if (tid < d && (bv[tid + d] > bv[tid] || (bv[tid + d] == bv[tid] && be[tid + d] < be[tid]))) {
            bv[tid] = bv[tid + d];
            be[tid] = be[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) {
        int e = be[0];
        e = e < 0 ? 0 : (e > total - 1 ? total - 1 : e);                  // (NaN compares false everywhere: still an entry)
        a.first_out[0] = a.lo + a.rhat[0] + (long long)(e / M2) * (a.K + a.CP);
        w.cfo_int_out[0] = e % M2 - w.M;
    }
}

// ---- several links per launch (dccn_capture_acquire_grouped) --------------------------------------------------------------------
// Each link has its own capture, origin, pilot cells, outputs and workspace; the shape, J and n_pilot are the call's.  The table
// travels by value in the kernel arguments and is indexed by a block-uniform value (scalar loads, as ChainOffs is read); the link
// index is grid dimension y of the symbol sums, z of the phase launch (whose grid is (q, j)) and x of the decision.
struct AcqLink {
    const float* cap;
    long long lo;
    const int* pilot_sc;
    float4* pe;
    float* partial;
    int* rhat;
    long long* first_out;
    float* cfo_out;
    float* sym_metric;
    float* phase_metric;
};
struct AcqGroupArgs {
    AcqLink link[kMaxChains];
    int S, K, CP, J, n_pilot;
    __device__ __forceinline__ AcqArgs of(const unsigned g) const {
        const AcqLink& l = link[g];
        return AcqArgs{l.cap, l.lo, l.pilot_sc, l.pe, l.partial, l.rhat, l.first_out, l.cfo_out, l.sym_metric, l.phase_metric,
                       S, K, CP, J, n_pilot};
    }
};
static __global__ void __launch_bounds__(kAcqSumThreads) acq_symbol_sums_grouped_kernel(const AcqGroupArgs g) {
    acq_symbol_sums_body(g.of(blockIdx.y), CapOfArgs{});
}
static __global__ void __launch_bounds__(kAcqThreads) acq_phase_grouped_kernel(const AcqGroupArgs g) {
    acq_phase_body(g.of(blockIdx.z), CapOfArgs{});
}
static __global__ void __launch_bounds__(kAcqMaxS) acq_decide_grouped_kernel(const AcqGroupArgs g) { acq_decide_body(g.of(blockIdx.x)); }

// ---- 16-bit integer I/Q captures (dccn_capture_acquire_sc16) ----------------------------------------------------------------------
// The two launches that read the capture, over CapSc16 (a.cap is not read); the decision is acq_decide_kernel itself.
struct AcqSc16Args {
    AcqArgs a;
    CapSc16 src;
};
static __global__ void __launch_bounds__(kAcqSumThreads) acq_symbol_sums_sc16_kernel(const AcqSc16Args g) {
    acq_symbol_sums_body(g.a, g.src);
}
static __global__ void __launch_bounds__(kAcqThreads) acq_phase_sc16_kernel(const AcqSc16Args g) { acq_phase_body(g.a, g.src); }

}  // namespace dccn

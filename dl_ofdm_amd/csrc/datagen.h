// Device-side input generator: what the reference produces per batch on the host with
// NumPy -- label bits (dev/py/util.py:25-29), the OFDM transmitter (dev/py/ofdm.py:328-380), a static
// multipath Rayleigh channel (dev/py/radio.py:277-372, 409-470) and AWGN (radio.py:513-526) -- written
// straight into the receiver engine's resident input buffers.  Random streams are Philox4x32-10
// (counter = (index lo, index hi, stream, batch offset), key = seed), so a batch is a pure function of
// (seed, offset) and every thread draws independently.  All of it is one pass over HBM; the IFFT + cyclic
// prefix is a dense MFMA GEMM with a constant [2K, 2(K+CP)] matrix (gemm_f32_mfma.h).
#pragma once
#include <hip/hip_fp16.h>
#include "common.h"
#include "gemm_f32_mfma.h"
#include "norm_adam.h"
#include "frame_sync.h"

namespace dccn {

constexpr unsigned kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr int kStreamBits = 0, kStreamTaps = 1, kStreamNoise = 2, kStreamDoppler = 3;
constexpr int kSinusoids = 48;            // Jakes sum-of-sinusoids terms (radio.py:376-407)

struct Philox4 {
    unsigned v[4];
};
__device__ __forceinline__ Philox4 philox4x32_10(unsigned long long index, unsigned stream, unsigned offset,
                                                 unsigned long long seed) {
    unsigned c0 = (unsigned)index, c1 = (unsigned)(index >> 32), c2 = stream, c3 = offset;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
        const unsigned hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    Philox4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}
__device__ __forceinline__ float uniform01(unsigned w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-8f; }
__device__ __forceinline__ float2 box_muller(unsigned w0, unsigned w1) {
    const float r = sqrtf(-2.0f * logf(uniform01(w0)));
    float sn, cs;
    sincosf(6.2831853071795864769f * uniform01(w1), &sn, &cs);
    return make_float2(r * cs, r * sn);
}
// two independent standard normals of counter (index, stream, offset)
__device__ __forceinline__ float2 normal_pair(unsigned long long index, unsigned stream, unsigned offset, unsigned long long seed) {
    const Philox4 p = philox4x32_10(index, stream, offset, seed);
    return box_muller(p.v[0], p.v[1]);
}

// ---- the channel's arithmetic, each piece once: the per-stage kernels, the fused generator body and (through norm_adam.h) R0's
// virtual input call these, which is what makes their outputs the same bits ----
// acc += a * b (complex); -ffp-contract=off: two roundings per product and sum, the terms of each component in this order
__device__ __forceinline__ void cmac(float2& acc, const float2 a, const float2 b) {
    acc.x += a.x * b.x - a.y * b.y;
    acc.y += a.x * b.y + a.y * b.x;
}
// radio.py:352-372 static tap k of frame fr: (z0 + i z1) / sqrt(2) * coeff_k, z from Philox stream 1 at index fr * tap_stride + k
__device__ __forceinline__ float2 scaled_tap(const float2 z, const float coeff_k) {
    const float c = coeff_k * 0.70710678118654752440f;
    return make_float2(z.x * c, z.y * c);
}
__device__ __forceinline__ float2 static_tap(const int fr, const int k, const int tap_stride, const float* __restrict__ coeff,
                                             unsigned offset, unsigned long long seed) {
    return scaled_tap(normal_pair((unsigned long long)fr * tap_stride + k, kStreamTaps, offset, seed), coeff[k]);
}
// impulse response g[l] = sum_k tap[k] alpha[k, l] (alpha: [n_taps, L] sinc interpolation), k ascending
__device__ __forceinline__ float2 taps_dot_alpha(const float2* tap, const float* __restrict__ alpha, const int n_taps, const int L,
                                                 const int l) {
    float2 a = make_float2(0.f, 0.f);
    for (int k = 0; k < n_taps; ++k) {
        const float w = alpha[k * L + l];
        a.x += tap[k].x * w;
        a.y += tap[k].y * w;
    }
    return a;
}
// frequency response H[f] = sum_l g[l] w^((f l) mod nfft), l ascending; twiddle(m) = w^m = (cos, sin)(-2 pi m / nfft), computed
// (twiddle_of) or read from a table of those values
__device__ __forceinline__ float2 twiddle_of(const int m, const int nfft) {
    float sn, cs;
    sincosf(-6.2831853071795864769f * (float)m / (float)nfft, &sn, &cs);
    return make_float2(cs, sn);
}
template <typename TW>
__device__ __forceinline__ float2 freq_response(const float2* g, const int L, const int f, const int nfft, TW twiddle) {
    float2 a = make_float2(0.f, 0.f);
    for (int l = 0; l < L; ++l) {
        const float2 w = twiddle((f * l) % nfft);
        cmac(a, g[l], w);
    }
    return a;
}
// radio.py:513-526 noise level of a frame: sqrt(.5) 10^(-SNR/20)
__device__ __forceinline__ float frame_noise_std(const float snr_db) { return 0.70710678118654752440f * exp10f(-snr_db * 0.05f); }
// radio.py:376-407 Jakes sum of sinusoids: tap k of symbol time t is coeff_k sqrt(1/48) (mu_0 + i mu_1),
// mu_c = sum_n cos(2 pi t Fd cos(a_n +- a0_k) + theta[c][n][k]) (c = 0: +, c = 1: -), a_n = (n + .5) pi / (4 * 48), a0_k = (k + 1) pi / (4 * 48),
// theta uniform in [0, 2 pi) from Philox stream 3 at index ((fr 2 + c) 48 + n) tap_stride + k
constexpr float kJakesNorm = 0.14433756729740644113f;          // sqrt(1/48)
__device__ __forceinline__ float doppler_phase(const int fr, const int c, const int n, const int k, const int tap_stride, unsigned offset,
                                               unsigned long long seed) {
    const unsigned long long i = (((unsigned long long)fr * 2 + c) * kSinusoids + n) * tap_stride + k;
    return 6.2831853071795864769f * uniform01(philox4x32_10(i, kStreamDoppler, offset, seed).v[0]);
}
__device__ __forceinline__ float jakes_shift(const float Fd, const int c, const int n, const int k) {
    const float step = 3.14159265358979323846f / (4.0f * kSinusoids);
    const float an = ((float)(n + 1) - 0.5f) * step, a0 = (float)(k + 1) * step;
    return Fd * cosf(c == 0 ? an + a0 : an - a0);
}
__device__ __forceinline__ float jakes_cos(const float t, const float shift, const float theta) {
    return cosf(6.2831853071795864769f * t * shift + theta);
}

// test hook: out[i] = the four words of counter (i, stream, offset)
static __global__ __launch_bounds__(256) void philox_fill_kernel(unsigned* __restrict__ out, long long n, unsigned stream,
                                                          unsigned offset, unsigned long long seed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Philox4 p = philox4x32_10((unsigned long long)i, stream, offset, seed);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[i * 4 + j] = p.v[j];
}

// util.py:25-29 bit_source + ofdm.py:339-356 constellation / pilot / guard mapping: one thread per resource
// cell.  cell_map[S*K]: >= 0 data-cell index d, -1 pilot, -2 empty.  bits_in == nullptr: draw the label bits
// (bit j of cell (frame,d) = bit j of Philox word 0 at index frame*D+d) and store them to bits_out;
// the constellation index is MSB-first over the nbits labels (ofdm.py:121-153 const_map order).
static __global__ __launch_bounds__(256) void tx_grid_kernel(const int* __restrict__ bits_in, int* __restrict__ bits_out,
                                                      const int* __restrict__ cell_map,
                                                      const float2* __restrict__ const_tab, float2 pilot,
                                                      float2* __restrict__ grid, long long n_cells, int SK, int D,
                                                      int nbits, unsigned offset, unsigned long long seed) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cells) return;
    const long long frame = i / SK;
    const int d = cell_map[(int)(i - frame * SK)];
    float2 v = make_float2(0.f, 0.f);
    if (d == -1) {
        v = pilot;
    } else if (d >= 0) {
        const long long cell = frame * D + d;
        unsigned word = 0;
        if (!bits_in) word = philox4x32_10((unsigned long long)cell, kStreamBits, offset, seed).v[0];
        int idx = 0;
        for (int j = 0; j < nbits; ++j) {
            const int b = bits_in ? (bits_in[cell * nbits + j] & 1) : (int)((word >> j) & 1u);
            if (bits_out) bits_out[cell * nbits + j] = b;
            idx = (idx << 1) | b;
        }
        v = const_tab[idx];
    }
    grid[i] = v;
}

// radio.py:352-372 static taps: tap_k = (z0 + i z1)/sqrt(2) * coeff_k, impulse response g = taps . alpha
// ([n_taps, L] sinc-interpolation matrix), H = fft(g, nfft).  One block (64 threads) per frame.
// taps_in (standard normals [n, n_taps, 2]) == nullptr: draw them.  identity != 0: g = [1] (AWGN channel).
// frames (nullable): the frame indices this launch covers (frame-interleaved 'mix' channels run one launch per
// profile); tap_stride: taps per frame in taps_in and in the Philox index; g_stride: float2 per frame in g;
// h_rep: copies of H per frame (the mix channels report H per symbol for static frames too).
static __global__ __launch_bounds__(64) void channel_taps_kernel(const float* __restrict__ taps_in,
                                                          const float* __restrict__ coeff,
                                                          const float* __restrict__ alpha, float2* __restrict__ g,
                                                          float2* __restrict__ H, int n_taps, int L, int nfft,
                                                          int identity, unsigned offset, unsigned long long seed,
                                                          const int* __restrict__ frames, int tap_stride, int g_stride,
                                                          int h_rep) {
    __shared__ float2 tap[16];
    __shared__ float2 gs[64];
    const int fr = frames ? frames[blockIdx.x] : (int)blockIdx.x, t = threadIdx.x;
    if (identity) {
        if (t < L) gs[t] = make_float2(t == 0 ? 1.f : 0.f, 0.f);
    } else {
        if (t < n_taps) {
            float2 z;                                        // (static_tap with the normals from the caller when given)
            if (taps_in) z = make_float2(taps_in[((size_t)fr * tap_stride + t) * 2], taps_in[((size_t)fr * tap_stride + t) * 2 + 1]);
            else z = normal_pair((unsigned long long)fr * tap_stride + t, kStreamTaps, offset, seed);
            tap[t] = scaled_tap(z, coeff[t]);
        }
        __syncthreads();
        if (t < L) gs[t] = taps_dot_alpha(tap, alpha, n_taps, L, t);
    }
    __syncthreads();
    if (t < L) g[(size_t)fr * g_stride + t] = gs[t];
    if (H) {
        for (int f = t; f < nfft; f += 64) {
            const float2 a = freq_response(gs, L, f, nfft, [nfft](int m) { return twiddle_of(m, nfft); });
            for (int r = 0; r < h_rep; ++r) H[((size_t)fr * h_rep + r) * nfft + f] = a;
        }
    }
}

// radio.py:360-366: y = np.convolve(frame, g, 'same') over the frame's T = n_sym*n_sc samples
// (y[t] = sum_l g[l] x[t + off - l], off = (L-1)//2, zero outside the frame) + per-block partial sums of
// |y|^2 for the AWGN stage's power normalisation.  grid = (ceil(T/256), frames).
// Persistent form: the grid is a fixed number of blocks (<= kChanPartials) that each walk a run of consecutive
// (frame, 256-sample chunk) items and leave ONE partial sum of |y|^2 each, in a fixed order -- few enough for the AWGN kernel to add
// them up itself (the separate sum_partials launch of rounds 1-2 is gone).  pbase: this launch's first slot in `partial`.
constexpr int kChanPartials = 2048;
// TapGen (enabled): the block draws the static taps of a frame itself when it moves to that frame -- static_tap and
// taps_dot_alpha, as channel_taps_kernel, so the impulse response has the same bits; the taps launch disappears when nobody
// asked for H (the generate-and-train loop of the basic receiver).
struct TapGen {
    const float* coeff; const float* alpha;
    int enabled, n_taps, identity, tap_stride;
    unsigned offset; unsigned long long seed;
};
static __global__ __launch_bounds__(256) void fir_same_kernel(const float2* __restrict__ x, const float2* __restrict__ g,
                                                       float2* __restrict__ y, double* __restrict__ partial, int T,
                                                       int L, const int* __restrict__ frames, int g_stride, int n_frames,
                                                       int pbase, const TapGen tg, const int ipb) {
    __shared__ double sh[4];
    __shared__ float2 gs[64];
    __shared__ float2 tap[16];
    const int bx = (T + 255) / 256;
    const int off = (L - 1) / 2;
    double pw = 0.0;
    // a block takes a run of consecutive items: mostly chunks of one frame, whose taps are loaded once
    // (ipb = items per block, a whole number of frames when the grid allows: a frame's taps are then set up once)
    const int items = n_frames * bx;
    int cur = -1;
    for (int item = blockIdx.x * ipb; item < min(items, ((int)blockIdx.x + 1) * ipb); ++item) {
        const int fi = item / bx, cb = item - fi * bx;
        const int fr = frames ? frames[fi] : fi;
        if (fr != cur) {                                      // (block-uniform)
            __syncthreads();                                  // previous frame's taps are no longer read
            if (!tg.enabled) {
                if (threadIdx.x < L) gs[threadIdx.x] = g[(size_t)fr * g_stride + threadIdx.x];
            } else if (tg.identity) {
                if (threadIdx.x < L) gs[threadIdx.x] = make_float2(threadIdx.x == 0 ? 1.f : 0.f, 0.f);
            } else {
                const int t = threadIdx.x;
                if (t < tg.n_taps) tap[t] = static_tap(fr, t, tg.tap_stride, tg.coeff, tg.offset, tg.seed);
                __syncthreads();
                if (t < L) gs[t] = taps_dot_alpha(tap, tg.alpha, tg.n_taps, L, t);
            }
            __syncthreads();
            cur = fr;
        }
        const int t = cb * 256 + threadIdx.x;
        if (t < T) {
            const float2* xf = x + (size_t)fr * T;
            float2 a = make_float2(0.f, 0.f);
            for (int l = 0; l < L; ++l) {
                const int u = t + off - l;
                if (u < 0 || u >= T) continue;
                const float2 v = xf[u];
                cmac(a, gs[l], v);
            }
            y[(size_t)fr * T + t] = a;
            pw += (double)a.x * a.x + (double)a.y * a.y;
        }
    }
    pw = block_sum4(pw, sh);
    if (threadIdx.x == 0) partial[pbase + blockIdx.x] = pw;
}

// radio.py:513-526 AWGN_channel_np: out = y / sqrt(mean |y|^2 over the batch) + noise * sqrt(0.5) 10^(-SNR/20),
// SNR per frame; mean |y|^2 = sum of the FIR stage's block partials / total, added up by every block itself.
// noise_in (standard normals [n, T, 2]) == nullptr: draw them.  Also emits the per-block partial sums of the
// noise power (finished by sum_partials_kernel).  grid = (ceil(T/256), frames).
static __global__ __launch_bounds__(256) void awgn_kernel(const float2* __restrict__ y, const double* __restrict__ power_partial,
                                                   int n_partial, double total,
                                                   const float* __restrict__ snr_db,
                                                   const float* __restrict__ noise_in, float2* __restrict__ out,
                                                   double* __restrict__ noise_partial, int T, unsigned offset,
                                                   unsigned long long seed) {
    __shared__ double sh[4];
    __shared__ float s_inv;
    // mean |y|^2 over the batch from the FIR stage's <= kChanPartials block sums, added up by every block
    const float inv_scale = batch_power_inv_scale(power_partial, n_partial, total, sh, &s_inv);
    const int fr = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    double pw = 0.0;
    if (t < T) {
        const size_t i = (size_t)fr * T + t;
        const float std_ = frame_noise_std(snr_db[fr]);
        float2 z = noise_in ? make_float2(noise_in[2 * i], noise_in[2 * i + 1]) : normal_pair((unsigned long long)i, kStreamNoise, offset, seed);
        z.x *= std_;
        z.y *= std_;
        out[i] = scale_add_noise(y[i], inv_scale, z);
        pw = (double)z.x * z.x + (double)z.y * z.y;
    }
    if (noise_partial) {                                 // (kernel argument: block-uniform)
        __syncthreads();                                 // (sh held the batch power's wave sums)
        pw = block_sum4(pw, sh);
        if (threadIdx.x == 0) noise_partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = pw;
    }
}

// ---- round 5: the whole static-channel generator chain of a batch in ONE launch ----------------------------------------
// What tx_grid_kernel -> IDFT GEMM -> (channel_taps_kernel) -> fir_same_kernel -> awgn_kernel do in four or five launches
// (26-37 us of a 110 us generate-and-train step, each launch latency-bound on 1170 frames), per block of two frames:
//   1. label bits (util.py:25-29, Philox stream 0) -> constellation / pilot / guard cells (ofdm.py:339-356) into an LDS grid
//      of 2 S rows x 2K floats (rows past 2 S zero);
//   2. ifft + cyclic prefix (ofdm.py:357-362) as a 16 x 2K x 2(K+CP) product on v_mfma_f32_16x16x4_f32 with the constant
//      matrix of DeviceDataGen.idft_cp_matrix read straight from L2 into the MFMA registers (every load of a wave is issued
//      before its first MFMA), the time-domain frames land in LDS;
//   3. the frames' static taps (radio.py:352-372, Philox stream 1: static_tap, taps_dot_alpha, freq_response);
//   4. y = np.convolve(frame, g, 'same') (radio.py:360-366; cmac over l ascending, as fir_same_kernel) -> y, and ONE partial
//      sum of |y|^2 per block;
//   5. the frame-scaled noise of radio.py:513-526 (Philox stream 2: normal_pair's draw times frame_noise_std) -> noise, and one
//      partial sum of |noise|^2 per block.
// What cannot be finished here is the batch-wide 1 / sqrt(mean |y|^2): x = y * that + noise is formed by the consumer -- R0 of
// the receiver step reads (y, noise, partials) as its virtual input (norm_adam.h NormVirtual), or gen_static_apply_kernel
// materialises x where a buffer is wanted.
constexpr int kGenMaxProfiles = 6;
struct GenProfile {                 // one fading profile: tap amplitudes, sinc interpolation [n_taps, L]; identity: g = [1];
    const float* coeff; const float* alpha; int n_taps, L, identity; float Fd;      // Fd: its Doppler frequency (Doppler frames)
};
struct GenStaticArgs {
    int32_t* bits_out; const int* cell_map; const float2* const_tab; float2 pilot; const float* idft;
    // frame f runs profile f % n_prof (radio.py:438-452 without Doppler frames; n_prof = 1: one channel for the batch);
    // tap_stride: taps per frame in the Philox index of the tap draws (static_tap)
    GenProfile prof[kGenMaxProfiles]; int n_prof, tap_stride;
    float2* H; int h_rep;           // nullable: fft(g, K) per frame, h_rep copies (freq_response)
    // Doppler frames (radio.py:376-407, 438-452; the Doppler instantiation only): frame f is one when dop_period > 0,
    // f % dop_period == 0 and its profile has Fd > 0.1 and is not the identity; t_sym: seconds per OFDM symbol
    int dop_period;
    const float* snr_db;
    float2* y; float2* noise; double* power_partial; double* noise_partial; float* tx_out;
    int frames, S, K, CP, D, nbits;
    unsigned offset; unsigned long long seed;
    int abl;            // timing ablations (DCCN_GEN_ABL, experiments only: results are wrong when set): 1 no noise draws, 2 no
                        // label draws, 4 no ifft matrix loads, 8 no FIR
    float t_sym;        // (dop_period and t_sym sit where the struct had padding: the static launch's argument block is unchanged)
    __device__ __forceinline__ GenStaticArgs at_chain(const long long coff) const {     // chain groups (common.h)
        GenStaticArgs q = *this;
        q.bits_out = chain_at(bits_out, coff); q.cell_map = chain_at(cell_map, coff); q.const_tab = chain_at(const_tab, coff);
        q.idft = chain_at(idft, coff);
        // (prof[] is NOT rebased here: the kernel reads the two profiles a workgroup needs from the kernel-argument segment by
        // index and rebases those -- an indexed COPY of the table lives in scratch memory, and the compiler turns a compare chain
        // over literal indices back into an index)
        q.H = chain_at(H, coff); q.snr_db = chain_at(snr_db, coff); q.y = chain_at(y, coff); q.noise = chain_at(noise, coff);
        q.power_partial = chain_at(power_partial, coff); q.noise_partial = chain_at(noise_partial, coff); q.tx_out = chain_at(tx_out, coff);
        return q;
    }
};
// what differs between the chains of a group besides their arenas: the modulation and the Philox stream (n == 0: one chain,
// the values of GenStaticArgs stand)
struct GenChainScalars {
    int n;
    int nbits[kMaxChains];
    unsigned offset[kMaxChains];
    unsigned long long seed[kMaxChains];
};
typedef float gen_f32x4 __attribute__((ext_vector_type(4)));
constexpr int kGenFramesPerBlock = 2;
constexpr int kGenFirPad = 64;             // >= the longest channel response the launch accepts (L <= 64)
// S, K, CP are compile-time (the N = 64 grid of the reference: 7 symbols, 64 + 16 samples, or 64 + 4 at the short prefix): every
// index split is a division by a constant, and the per-thread loops over a block's 1024 grid cells and 1120 (952) samples are
// unrolled -- a thread's cells / samples
// are INDEPENDENT chains (Philox -> Box-Muller -> store; cell map -> Philox -> constellation table) whose latencies then
// overlap instead of adding up (the first version walked them one after the other with run-time divisions: 26.8 us per launch;
// profiles/r05_e2e_kernel_stats.txt has this one)
// The body is a device function so that the generator's workgroups can also RIDE on another launch (round 6: behind the
// equaliser step's bottleneck backward launch, eq_bottleneck.h): a = the launch's argument block as gen_args_of_chain
// prepared it for this chain, block = this workgroup's index among the generator's; the body uses gen_static_smem_bytes() of
// dynamic LDS.
// The launch's argument block for one chain (arena offset applied, per-chain scalars taken), written out where the KERNEL
// PARAMETERS are in scope: handing them to a helper by reference takes their address, which turns the by-value kernel
// arguments into a private copy -- and the per-chain index into a scratch access.
#define DCCN_GEN_ARGS_OF_CHAIN(a, P0, P1, a0, gc, coff, chain, block)                                         \
    GenStaticArgs a = (a0).at_chain(coff);                                                                     \
    if ((gc).n > 0) { a.nbits = (gc).nbits[chain]; a.offset = (gc).offset[chain]; a.seed = (gc).seed[chain]; } \
    /* the profiles of the block's two frames (block-uniform; frame 1 of a one-frame block repeats frame 0) */  \
    GenProfile P0 = (a0).prof[((block) * kGenFramesPerBlock) % (a0).n_prof];                                    \
    GenProfile P1 = (a0).prof[((block) * kGenFramesPerBlock + (((a0).frames - (block) * kGenFramesPerBlock) > 1 ? 1 : 0)) % (a0).n_prof]; \
    P0.coeff = chain_at(P0.coeff, coff); P0.alpha = chain_at(P0.alpha, coff);                                   \
    P1.coeff = chain_at(P1.coeff, coff); P1.alpha = chain_at(P1.alpha, coff);
// DOPPLER (its own instantiation; static descriptors keep launching the DOPPLER = false code): a frame of the block can be a
// Doppler frame (GenStaticArgs::dop_period; block-uniform per frame, as its profile is).  Such a frame takes, in the arithmetic
// of doppler_taps_kernel / fir_doppler_kernel: its 2 x 48 x n_taps uniform phases (Philox stream 3, drawn once per frame, spread
// over the block, into LDS next to Fd cos(a_n +- a0_k), which depends on (n, k) only); per symbol and tap the two 48-term cosine
// sums (same order over n); g[s] = taps[s] . alpha (same order over k); H[s] = fft(g[s], K) from the twiddle table; and the
// per-symbol 'same' FIR with n_taps samples of history on the time-domain frame in LDS.  Labels, ifft, noise, the partial sums
// and the static frames of the same block are the code of the static instantiation.
template <int S, int K, int CP, bool DOPPLER = false>
__device__ __forceinline__ void gen_static_frames_body(const GenStaticArgs a, const GenProfile P0, const GenProfile P1, const int block) {
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    constexpr int K2 = 2 * K, N2 = 2 * (K + CP), T = S * (K + CP), LDG = K2 + 4;
    // the cyclic-prefix columns of the ifft matrix are bitwise copies of its last 2 CP columns (t = (t' - CP) mod K,
    // datagen.py idft_cp_matrix): only the K2 / 16 tiles behind the prefix are multiplied, the prefix is stored twice.
    // TILED (CP = 16): the prefix is CPT whole tiles of a 16-aligned grid over the N2 columns, the multiplied tiles are
    // CPT..NTILE-1 and the last CPT of them are stored twice.  Otherwise (CP = 4: 8 prefix columns, N2 = 136) the same K2 / 16
    // tiles are anchored at column 2 CP -- body tile t covers columns 2 CP + 16 t .. -- and a column whose index behind the
    // prefix is >= K2 - 2 CP goes to the prefix too: a per-lane condition inside the last tile.  (Two forms of one index
    // computation under `if constexpr`: the tiled instantiations keep the code objects they had.)
    constexpr bool TILED = (2 * CP) % 16 == 0;
    constexpr int G16 = K2 / 16, CP2 = 2 * CP, NTILE = N2 / 16, CPT = CP2 / 16, NMUL = TILED ? NTILE - CPT : G16, TPW = (NMUL + 3) / 4;
    static_assert(TILED ? (N2 % 16 == 0 && CPT <= NMUL) : (CP2 < 16 && NMUL % 4 == 0),
                  "cyclic prefix: whole 16-column tiles, or less than one tile with every wave multiplying TPW whole tiles");
    constexpr int NSMP = (kGenFramesPerBlock * T + 255) / 256;          // samples per thread (CP = 16: 5, CP = 4: 4)
    constexpr int NCELL = 16 * K / 256;                                  // grid cells per thread (4)
    static_assert(kGenFramesPerBlock * S <= 16 && K2 % 16 == 0 && (16 * K) % 256 == 0, "generator tile shape");
    // the time-domain frames sit between two runs of kGenFirPad zeros: the 'same' FIR then reads its out-of-range neighbours
    // as zeros instead of branching around them (adding +-0 leaves every partial sum as it was: same bits as the skipped form)
    constexpr int TP = T + 2 * kGenFirPad;
    float* sG = gsm;                                   // [16][LDG]   grid rows (frame, symbol), (k, iq) contiguous
    float2* sTX = reinterpret_cast<float2*>(gsm + 16 * LDG);      // [2][pad | T | pad]  time-domain frames
    __shared__ float2 gs[kGenFramesPerBlock][64];
    __shared__ float2 tap[kGenFramesPerBlock][16];
    __shared__ float2 tw[K];                           // (cos, sin) of -2 pi m / K: the frequency response's twiddles
    __shared__ double sh[2][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int f0 = block * kGenFramesPerBlock;
    const int nfr = min(kGenFramesPerBlock, a.frames - f0);
    const int L0 = P0.identity ? 1 : P0.L, L1 = P1.identity ? 1 : P1.L;
    // Doppler frames of the block (DeviceDataGen.frame_plan); dynamic LDS behind the time-domain frames:
    bool dop0 = false, dop1 = false;
    float2* sGd = nullptr;      // [2][S][64]      per-symbol impulse responses
    float2* sTapD = nullptr;    // [2][S][16]      per-symbol taps
    float* sTh = nullptr;       // [2][2][48][16]  phases theta[c][n][k]
    float* sFc = nullptr;       // [2][2][48][16]  Fd cos(a_n + a0_k) (c = 0), Fd cos(a_n - a0_k) (c = 1)
    if constexpr (DOPPLER) {
        if (a.dop_period > 0) {
            dop0 = (f0 % a.dop_period) == 0 && !P0.identity && P0.Fd > 0.1f;
            dop1 = nfr > 1 && ((f0 + 1) % a.dop_period) == 0 && !P1.identity && P1.Fd > 0.1f;
        }
        sGd = sTX + kGenFramesPerBlock * TP;
        sTapD = sGd + kGenFramesPerBlock * S * 64;
        sTh = reinterpret_cast<float*>(sTapD + kGenFramesPerBlock * S * 16);
        sFc = sTh + kGenFramesPerBlock * 2 * kSinusoids * 16;
    }
    if (a.H != nullptr && tid < K) tw[tid] = twiddle_of(tid, K);
    static_assert(kGenFramesPerBlock * 2 * kGenFirPad == 256, "one pad cell per thread");
    sTX[(tid >> 7) * TP + ((tid >> 6) & 1) * (kGenFirPad + T) + (tid & 63)] = make_float2(0.f, 0.f);

    // 2 (early). this wave's share of the ifft matrix: body tiles w, w + 4, ... ; lane (c, kq) needs
    // idft[16 g + 4 kq + j][2 CP + 16 tile + c] (per-lane scalar loads: the column origin needs no alignment)
    const int c = lane & 15, kq = lane >> 4;
    float bfr[TPW][G16][4];
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
        const float* B;
        if constexpr (TILED) {
            const int tile = min(CPT + w + 4 * ti, NTILE - 1);
            B = a.idft + (size_t)(4 * kq) * N2 + 16 * tile + c;
        } else {
            B = a.idft + (size_t)(4 * kq) * N2 + CP2 + 16 * (w + 4 * ti) + c;
        }
#pragma unroll
        for (int g = 0; g < G16; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[ti][g][j] = (a.abl & 4) ? 0.5f : B[(size_t)(16 * g + j) * N2];
    }
    // 1 (early). cell map entries of this thread's grid cells
    int cd[NCELL];
#pragma unroll
    for (int q = 0; q < NCELL; ++q) {
        const int i = tid + 256 * q, row = i / K, k = i - row * K, fr = row / S;
        cd[q] = fr < nfr ? a.cell_map[(row - fr * S) * K + k] : -2;
    }
    // 5. the frame-scaled noise (depends on nothing else: its Philox / Box-Muller chains run under the loads above)
    double nw = 0.0;
    {
        const float std0 = frame_noise_std(a.snr_db[f0]), std1 = frame_noise_std(a.snr_db[f0 + (nfr > 1 ? 1 : 0)]);
        float2 z[NSMP];
#pragma unroll
        for (int q = 0; q < NSMP; ++q) {
            const int i = tid + 256 * q, fr = i / T;
            const size_t o = (size_t)f0 * T + i;                         // (f0 + fr) * T + (i - fr * T)
            if (a.abl & 1) { z[q] = make_float2(0.3f, 0.1f); continue; }
            const Philox4 p = philox4x32_10((unsigned long long)o, kStreamNoise, a.offset, a.seed);
            z[q] = box_muller(p.v[0], p.v[1]);          // (normal_pair, written out: the call changes this kernel's schedule)
            const float sd = fr == 0 ? std0 : std1;
            z[q].x *= sd;
            z[q].y *= sd;
        }
#pragma unroll
        for (int q = 0; q < NSMP; ++q) {
            const int i = tid + 256 * q;
            if (i < nfr * T) {
                out_store2<5>(reinterpret_cast<float*>(a.noise + (size_t)f0 * T + i), z[q].x, z[q].y);
                nw += (double)z[q].x * z[q].x + (double)z[q].y * z[q].y;
            }
        }
    }
    // 3 (early). static taps of the block's frames (threads 0..n_taps-1 of waves 0 / 1 draw frame 0 / 1)
    const GenProfile Pw = w == 0 ? P0 : P1;            // (waves 0 / 1 own the taps of frames 0 / 1)
    const bool dopw = w == 0 ? dop0 : dop1;            // (false in the static instantiation)
    if (w < nfr && !Pw.identity && lane < Pw.n_taps && !dopw)
        tap[w][lane] = static_tap(f0 + w, lane, a.tap_stride, Pw.coeff, a.offset, a.seed);
    // 3d (early). phases of the block's Doppler frames and the Doppler shift of sinusoid (n, k): doppler_phase and jakes_shift,
    // written out (with either call this kernel's instruction stream changes)
    if constexpr (DOPPLER) {
        const float step = 3.14159265358979323846f / (4.0f * kSinusoids);
#pragma unroll
        for (int j = 0; j < kGenFramesPerBlock; ++j) {
            if (!(j == 0 ? dop0 : dop1)) continue;                      // (block-uniform)
            const int nt = j == 0 ? P0.n_taps : P1.n_taps;
            const float Fd = j == 0 ? P0.Fd : P1.Fd;
            for (int e = tid; e < 2 * kSinusoids * nt; e += 256) {
                const int cn = e / nt, k = e - cn * nt, cc = cn / kSinusoids, n = cn - cc * kSinusoids;
                const unsigned long long pi = ((unsigned long long)(f0 + j) * 2 * kSinusoids + cn) * a.tap_stride + k;
                const float th = 6.2831853071795864769f * uniform01(philox4x32_10(pi, kStreamDoppler, a.offset, a.seed).v[0]);
                const float an = ((float)(n + 1) - 0.5f) * step, a0 = (float)(k + 1) * step;
                const int o = (j * 2 * kSinusoids + cn) * 16 + k;
                sTh[o] = th;
                sFc[o] = Fd * cosf(cc == 0 ? an + a0 : an - a0);
            }
        }
    }
    // 1. resource grid: label bits (Philox word 0 of the cell), constellation / pilot / guard value
    {
        int idx[NCELL];
#pragma unroll
        for (int q = 0; q < NCELL; ++q) {
            const int i = tid + 256 * q, row = i / K, fr = row / S;
            idx[q] = 0;
            if (cd[q] >= 0) {
                const long long cell = (long long)(f0 + fr) * a.D + cd[q];
                const unsigned word = (a.abl & 2) ? (unsigned)cell : philox4x32_10((unsigned long long)cell, kStreamBits, a.offset, a.seed).v[0];
                for (int j = 0; j < a.nbits; ++j) {
                    const int bit = (int)((word >> j) & 1u);
                    out_store<5>(a.bits_out + cell * a.nbits + j, bit);
                    idx[q] = (idx[q] << 1) | bit;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NCELL; ++q) {
            const int i = tid + 256 * q, row = i / K, k = i - row * K;
            float2 v = make_float2(0.f, 0.f);
            if (cd[q] == -1) v = a.pilot;
            else if (cd[q] >= 0) v = a.const_tab[idx[q]];
            *reinterpret_cast<float2*>(sG + row * LDG + 2 * k) = v;
        }
    }
    __syncthreads();
    if (w < kGenFramesPerBlock) {                      // g = taps . alpha; zeros behind L: the FIR below runs both frames over
        float2 acc = make_float2(0.f, 0.f);            // the longer of the two responses
        const int Lw = w == 0 ? L0 : L1;
        if (w < nfr && lane < Lw && !dopw) {
            if (Pw.identity) acc = make_float2(lane == 0 ? 1.f : 0.f, 0.f);
            else {                                     // (taps_dot_alpha, written out: the call changes this kernel's exec-mask code)
                for (int k = 0; k < Pw.n_taps; ++k) {
                    const float wgt = Pw.alpha[k * Pw.L + lane];
                    acc.x += tap[w][k].x * wgt;
                    acc.y += tap[w][k].y * wgt;
                }
            }
        }
        gs[w][lane] = acc;
    }
    // 2. tx[row][n] = sum_k grid[row][k] idft[k][n]
    {
        gen_f32x4 acc[TPW];
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti) acc[ti] = gen_f32x4{0.f, 0.f, 0.f, 0.f};
        const float* Ar = sG + c * LDG + 4 * kq;
#pragma unroll
        for (int g = 0; g < G16; ++g) {
            const float4 av = *reinterpret_cast<const float4*>(Ar + 16 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ti = 0; ti < TPW; ++ti)
                    acc[ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4c(av, j), bfr[ti][g][j], acc[ti], 0, 0, 0);
        }
        // C layout: col = lane & 15, row = 4 (lane >> 4) + r
        float* txf = reinterpret_cast<float*>(sTX);
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti) {
            if constexpr (TILED) {
                const int tile = CPT + w + 4 * ti;
                if (tile < NTILE) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 4 * kq + r, fr = row / S;
                        if (fr < nfr) {
                            float* o = txf + fr * 2 * TP + 2 * kGenFirPad + (row - fr * S) * N2 + 16 * tile + c;
                            o[0] = acc[ti][r];
                            if (tile >= NTILE - CPT) o[-K2] = acc[ti][r];          // the prefix: columns 2K.. are columns 0..
                        }
                    }
                }
            } else {
                const int col = 16 * (w + 4 * ti) + c;                             // behind the prefix: 0 .. K2 - 1
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 4 * kq + r, fr = row / S;
                    if (fr < nfr) {
                        float* o = txf + fr * 2 * TP + 2 * kGenFirPad + (row - fr * S) * N2 + CP2 + col;
                        o[0] = acc[ti][r];
                        if (col >= K2 - CP2) o[-K2] = acc[ti][r];                  // the prefix, as above
                    }
                }
            }
        }
    }
    // 3d. Jakes taps of the Doppler frames: one (frame, re|im, symbol, tap) sum of 48 cosines per thread, n ascending
    if constexpr (DOPPLER) {
        const int nt0 = P0.n_taps, nt1 = P1.n_taps;
        const int n0 = dop0 ? 2 * S * nt0 : 0, n1 = dop1 ? 2 * S * nt1 : 0;
        for (int e = tid; e < n0 + n1; e += 256) {
            const int j = e >= n0 ? 1 : 0, r = e - (j ? n0 : 0), nt = j ? nt1 : nt0;
            const int cs = r / nt, k = r - cs * nt, cc = cs / S, sym = cs - cc * S;
            const float t = (float)sym * a.t_sym;
            const float* th = sTh + (j * 2 + cc) * kSinusoids * 16 + k;
            const float* fc = sFc + (j * 2 + cc) * kSinusoids * 16 + k;
            float sum = 0.f;
            for (int n = 0; n < kSinusoids; ++n) sum += jakes_cos(t, fc[n * 16], th[n * 16]);
            const float cf = (j ? P1.coeff : P0.coeff)[k] * kJakesNorm;
            reinterpret_cast<float*>(sTapD + (j * S + sym) * 16 + k)[cc] = sum * cf;
        }
    }
    __syncthreads();
    if constexpr (DOPPLER) {       // g[s] = taps[s] . alpha (k ascending)
        const int n0 = dop0 ? S * P0.L : 0, n1 = dop1 ? S * P1.L : 0;
        for (int e = tid; e < n0 + n1; e += 256) {
            const int j = e >= n0 ? 1 : 0, r = e - (j ? n0 : 0), Lj = j ? P1.L : P0.L, nt = j ? P1.n_taps : P0.n_taps;
            const int sym = r / Lj, l = r - sym * Lj;
            const float* al = (j ? P1.alpha : P0.alpha) + l;      // (taps_dot_alpha, written out: the call changes the registers
            const float2* tp = sTapD + (j * S + sym) * 16;        // this kernel gets)
            float2 acc = make_float2(0.f, 0.f);
            for (int k = 0; k < nt; ++k) {
                const float wgt = al[k * Lj];
                acc.x += tp[k].x * wgt;
                acc.y += tp[k].y * wgt;
            }
            sGd[(j * S + sym) * 64 + l] = acc;
        }
    }
    if (a.tx_out != nullptr)
        for (int i = tid; i < nfr * 2 * T; i += 256) {
            const int fr = i / (2 * T);
            a.tx_out[(size_t)f0 * 2 * T + i] = reinterpret_cast<const float*>(sTX)[fr * 2 * TP + 2 * kGenFirPad + (i - fr * 2 * T)];
        }
    // frequency response of the block's frames (freq_response, its twiddles from the table: same arguments, same bits)
    if constexpr (DOPPLER) __syncthreads();            // the per-symbol responses are complete
    if (a.H != nullptr) {
        const auto twt = [](int m) { return tw[m]; };         // (tw is in LDS: static storage, nothing to capture)
        for (int idx = tid; idx < nfr * K; idx += 256) {
            const int fr = idx / K, f = idx - fr * K, Lf = fr == 0 ? L0 : L1;
            if (fr == 0 ? dop0 : dop1) continue;       // (a Doppler frame writes S distinct responses: below)
            const float2 acc = freq_response(gs[fr], Lf, f, K, twt);
            for (int r = 0; r < a.h_rep; ++r) a.H[((size_t)(f0 + fr) * a.h_rep + r) * K + f] = acc;
        }
        if constexpr (DOPPLER) {                       // H[f, s] = fft(g[s], K) (h_rep == S)
            for (int idx = tid; idx < nfr * S * K; idx += 256) {
                const int fs = idx / K, f = idx - fs * K, fr = fs / S, Lf = fr == 0 ? L0 : L1;
                if (!(fr == 0 ? dop0 : dop1)) continue;
                const float2* gp = sGd + fs * 64;
                float2 acc = make_float2(0.f, 0.f);           // (freq_response, written out: the call moves one instruction)
                for (int l = 0; l < Lf; ++l) {
                    const float2 t2 = tw[(f * l) % K];
                    cmac(acc, gp[l], t2);
                }
                a.H[((size_t)(f0 + fr) * S + (fs - fr * S)) * K + f] = acc;
            }
        }
    }
    // 4. 'same' FIR and its power
    const int off0 = (L0 - 1) / 2, off1 = (L1 - 1) / 2, Lmax = max(L0, nfr > 1 ? L1 : 0);
    double pw = 0.0;
    {
        float2 yv[NSMP];
#pragma unroll
        for (int q = 0; q < NSMP; ++q) {
            const int i = min(tid + 256 * q, nfr * T - 1), fr = i / T, t = i - fr * T;
            const float2* xf = sTX + fr * TP + kGenFirPad + t + (fr == 0 ? off0 : off1);
            float2 acc = make_float2(0.f, 0.f);
            if constexpr (DOPPLER) {
                // a static frame: its own L taps (the terms the static instantiation adds behind L are zeros).  A Doppler frame:
                // fir_doppler_kernel's window r = tl + off - l in [-n_taps, n_sc) of symbol t / n_sc, l ascending; what lies
                // before the frame's first sample is the zero pad
                constexpr int NSC = K + CP;
                const bool dp = fr == 0 ? dop0 : dop1;
                const int Lf = fr == 0 ? L0 : L1, sym = t / NSC, r0 = t - sym * NSC + (fr == 0 ? off0 : off1);
                const int ntf = fr == 0 ? P0.n_taps : P1.n_taps;
                const int lo = dp ? max(0, r0 - NSC + 1) : 0, hi = dp ? min(Lf - 1, r0 + ntf) : Lf - 1;
                const float2* gp = dp ? sGd + (fr * S + sym) * 64 : gs[fr];
                for (int l = lo; l <= hi; ++l) {
                    const float2 v = xf[-l];
                    cmac(acc, gp[l], v);
                }
            } else {
                for (int l = 0; l < ((a.abl & 8) ? 1 : Lmax); ++l) {
                    const float2 v = xf[-l];
                    cmac(acc, gs[fr][l], v);
                }
            }
            yv[q] = acc;
        }
#pragma unroll
        for (int q = 0; q < NSMP; ++q) {
            const int i = tid + 256 * q;
            if (i < nfr * T) {
                out_store2<5>(reinterpret_cast<float*>(a.y + (size_t)f0 * T + i), yv[q].x, yv[q].y);
                pw += (double)yv[q].x * yv[q].x + (double)yv[q].y * yv[q].y;
            }
        }
    }
    pw = wave_sum(pw);
    nw = wave_sum(nw);
    if (lane == 0) { sh[0][w] = pw; sh[1][w] = nw; }
    __syncthreads();
    if (tid == 0) {
        a.power_partial[block] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
        if (a.noise_partial != nullptr) a.noise_partial[block] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
    }
}
template <int S, int K, int CP>
constexpr size_t gen_static_smem_bytes() {
    return (size_t)16 * (2 * K + 4) * sizeof(float) + (size_t)kGenFramesPerBlock * (S * (K + CP) + 2 * kGenFirPad) * sizeof(float2);
}
template <int S, int K, int CP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void gen_static_frames_kernel(const GenStaticArgs a0, const GenChainScalars gc,
                                                                                                           const ChainOffs co) {
    DCCN_GEN_ARGS_OF_CHAIN(a, P0, P1, a0, gc, co.off[blockIdx.z], blockIdx.z, (int)blockIdx.x)
    gen_static_frames_body<S, K, CP>(a, P0, P1, (int)blockIdx.x);
}
// the launch for descriptors with Doppler frames.  33.5 KB of LDS more than the static launch (per-symbol responses 7 KB, taps
// 1.75 KB, phases 12 KB, Doppler shifts 12 KB): 54.9 KB per workgroup (CP = 4: 53.5 KB), two workgroups per CU instead of the
// static launch's three -- 512 resident workgroups, which a 73-frame batch (37) never reaches and a 1170-frame batch (585) passes either way
template <int S, int K, int CP>
constexpr size_t gen_doppler_smem_bytes() {
    return gen_static_smem_bytes<S, K, CP>() + (size_t)kGenFramesPerBlock * (S * 64 + S * 16) * sizeof(float2) +
           (size_t)2 * kGenFramesPerBlock * 2 * kSinusoids * 16 * sizeof(float);
}
template <int S, int K, int CP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void gen_doppler_frames_kernel(const GenStaticArgs a0, const GenChainScalars gc,
                                                                                                            const ChainOffs co) {
    DCCN_GEN_ARGS_OF_CHAIN(a, P0, P1, a0, gc, co.off[blockIdx.z], blockIdx.z, (int)blockIdx.x)
    gen_static_frames_body<S, K, CP, true>(a, P0, P1, (int)blockIdx.x);
}
// x = y / sqrt(mean |y|^2) + noise where a buffer is wanted (the first batch of a pipelined loop, tests, iq dumps):
// scale_add_noise on the generator's y and noise, and `noise_power:0` from its partials when npow_out is given.
// grid: any; 256 threads.  This kernel serves chain groups (common.h).
static __global__ __launch_bounds__(256) void gen_static_apply_kernel(const float4* y_, const float4* noise_, const double* ppart_, int npart,
                                                               double total, float4* x_, long long n4, const double* npart_noise_,
                                                               int n_noise, float* npow_out_, const ChainOffs co) {
    const long long coff = co.off[blockIdx.z];
    const float4* __restrict__ y = chain_at(y_, coff);
    const float4* __restrict__ noise = chain_at(noise_, coff);
    const double* __restrict__ ppart = chain_at(ppart_, coff);
    float4* __restrict__ x = chain_at(x_, coff);
    const double* __restrict__ npart_noise = chain_at(npart_noise_, coff);
    float* __restrict__ npow_out = chain_at(npow_out_, coff);
    __shared__ double sh4[4];
    __shared__ float s_inv;
    const float inv = batch_power_inv_scale(ppart, npart, total, sh4, &s_inv);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
        x[i] = scale_add_noise(y[i], inv, noise[i]);
    if (npow_out != nullptr && blockIdx.x == 0) noise_power_from_partials(npart_noise, n_noise, total, sh4, npow_out);
}
// the same for a cp=False receiver (model.py:1236-1240 drops the cyclic prefix inside the graph): x [frames, S, K, 2] holds the K
// samples behind the prefix of every symbol, x[f, s, 0:K] = y[f, s, CP:CP+K] * inv + noise[f, s, CP:CP+K] -- the scale still that
// of the whole frames (total = frames * S * (K + CP)): the bits of the full output, cropped.  In float4s: output i is element
// i % kw4 of symbol i / kw4 (symbols of all frames are consecutive), whose source symbol has sym4 = 2 (K + CP) / 4 float4s
// with the window off4 = 2 CP / 4 into it.  Its own loop, not a shared body with a flag: the plain kernel pays no division per
// element, and behind a common body this kernel's address arithmetic changes.  No chain table.  grid: any; 256 threads.
static __global__ __launch_bounds__(256) void gen_static_apply_window_kernel(const float4* __restrict__ y, const float4* __restrict__ noise,
                                                                      const double* __restrict__ ppart, int npart, double total,
                                                                      float4* __restrict__ x, long long n4, int kw4, int sym4, int off4,
                                                                      const double* __restrict__ npart_noise, int n_noise,
                                                                      float* __restrict__ npow_out) {
    __shared__ double sh4[4];
    __shared__ float s_inv;
    const float inv = batch_power_inv_scale(ppart, npart, total, sh4, &s_inv);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const long long sym = i / kw4, src = sym * sym4 + off4 + (i - sym * kw4);
        x[i] = scale_add_noise(y[src], inv, noise[src]);
    }
    if (npow_out != nullptr && blockIdx.x == 0) noise_power_from_partials(npart_noise, n_noise, total, sh4, npow_out);
}
// gen_static_apply_kernel and frame_sync_kernel (frame_sync.h) as ONE launch (dccn_gen_static_apply_sync): a training batch
// aligned by the cyclic-prefix estimator without x going to memory and back in between.  frame_sync_kernel's geometry (one wave
// per frame, kSyncWaves frames per 256-thread block, its LDS region per frame, no atomics, no workspace); in place of its step 1
// the wave forms its frame in LDS with batch_power_inv_scale / scale_add_noise -- the fp32 values gen_static_apply_kernel writes
// -- and steps 2-5 are frame_sync.h's device functions, so x_out and offset carry the bits of the two-launch sequence.  Block 0
// serves `noise_power:0` as the apply kernels do.  H (nullable, [frames, h_rep, K] complex: the generator's freq_response rows,
// column k = DFT bin k) is rotated with the frame: aligned[n] = x[n + theta] has the response H[k] exp(+2 pi i k theta / K), the
// integer k theta reduced mod K first and the factor from sincospif, so it is exact at every multiple of a quarter turn.  No
// chain table.
struct GenApplySyncArgs {
    const float4* y; const float4* noise; const double* ppart; int npart; double total;
    float* x_out; int32_t* offset; float2* H; int h_rep;
    const double* npart_noise; int n_noise; float* npow_out;
    int frames, S, K, CP, W, crop;
};
static __global__ void __launch_bounds__(kSyncWaves * kSyncLanes) gen_apply_sync_kernel(const GenApplySyncArgs a) {
    extern __shared__ float4 sync_lds[];
    __shared__ double sh4[4];
    __shared__ float s_inv;
    const float inv = batch_power_inv_scale(a.ppart, a.npart, a.total, sh4, &s_inv);
    if (a.npow_out != nullptr && blockIdx.x == 0) noise_power_from_partials(a.npart_noise, a.n_noise, a.total, sh4, a.npow_out);
    const int lane = threadIdx.x & (kSyncLanes - 1), wave = threadIdx.x / kSyncLanes;
    const int T = a.S * (a.K + a.CP);
    const long long f = (long long)blockIdx.x * kSyncWaves + wave;
    const bool live = f < a.frames;          // (a ragged last block: the wave still meets the block's barriers)
    float4* const region = sync_lds + (size_t)wave * (frame_sync_lds_per_frame(T) / 16);
    float2* const yf = reinterpret_cast<float2*>(region);
    float4* const pe = region + T / 2;

    // 1. the frame x = y * inv + noise, formed once, into LDS
    if (live) {
        const float4* __restrict__ ys = a.y + (size_t)f * (T / 2);
        const float4* __restrict__ zs = a.noise + (size_t)f * (T / 2);
        for (int i = lane; i < T / 2; i += kSyncLanes) region[i] = scale_add_noise(ys[i], inv, zs[i]);
    }
    const int theta = frame_sync_estimate(yf, pe, lane, live, a.S, a.K, a.CP, a.W, nullptr);
    if (!live) return;
    if (lane == 0) a.offset[f] = theta;
    frame_sync_store(yf, a.x_out + (size_t)f * a.S * (a.crop ? a.K : a.K + a.CP) * 2, theta, lane, a.S, a.K, a.CP, a.crop);
    if (a.H != nullptr) {
        float2* __restrict__ Hf = a.H + (size_t)f * a.h_rep * a.K;
        for (int i = lane; i < a.h_rep * a.K; i += kSyncLanes) {
            const int k = i % a.K;
            const int m = ((k * theta) % a.K + a.K) % a.K;          // (|k theta| < K W: no overflow)
            float sn, cs;
            sincospif(2.0f * (float)m / (float)a.K, &sn, &cs);
            const float2 h = Hf[i];
            Hf[i] = make_float2(h.x * cs - h.y * sn, h.x * sn + h.y * cs);
        }
    }
}

// radio.py:62-88 AWGN_channel, the *in-graph* monitor branch of the receiver graph (ofdmreceiver_np.py:136,151-152):
// xn = batch-normalised (eps 1e-8) clipped signal / sqrt(2) (computed by the caller with the R0 kernel),
// level = sqrt(.5) 10^(-SNR/20) per frame, amp = level * N(0,1), phase = U(0, 2 pi),
// noise = (|amp| sin(phase), |amp| cos(phase)); iq_rx = fp16(xn + noise), iq_tx = fp16(clipped signal),
// noise_power = mean(noise_re^2 + noise_im^2).  The receiver never consumes this branch (`rx_iq_data = iq_tx_re`);
// it only feeds the constellation dumps and the printed noise power.  grid = (ceil(T/256), frames).
static __global__ __launch_bounds__(256) void ingraph_awgn_kernel(const float2* __restrict__ clipped,
                                                           const float2* __restrict__ xn,
                                                           const float* __restrict__ snr_db, __half2* __restrict__ iq_tx,
                                                           __half2* __restrict__ iq_rx, double* __restrict__ noise_partial,
                                                           int T, unsigned offset, unsigned long long seed) {
    __shared__ double sh[4];
    const int fr = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    double pw = 0.0;
    if (t < T) {
        const size_t i = (size_t)fr * T + t;
        const float level = frame_noise_std(snr_db[fr]);
        const Philox4 p = philox4x32_10((unsigned long long)i, kStreamNoise, offset, seed);     // (word 2 is used as well: not normal_pair)
        const float amp = fabsf(level * box_muller(p.v[0], p.v[1]).x);
        float sn, cs;
        sincosf(6.2831853071795864769f * uniform01(p.v[2]), &sn, &cs);
        const float nr = amp * sn, ni = amp * cs;
        const float2 v = xn[i];
        if (iq_rx) iq_rx[i] = __floats2half2_rn(v.x + nr, v.y + ni);
        if (iq_tx) {
            const float2 c = clipped[i];
            iq_tx[i] = __floats2half2_rn(c.x, c.y);
        }
        pw = (double)nr * nr + (double)ni * ni;
    }
    pw = block_sum4(pw, sh);
    if (threadIdx.x == 0) noise_partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = pw;
}

// radio.py:376-407 Jakes sum-of-sinusoids Doppler (doppler_phase, jakes_shift, jakes_cos above): per OFDM symbol s
// (t = s * n_sc / Fs) and tap k the tap (mu_re + i mu_im) coeff_k sqrt(1/48);  g[s] = taps[s] . alpha;  H[s] = fft(g[s])
// theta_in [frames, 2, 48, n_taps] (uniform phases in [0, 2 pi)) == nullptr: draw them.  One block per frame.
static __global__ __launch_bounds__(64) void doppler_taps_kernel(const float* __restrict__ theta_in,
                                                          const float* __restrict__ coeff,
                                                          const float* __restrict__ alpha, float2* __restrict__ g,
                                                          float2* __restrict__ H, int n_taps, int L, int nfft, int S,
                                                          float Fd, float t_sym, unsigned offset,
                                                          unsigned long long seed, const int* __restrict__ frames,
                                                          int tap_stride, int g_stride) {
    __shared__ float2 tap[16 * 16];          // [S][n_taps], S <= 16
    __shared__ float2 gs[16 * 64];           // [S][L]
    const int fr = frames ? frames[blockIdx.x] : (int)blockIdx.x;
    for (int e = threadIdx.x; e < S * n_taps; e += 64) {
        const int sym = e / n_taps, k = e % n_taps;
        const float t = (float)sym * t_sym;
        float sr = 0.f, si = 0.f;
        for (int n = 0; n < kSinusoids; ++n) {
            float thr, thi;
            if (theta_in) {
                thr = theta_in[(((size_t)fr * 2 + 0) * kSinusoids + n) * tap_stride + k];
                thi = theta_in[(((size_t)fr * 2 + 1) * kSinusoids + n) * tap_stride + k];
            } else {
                thr = doppler_phase(fr, 0, n, k, tap_stride, offset, seed);
                thi = doppler_phase(fr, 1, n, k, tap_stride, offset, seed);
            }
            sr += jakes_cos(t, jakes_shift(Fd, 0, n, k), thr);
            si += jakes_cos(t, jakes_shift(Fd, 1, n, k), thi);
        }
        const float c = coeff[k] * kJakesNorm;
        tap[sym * n_taps + k] = make_float2(sr * c, si * c);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < S * L; e += 64) {
        const int sym = e / L, l = e % L;
        const float2 a = taps_dot_alpha(tap + sym * n_taps, alpha, n_taps, L, l);
        gs[e] = a;
        g[(size_t)fr * g_stride + sym * L + l] = a;
    }
    __syncthreads();
    if (H) {
        for (int e = threadIdx.x; e < S * nfft; e += 64) {
            const int sym = e / nfft, f = e % nfft;
            float2 a = make_float2(0.f, 0.f);              // (freq_response, written out on gs[sym * L + l]: called on the
            for (int l = 0; l < L; ++l) {                  // pointer gs + sym * L, this kernel loses a wait state)
                const float2 w = twiddle_of((f * l) % nfft, nfft);
                cmac(a, gs[sym * L + l], w);
            }
            H[((size_t)fr * S + sym) * nfft + f] = a;
        }
    }
}

// radio.py:385-407 per-symbol impulse response with n_taps samples of history: symbol s filters the segment
// x[s*n_sc - n_taps .. (s+1)*n_sc) with np.convolve(., g_s, 'same') and keeps its last n_sc outputs, i.e.
// y[s*n_sc + t] = sum_l g_s[l] x[s*n_sc + t + off - l] over t + off - l in [-n_taps, n_sc) (nothing beyond the
// symbol's own end, nothing before the frame).  grid = (ceil(T/256), frames); + partial sums of |y|^2.
static __global__ __launch_bounds__(256) void fir_doppler_kernel(const float2* __restrict__ x, const float2* __restrict__ g,
                                                          float2* __restrict__ y, double* __restrict__ partial, int T,
                                                          int L, int n_sc, int n_taps, const int* __restrict__ frames,
                                                          int g_stride, int n_frames, int pbase) {
    __shared__ double sh[4];
    const int bx = (T + 255) / 256;
    const int off = (L - 1) / 2;
    double pw = 0.0;
    const int items = n_frames * bx, ipb = (items + (int)gridDim.x - 1) / (int)gridDim.x;
    for (int item = blockIdx.x * ipb; item < min(items, ((int)blockIdx.x + 1) * ipb); ++item) {      // persistent: see fir_same_kernel
        const int fi = item / bx, cb = item - fi * bx;
        const int fr = frames ? frames[fi] : fi;
        const int t = cb * 256 + threadIdx.x;
        if (t < T) {
            const int sym = t / n_sc, tl = t - sym * n_sc;
            const float2* xf = x + (size_t)fr * T;
            const float2* gf = g + (size_t)fr * g_stride + sym * L;
            float2 a = make_float2(0.f, 0.f);
            for (int l = 0; l < L; ++l) {
                const int r = tl + off - l;                     // position relative to the symbol start
                const int u = sym * n_sc + r;
                if (r < -n_taps || r >= n_sc || u < 0) continue;
                const float2 v = xf[u];
                cmac(a, gf[l], v);
            }
            y[(size_t)fr * T + t] = a;
            pw += (double)a.x * a.x + (double)a.y * a.y;
        }
    }
    pw = block_sum4(pw, sh);
    if (threadIdx.x == 0) partial[pbase + blockIdx.x] = pw;
}

}  // namespace dccn

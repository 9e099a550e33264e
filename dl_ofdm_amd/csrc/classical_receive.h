// The label-free classical detector of the receive path as ONE launch (include/dccn.h "classical receive"): frames as the
// front end writes them -> FFT window -> pilot LS -> interpolation -> (ALMMSE) -> one-tap equalisation -> hard bits packed
// as decide.h packs them, plus max-log LLRs.  The noise variance is the frame's own: the mean power of its empty carriers.
// No workspace, no atomics, no frame depends on another; nothing goes to memory between the stages except the nullable
// outputs.  The stages around the DFT restate classical.h's per-cell expressions (pilot LS, ALMMSE, detection), so the
// decision is bit for bit classical_detect_kernel's on this kernel's own Y and G.
//
// Definition, per frame f of x [frames, S, K+CP, 2] (fp32).  -ffp-contract=off: every a*b+c below is two roundings; the MFMA
// is the one fused operation.
//   1. xw[s, t] = x[f, s, win + t], t < K.   Y[s] = xw[s] . dft   (dft [2K, 2K] real-expanded, rows/columns 2t / 2t+1 = I / Q)
//        ORDER: v_mfma_f32_16x16x4_f32 steps over the 2K real inputs i = 0, 4, 8, ...; step i adds the products of inputs
//        i, i+1, i+2, i+3 to the accumulator as a chain of fp32 FMAs in that order (one rounding per product).  The same for
//        every row, whatever its place in the tile.
//   2. gp[j] = Y[pil[j]] / pv:  d = pv.x pv.x + pv.y pv.y;  re = (y.x pv.x + y.y pv.y) / d;  im = (y.y pv.x - y.x pv.y) / d
//   3. Gls[c] = sum_j gp[j] w[j, c]    ORDER: j = 0, 1, ..., P-1, acc = acc + gp[j] * w[j, c] from acc = 0, each plane alone
//   4. nv = noise_var when > 0, else max(sum_e |Y[empty[e]]|^2 / E, kClsRxTinyNoise)
//        ORDER: lane l of one wave adds e = l, l + 64, ... from 0 (|y|^2 = y.x y.x + y.y y.y), then common.h wave_sum
//        kClsRxTinyNoise = 1e-20: a noise-free frame (empty cells hold rounding residue or exact zeros) keeps finite LLRs as
//        long as |G|^2 (d0 - d1) < 3e18; the reference grids have |G|^2 of the order of K
//      c = nv / (pv.x pv.x + pv.y pv.y)
//   5. mode 0 (LS): G = Gls.   mode 2 (ALMMSE): v[k] = (sum_s Gls[s, k]) / S   (s ascending from 0; re and im alone);
//        e = (sum_k |v[k]|^2) / S   ORDER: lane l adds k = l, l + 64, ... from 0, then wave_sum;   wgt = e / (e + c);
//        G[s, k] = (v[k].x * wgt, v[k].y * wgt)
//   6. at data cell dat[i]: g = G, y = Y, d = g.x g.x + g.y g.y, xh = ((y.x g.x + y.y g.y) / d, (y.y g.x - y.x g.y) / d);
//        d_q = (xh.x - table[q].x)^2 + (xh.y - table[q].y)^2; best = first minimum (d_q < running minimum from 3e38);
//        hard = labels[best];  llr[b] = (d / nv) * (min_{labels[q, b] = 0} d_q - min_{labels[q, b] = 1} d_q), from the SAME
//        d_q: llr > 0 => bit 1, llr < 0 => bit 0 exactly (positive = bit 1, the receive path's convention)
//   7. packed row f = numpy.packbits(hard[f].reshape(-1)) (decide.h's layout and store_row_bytes; rows need no alignment)
// Device-side index lists cannot be checked on the host: every entry of pil / dat / empty is clamped to [0, S K).
//
// Blocking.  The DFT is the only contraction with real work (S x 2K x 2K per frame).  A 16-row MFMA tile holds FPB = 16 / S
// whole frames (two at S = 7; the rows left over are zero); a block of four waves owns one such tile: it reads the frames'
// FFT windows once into LDS (16-byte loads; a window that starts on an odd sample has an 8-byte half at each end, as
// frame_sync.h reads such a window), wave w runs the 16-column tiles w, w + 4, ... of Y, and the stages behind the DFT are
// VALU work on the LDS-resident Y.  The DFT matrix is NOT staged: with 16 rows per block every element of it feeds exactly
// one MFMA of the block, so a copy in LDS would be written once and read once -- the same L2 traffic plus an LDS round
// trip, and 64 KB (K = 64) per block would leave two blocks per CU; at K = 128 (256 KB) it does not fit at all.  Lane
// (c, kq) reads dft[4 i + kq][16 t + c] straight into the B operand (16 lanes = one 64-byte segment; the matrix stays in L2).
// LDS (floats): xw 16 (2K + 4) (row pad 4: the 64 lanes of an A read hit 64 banks; reused for G once the DFT is done),
// Y 16 * 2K, gp 2 FPB P, 32 scalars.  K = 64, P = 16: 16.6 KB; K = 128, P = 32: 32.9 KB; refused beyond 48 KB.
#pragma once
#include "classical.h"
#include "decide.h"

namespace dccn {

constexpr int kClsRxThreads = 256;
constexpr int kClsRxRows = 16;             // rows of the MFMA tile
constexpr int kClsRxPad = 4;               // floats between the rows of the window tile
constexpr float kClsRxTinyNoise = 1e-20f;
constexpr size_t kClsRxMaxLds = 48 * 1024;

// What a launch's links share, and what one link is (the solo launch has one; dccn_classical_receive_grouped a table of them).
struct ClsRxShape {
    int frames, S, K, CP, P, D, E, fpb;
};
struct ClsRxLink {
    int nbits, win, mode, RB;                                      // RB: bytes of a packed row, ceil(D nbits / 8)
    float noise_var;
    float2 pv;
    const float* dft; const float* w; const int* pil; const int* dat; const int* empty;
    const float2* table; const int* labels; const float* x;
    unsigned char* packed; float* llr; float2* chest; float2* y_freq; float* noise;
};
struct ClsRxParams {
    ClsRxLink l;
    ClsRxShape s;
};

// floats of dynamic LDS (host and device agree on the layout through this and the kernel's carving)
static inline size_t clsrx_lds_floats(int S, int K, int P) {
    const int fpb = kClsRxRows / S;
    return (size_t)kClsRxRows * (2 * K + kClsRxPad) + (size_t)kClsRxRows * 2 * K + (size_t)2 * fpb * P + 32;
}

typedef float clsrx_f32x4 __attribute__((ext_vector_type(4)));

// One tile of one link: block blockIdx.x of the link's ceil(frames / fpb) blocks, whatever else the grid carries.
template <int NB>
__device__ __forceinline__ void classical_receive_body(const ClsRxLink& p, const ClsRxShape& sh) {
    extern __shared__ __align__(16) float clsrx_smem[];
    constexpr int M = 1 << NB;
    const int K = sh.K, S = sh.S, K2 = 2 * K, SK = S * K, ldx = K2 + kClsRxPad, P = sh.P;
    float* xs = clsrx_smem;                                        // [16][ldx]   FFT windows (dead after the DFT)
    float2* G = reinterpret_cast<float2*>(clsrx_smem);            // [fpb][SK]   Gls, then G
    float* Yf = clsrx_smem + kClsRxRows * ldx;                    // [16][2K]
    float2* Y = reinterpret_cast<float2*>(Yf);                    // [fpb][SK]: row fi S + s of the tile is symbol s of frame fi
    float2* gp = reinterpret_cast<float2*>(Yf + kClsRxRows * K2); // [fpb][P]
    float* s_nv = reinterpret_cast<float*>(gp + sh.fpb * P);       // [16]
    int* s_lab = reinterpret_cast<int*>(s_nv + 16);               // [16]  labels of point q, bit b at position NB-1-b
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = lane & 15, kq = lane >> 4;
    const long long f0 = (long long)blockIdx.x * sh.fpb;
    const int nf = (int)min((long long)sh.fpb, (long long)sh.frames - f0);
    const int rows = nf * S;
    const int last_cell = SK - 1;

    // ---- the frames' FFT windows -> LDS (rows past the block's frames are zero) ----
    {
        const int n_sc = K + sh.CP;
        const bool odd = (p.win & 1) != 0;
        const int cpr = K2 / 4 + (odd ? 1 : 0);                    // chunks per row
        const float* src0 = p.x + ((size_t)f0 * S * n_sc + p.win) * 2;
        for (int i = tid; i < kClsRxRows * cpr; i += kClsRxThreads) {
            const int r = i / cpr, j = i - r * cpr;
            const float* src = src0 + (size_t)r * n_sc * 2;
            float* dst = xs + r * ldx;
            const bool live = r < rows;
            if (!odd) {
                const float4 v = live ? *reinterpret_cast<const float4*>(src + 4 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(dst + 4 * j) = v;
            } else if (j == 0 || j == cpr - 1) {
                const int o = j == 0 ? 0 : K2 - 2;
                const float2 v = live ? *reinterpret_cast<const float2*>(src + o) : make_float2(0.f, 0.f);
                *reinterpret_cast<float2*>(dst + o) = v;
            } else {
                const int o = 4 * j - 2;
                const float4 v = live ? *reinterpret_cast<const float4*>(src + o) : make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float2*>(dst + o) = make_float2(v.x, v.y);
                *reinterpret_cast<float2*>(dst + o + 2) = make_float2(v.z, v.w);
            }
        }
        if (tid < M) {
            int mask = 0;
#pragma unroll
            for (int b = 0; b < NB; ++b) mask |= (p.labels[tid * NB + b] != 0 ? 1 : 0) << (NB - 1 - b);
            s_lab[tid] = mask;
        }
    }
    __syncthreads();

    // ---- Y = xw . dft: wave wv owns the 16-column tiles wv, wv + 4, ... ----
    // Two tiles at a time share each A operand and give the matrix core two independent accumulators (a dependent
    // 16x16x4 f32 MFMA issues every 40 cycles, an independent one every 32); each accumulator's chain is the stated order.
    const int ntile = K2 / 16;
    for (int t0 = wv; t0 < ntile; t0 += 8) {
        const int t1 = t0 + 4;
        const bool two = t1 < ntile;
        clsrx_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const float* a = xs + c * ldx + kq;
        const float* b0 = p.dft + (size_t)kq * K2 + t0 * 16 + c;
        const float* b1 = p.dft + (size_t)kq * K2 + (two ? t1 : t0) * 16 + c;
        for (int i0 = 0; i0 < K2; i0 += 32) {                     // (K % 16 == 0) eight steps' operands requested together
            float av[8], bv0[8], bv1[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                av[u] = a[i0 + 4 * u];
                bv0[u] = b0[(size_t)(i0 + 4 * u) * K2];
                bv1[u] = b1[(size_t)(i0 + 4 * u) * K2];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv0[u], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv1[u], acc1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {                              // C/D: col = lane % 16, row = 4 (lane / 16) + r
            Yf[(4 * kq + r) * K2 + t0 * 16 + c] = acc0[r];
            if (two) Yf[(4 * kq + r) * K2 + t1 * 16 + c] = acc1[r];
        }
    }
    __syncthreads();

    // ---- LS at the pilots, the frames' noise variance, Y out ----
    const float pd = p.pv.x * p.pv.x + p.pv.y * p.pv.y;
    for (int i = tid; i < nf * P; i += kClsRxThreads) {
        const int fi = i / P, j = i - fi * P;
        const float2 y = Y[fi * SK + min(max(p.pil[j], 0), last_cell)];
        gp[i] = make_float2((y.x * p.pv.x + y.y * p.pv.y) / pd, (y.y * p.pv.x - y.x * p.pv.y) / pd);
    }
    for (int fi = wv; fi < nf; fi += 4) {
        float nv = p.noise_var;
        if (!(nv > 0.f)) {
            float a = 0.f;
            for (int e = lane; e < sh.E; e += 64) {
                const float2 y = Y[fi * SK + min(max(p.empty[e], 0), last_cell)];
                a += y.x * y.x + y.y * y.y;
            }
            nv = fmaxf(wave_sum(a) / (float)sh.E, kClsRxTinyNoise);
        }
        if (lane == 0) {
            s_nv[fi] = nv;
            if (p.noise != nullptr) p.noise[f0 + fi] = nv;
        }
    }
    if (p.y_freq != nullptr)
        for (int i = tid; i < nf * SK; i += kClsRxThreads) p.y_freq[(size_t)f0 * SK + i] = Y[i];
    __syncthreads();

    // ---- interpolation over the grid (a thread per cell; two frames share each weight) ----
    for (int cell = tid; cell < SK; cell += kClsRxThreads) {
        for (int fb = 0; fb < nf; fb += 2) {
            const bool two = fb + 1 < nf;
            const float2* g0 = gp + fb * P;
            const float2* g1 = gp + (two ? fb + 1 : fb) * P;
            float r0 = 0.f, i0 = 0.f, r1 = 0.f, i1 = 0.f;
            for (int j = 0; j < P; ++j) {
                const float wj = p.w[(size_t)j * SK + cell];
                const float2 a0 = g0[j], a1 = g1[j];
                r0 += a0.x * wj; i0 += a0.y * wj;
                r1 += a1.x * wj; i1 += a1.y * wj;
            }
            G[fb * SK + cell] = make_float2(r0, i0);
            if (two) G[(fb + 1) * SK + cell] = make_float2(r1, i1);
        }
    }
    __syncthreads();

    // ---- ALMMSE: a wave per frame ----
    if (p.mode == CE_ALMMSE) {
        for (int fi = wv; fi < nf; fi += 4) {
            float2* g = G + fi * SK;
            float pe = 0.f;
            for (int k = lane; k < K; k += 64) {
                float vr = 0.f, vi = 0.f;
                for (int s = 0; s < S; ++s) { vr += g[s * K + k].x; vi += g[s * K + k].y; }
                vr /= (float)S; vi /= (float)S;
                g[k] = make_float2(vr, vi);                        // (row 0 of column k: this lane's own)
                pe += vr * vr + vi * vi;
            }
            const float e = wave_sum(pe) / (float)S;
            const float cv = s_nv[fi] / pd;
            const float wgt = e / (e + cv);
            for (int k = lane; k < K; k += 64) {
                const float2 v = g[k];
                const float2 o = make_float2(v.x * wgt, v.y * wgt);
                for (int s = 0; s < S; ++s) g[s * K + k] = o;
            }
        }
        __syncthreads();
    }
    if (p.chest != nullptr)
        for (int i = tid; i < nf * SK; i += kClsRxThreads) p.chest[(size_t)f0 * SK + i] = G[i];

    // ---- decision: a lane per data cell, eight lanes = NB whole bytes of a row (decide.h) ----
    const int gpr = (sh.D + 7) / 8;
    const int total = nf * gpr * 8;
    for (int base = 0; base < total; base += kClsRxThreads) {
        const int t = base + tid;
        const int grp_all = t >> 3, ci = t & 7;
        const int fi = grp_all / gpr, grp = grp_all - fi * gpr;
        const int d = grp * 8 + ci;
        const bool in_frame = fi < nf;
        const bool valid = in_frame && d < sh.D;
        const int fiv = valid ? fi : 0;
        const int cell = valid ? min(max(p.dat[d], 0), last_cell) : 0;
        const float2 y = Y[fiv * SK + cell], g = G[fiv * SK + cell];
        const float gd = g.x * g.x + g.y * g.y;
        const float2 xh = make_float2((y.x * g.x + y.y * g.y) / gd, (y.y * g.x - y.x * g.y) / gd);
        float dq[M];
        int best = 0;
        float bd = 3.0e38f;
#pragma unroll
        for (int q = 0; q < M; ++q) {                              // first minimum, like np.argmin
            const float2 tq = p.table[q];
            const float dx = xh.x - tq.x, dy = xh.y - tq.y;
            const float dd = dx * dx + dy * dy;
            dq[q] = dd;
            if (dd < bd) { bd = dd; best = q; }
        }
        const unsigned hard = (unsigned)s_lab[best];
        if (p.llr != nullptr && valid) {
            const float scale = gd / s_nv[fiv];
            float* dst = p.llr + ((size_t)(f0 + fi) * sh.D + d) * NB;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                float m0 = 3.0e38f, m1 = 3.0e38f;
#pragma unroll
                for (int q = 0; q < M; ++q) {
                    if ((s_lab[q] >> (NB - 1 - b)) & 1) m1 = dq[q] < m1 ? dq[q] : m1;
                    else m0 = dq[q] < m0 ? dq[q] : m0;
                }
                dst[b] = scale * (m0 - m1);
            }
        }
        unsigned v = valid ? hard << (NB * (7 - ci)) : 0u;         // the group's 8 NB bits: cell 0's first bit is the top one
        v = oct_or(v);
        if (in_frame && ci == 0) {
            const int b0 = grp * NB;
            const int n = min(NB, p.RB - b0);                      // bytes of this group that exist in the row
            const unsigned word[2] = {__builtin_bswap32(v << (32 - 8 * NB)), 0u};
            store_row_bytes(p.packed + (size_t)(f0 + fi) * p.RB + b0, word, n);
        }
    }
}

template <int NB>
__global__ __launch_bounds__(kClsRxThreads) void classical_receive_kernel(const ClsRxParams p) {
    classical_receive_body<NB>(p.l, p.s);
}

// Several links per launch (dccn_classical_receive_grouped): each link has its own tables, frames and outputs -- and its own
// modulation; the shape is the call's.  The table travels by value in the kernel arguments and is indexed by blockIdx.y, a
// block-uniform value (scalar loads, as frame_sync.h's link table is read); blockIdx.x stays what the body takes it for, so a
// link's blocks are the solo launch's and no tile holds frames of two links.  The switch on the link's nbits is block-uniform:
// every wave of a block runs one NB body, the solo kernel's, with its expressions and orders.
struct ClsRxGroupArgs {
    ClsRxLink link[kMaxChains];
    ClsRxShape s;
};
static __global__ __launch_bounds__(kClsRxThreads) void classical_receive_grouped_kernel(const ClsRxGroupArgs g) {
    const ClsRxLink& l = g.link[blockIdx.y];
    switch (l.nbits) {
        case 1: classical_receive_body<1>(l, g.s); break;
        case 2: classical_receive_body<2>(l, g.s); break;
        case 3: classical_receive_body<3>(l, g.s); break;
        default: classical_receive_body<4>(l, g.s); break;
    }
}

}  // namespace dccn

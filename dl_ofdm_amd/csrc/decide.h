// The decision stage of the receive path: R3 forward only (dev/py/model.py:1278-1291) and the hard decision of
// dev/py/ofdmreceiver_np.py:166 -- no labels, no cross entropy, no confusion tallies, no block reduction, no finalize stage,
// no workspace.  Per data cell: z = (I, Q) of the dense output -> the NB bit pairs' probabilities (`output:0`, nullable),
// llr = u1 - u0 of the two post-leaky-ReLU logits (= log(p1 / p0), nullable) and the NB hard bits, packed MSB first.
//
// The arithmetic is tail.h's own: tail_fwd_logits to the logits and tail_softmax over each bit pair, the functions the
// evaluation step (tail_cells_out) calls, and the same p1 > p0 -- so a decision here is bit for bit the decision the evaluation
// step tallies.  Consequence: where u1 - u0 is positive but so small that exp rounds to 1, p1 == p0 and the bit is 0 (argmax
// takes the first index on ties) although llr > 0.
//
// Packed layout: row f of `packed` [frames, ceil(D * NB / 8)] is numpy.packbits(hard[f].reshape(-1)) -- bit (d, j) of the
// frame sits at bit position d * NB + j, most significant bit of a byte first, padding bits of the last byte 0.  Eight
// consecutive cells of a row are NB whole bytes: eight lanes form them with an OR over the DPP crossbar (no LDS, no atomics)
// and store them with the widest vector store the address allows (dword / short / bytes).
#pragma once
#include "tail.h"

namespace dccn {

struct DecideEpiParams {
    const float* tailp;
    unsigned char* packed;          // [M, RB]
    float* llr;                     // [M, N/2, NB], nullable
    float* prob;                    // [M, N/2, NB, 2], nullable
    int RB;                         // bytes per row = ceil(N/2 * NB / 8)
    __device__ __forceinline__ DecideEpiParams at_chain(const long long off) const {   // chain groups (common.h)
        DecideEpiParams q = *this;
        q.tailp = chain_at(tailp, off); q.packed = chain_at(packed, off); q.llr = chain_at(llr, off); q.prob = chain_at(prob, off);
        return q;
    }
};

// OR over the 16 lanes of a DPP row / over each group of 8 lanes; the result is in every lane of the row / group
__device__ __forceinline__ unsigned row16_or(unsigned v) {
#pragma unroll
    for (int s = 0; s < 4; ++s) v |= (unsigned)dpp_mov_i32((int)v, s);
    return v;
}
__device__ __forceinline__ unsigned oct_or(unsigned v) {
#pragma unroll
    for (int s = 0; s < 3; ++s) v |= (unsigned)dpp_mov_i32((int)v, s);
    return v;
}

// W data cells through R3 and the decision in one interleaved instruction stream (see tail.h tail_cells for why).
// prob_cell[u] (nullable) -> NB float2, llr_cell[u] (nullable) -> NB floats; hard[u] = the NB bits, bit j at position NB-1-j.
template <int NB, int W>
__device__ __forceinline__ void decide_cells(const float (&z0)[W], const float (&z1)[W], const float* __restrict__ sw,
                                             float* const (&prob_cell)[W], float* const (&llr_cell)[W],
                                             unsigned (&hard)[W]) {
    using L = TailLayout<NB>;
    float c[L::M + 2][W], pre1[L::M][W], pre2[L::O][W];
    tail_fwd_logits<NB, W>(z0, z1, sw, c, pre1, pre2);          // (pre1 is the backward's: not read here)
#pragma unroll
    for (int u = 0; u < W; ++u) hard[u] = 0u;
    float lv[W][NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        float p0[W], p1[W];
#pragma unroll
        for (int u = 0; u < W; ++u) {
            const float u0 = leaky_relu(pre2[2 * j][u]), u1 = leaky_relu(pre2[2 * j + 1][u]);
            const float2 p = tail_softmax(u0, u1);
            p0[u] = p.x;
            p1[u] = p.y;
            lv[u][j] = u1 - u0;
        }
#pragma unroll
        for (int u = 0; u < W; ++u) {
            if (prob_cell[u] != nullptr) *reinterpret_cast<float2*>(prob_cell[u] + 2 * j) = make_float2(p0[u], p1[u]);
        }
#pragma unroll
        for (int u = 0; u < W; ++u) hard[u] |= (p1[u] > p0[u] ? 1u : 0u) << (NB - 1 - j);    // argmax, first index on ties
    }
#pragma unroll
    for (int u = 0; u < W; ++u) {
        if (llr_cell[u] == nullptr) continue;
        if constexpr (NB == 2) *reinterpret_cast<float2*>(llr_cell[u]) = make_float2(lv[u][0], lv[u][1]);
        else if constexpr (NB == 4) *reinterpret_cast<float4*>(llr_cell[u]) = make_float4(lv[u][0], lv[u][1], lv[u][2], lv[u][3]);
        else {
#pragma unroll
            for (int j = 0; j < NB; ++j) llr_cell[u][j] = lv[u][j];
        }
    }
}

// n <= 8 bytes b[0..n) to dst: dwords when dst is 4-byte aligned and n is a multiple of 4, bytes otherwise
__device__ __forceinline__ void store_row_bytes(unsigned char* __restrict__ dst, const unsigned (&word)[2], const int n) {
    if ((reinterpret_cast<uintptr_t>(dst) & 3u) == 0 && (n & 3) == 0) {
        if (n >= 4) *reinterpret_cast<unsigned*>(dst) = word[0];
        if (n >= 8) *reinterpret_cast<unsigned*>(dst + 4) = word[1];
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < n) dst[k] = (unsigned char)((word[k >> 2] >> (8 * (k & 3))) & 0xffu);
    }
}

constexpr int kDecideThreads = 256;

// Stand-alone decision kernel: z [frames, D, 2] + tail weights -> packed / llr / prob.  A lane per cell; lanes 8g .. 8g+7 own
// the eight cells 8 grp .. 8 grp + 7 of one frame (a frame has gpr = ceil(D / 8) such groups; cells past D are masked), i.e.
// NB whole bytes of that frame's row, whatever D and NB are: no byte is shared between groups, rows need no alignment.
// (chain groups, common.h: blockIdx.z = chain, every pointer moves by that chain's arena offset; frames, D, RB and NB are the
// launch's -- a group runs this kernel once per modulation, on the chains of that modulation)
template <int NB>
__global__ __launch_bounds__(kDecideThreads) void demod_decide_kernel(
    const float* __restrict__ z0, const float* __restrict__ tailp0, unsigned char* __restrict__ packed0, float* __restrict__ llr0,
    float* __restrict__ prob0, const int frames, const int D, const int gpr, const int RB, const ChainOffs co) {
    const long long coff = co.off[blockIdx.z];
    const float* __restrict__ z = chain_at(z0, coff);
    const float* __restrict__ tailp = chain_at(tailp0, coff);
    unsigned char* __restrict__ packed = chain_at(packed0, coff);
    float* __restrict__ llr = chain_at(llr0, coff);
    float* __restrict__ prob = chain_at(prob0, coff);
    const float* __restrict__ sw = tail_stage_weights<NB, kDecideThreads>(tailp);
    const long long t = (long long)blockIdx.x * kDecideThreads + threadIdx.x;
    const long long g = t >> 3;
    const int ci = (int)(t & 7);
    const long long f = g / gpr;
    const int grp = (int)(g - f * gpr);
    const int d = grp * 8 + ci;
    const bool valid = f < frames && d < D;
    const long long cell = valid ? f * D + d : 0;                 // masked lanes read cell 0: the load is always legal
    const float2 zv = *reinterpret_cast<const float2*>(z + 2 * cell);
    const float a0[1] = {zv.x}, a1[1] = {zv.y};
    float* const pc[1] = {(prob != nullptr && valid) ? prob + cell * NB * 2 : nullptr};
    float* const lc[1] = {(llr != nullptr && valid) ? llr + cell * NB : nullptr};
    unsigned hard[1];
    decide_cells<NB, 1>(a0, a1, sw, pc, lc, hard);
    // the group's 8 * NB bits: cell 0's first bit is the most significant one
    unsigned v = valid ? hard[0] << (NB * (7 - ci)) : 0u;
    v = oct_or(v);
    if (f < frames) {
        const int b0 = grp * NB;
        const int n = min(NB, RB - b0);                           // bytes of this group that exist in the row
        unsigned char* dst = packed + f * RB + b0;
        const uintptr_t ad = reinterpret_cast<uintptr_t>(dst);
        if (NB == 4 && n == 4 && (ad & 3u) == 0) {
            if (ci == 0) *reinterpret_cast<unsigned*>(dst) = __builtin_bswap32(v);
        } else if (NB == 2 && n == 2 && (ad & 1u) == 0) {
            if (ci == 0) *reinterpret_cast<unsigned short*>(dst) = __builtin_bswap16((unsigned short)v);
        } else if (ci < n) {
            dst[ci] = (unsigned char)((v >> (8 * (NB - 1 - ci))) & 0xffu);
        }
    }
}

}  // namespace dccn

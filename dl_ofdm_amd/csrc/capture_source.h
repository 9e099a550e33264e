// Where a capture's samples come from: the kernels that read a contiguous capture (frame_sync.h's cut,
// pooled estimate and pooled cut; capture_acquire.h's two stages) are bodies over a capture-source type, and the sample format is
// a property of that type alone.  A source is used as a pointer to complex samples is: src + n starts n samples on, src[n] is
// sample n as a float2.
//   CapF32   float32 [n, 2]: the pointer itself, const float2*.  The float32 instantiations are the statements they were.
//   CapSc16  int16 [n, 2], (I, Q) interleaved, native byte order ("sc16", what ADCs and SDR drivers deliver) and a scale:
//            sample n is (float(I) * scale, float(Q) * scale) -- the conversion int16 -> fp32 is exact, each component gets ONE
//            fp32 multiply rounded to nearest (the library is built with -ffp-contract=off: nothing fuses it into what follows).
//            So an sc16 kernel holds, sample for sample, the bits the float32 kernel holds when it is given the capture converted
//            on the host, and everything behind the load is the same code.
// src[n] is one load of one sample (acquisition: any n is naturally aligned, 8 bytes there and 4 here); the window loaders of
// frame_sync.h read several samples per load.
#pragma once
#include "common.h"

namespace dccn {

using CapF32 = const float2*;
// What a body is instantiated over: of(args) is the source, taken where the body first needs it.  CapOfArgs: the float32 capture
// the argument block names (args.cap), read there and then as the float32 kernels always read it.
struct CapOfArgs {
    template <class Args>
    __device__ __forceinline__ CapF32 of(const Args& a) const { return reinterpret_cast<const float2*>(a.cap); }
};

struct CapSc16 {
    const int16_t* cap;         // [n_samples, 2]
    float scale;                // finite, > 0 (the host checked)
    // one sample from its 32-bit word: I in the low half, Q in the high half, both sign-extended
    static __device__ __forceinline__ float2 value(const uint32_t w, const float scale) {
        const float i = (float)(int)(int16_t)(uint16_t)(w & 0xffffu), q = (float)((int)w >> 16);
        return make_float2(i * scale, q * scale);
    }
    template <class Args>
    __device__ __forceinline__ CapSc16 of(const Args&) const { return *this; }      // (its own source: args.cap is not read)
    template <class I>
    __device__ __forceinline__ CapSc16 operator+(const I n) const { return CapSc16{cap + 2 * (long long)n, scale}; }
    template <class I>
    __device__ __forceinline__ float2 operator[](const I n) const { return value(reinterpret_cast<const uint32_t*>(cap)[n], scale); }
};

}  // namespace dccn

// dev_coder.h -- the carry-less range coder (reference: coder.hpp) as lane-serial device code.
// One instance = one serial coder chain.  All arithmetic is unsigned integer and bit-exact with the
// reference: u64 low/code, u32 range, u32 wrap of cum*range (coder.hpp:68-70, 88-92).
#pragma once
#include <hip/hip_runtime.h>
#include "dev_common.h"

#define RC_TOP (1u << 24)   // coder.hpp:24

// Byte sink replacing FilerSave::put (filer.hpp:70-75): a bounded region of the scratch arena.
// pos keeps counting past cap so the caller can detect (and size) an overflow.
struct ByteSink {
    u8* p;
    u32 pos;
    u32 cap;
    __device__ __forceinline__ void put(u8 b) {
        if (pos < cap) p[pos] = b;
        pos++;
    }
};

// Byte source replacing FilerLoad::get (filer.hpp:94-97): 0 past the end.  The decoders are one serial chain per
// lane and every renormalisation needs the next stream byte, so the bytes are fetched eight at a time: one memory
// round trip per eight bytes instead of one per byte (the last seven bytes of a stream are read singly, so
// nothing beyond the stream is ever touched).
struct ByteSrc {
    const u8* p;
    u32 pos;
    u32 n;
    u64 buf;      // bytes already fetched, next one in the low byte
    u32 have;     // how many of them
    __device__ __forceinline__ void init(const u8* ptr, u32 len) { p = ptr; pos = 0; n = len; buf = 0; have = 0; }
    __device__ __forceinline__ u32 get() {
        if (have == 0) {
            if (pos + 8 <= n) {
                const u32* q = reinterpret_cast<const u32*>(p + pos);      // global loads need no alignment on gfx9
                buf = (u64)q[0] | ((u64)q[1] << 32);
                have = 8;
            } else { buf = pos < n ? p[pos] : 0u; have = 1; }
        }
        const u32 b = (u32)buf & 0xffu;
        buf >>= 8; have--;
        pos++;
        return b;
    }
};

// The same for code that runs wave-UNIFORM (every lane the same stream position): there the compiler turns the eight-byte
// fetch above into scalar loads, and scalar loads drop the low two address bits -- an unaligned stream would be read from
// the wrong place.  Byte loads have no such trap.
struct ByteSrc1 {
    const u8* p;
    u32 pos;
    u32 n;
    __device__ __forceinline__ void init(const u8* ptr, u32 len) { p = ptr; pos = 0; n = len; }
    __device__ __forceinline__ u32 get() { const u32 b = pos < n ? p[pos] : 0u; pos++; return b; }
};

// ---- the range coder's step (coder.hpp:66-102), stated once for every device coder -----------------------------------
// renormalisation rounds a symbol may take before its chain is declared broken (rc_renorm has the reason)
#define RC_GUARD 12         // the lane-serial and the masked coders
#define RC_GUARD_MULTI 13   // MultiCoder

// reciprocal for rc_div: floor(2^32 / tot) for tot >= 2 (the estimate is at most 1 below); tot == 1 (only MultiCoder's
// neutral step) keeps 2^32 - 1, which rc_div's single fix-up handles
__device__ __forceinline__ u32 rc_recip(u32 tot) {
    const u32 m0 = 0xFFFFFFFFu / tot;
    return (tot != 1 && (0xFFFFFFFFu - m0 * tot) == tot - 1) ? m0 + 1 : m0;
}
// range / tot (coder.hpp:68) as a multiply-high by recip = rc_recip(tot) plus one exact fix-up
__device__ __forceinline__ u32 rc_div(u32 range, u32 tot, u32 recip) {
    u32 r = __umulhi(range, recip);
    r += (range - r * tot) >= tot ? 1u : 0u;
    return r;
}
// coder.hpp:76-77, the carry clamp: where [low, low + range) crosses a multiple of 2^56, the range that ends at the next
// multiple of 2^24 instead
__device__ __forceinline__ u32 rc_clamped(u64 low, u32 range) {
    if ((low ^ (low + range)) >> 56) range = (((u32)low | (RC_TOP - 1)) - (u32)low);
    return range;
}
// The same for the coders whose step every lane executes, taking effect where nm is all ones (masks, not selects: the
// compiler turns a select between two computed values back into a branch).  With range < 2^24 the interval crosses only
// where bits 24..55 of low are all ones, once in 2^32 renormalisations: a cheap necessary test for the whole wavefront,
// the exact one behind it.  (nm and sm are applied one after the other: with `& (nm & sm)` the compiler folds sm's select into
// nm before this is inlined, and every caller keeps nm in a register it otherwise does not need.)
__device__ __forceinline__ void rc_clamp_mask(u64 low, u32& range, u32 nm) {
    const u32 lo = (u32)low, hi = (u32)(low >> 32);
    if (__any((hi | 0xFF000000u) == 0xFFFFFFFFu)) {
        const u32 thi = (u32)((low + range) >> 32);
        const u32 sm = ((thi ^ hi) >> 24) ? ~0u : 0u;
        range ^= ((range ^ (~lo & (RC_TOP - 1))) & nm) & sm;                  // (lo | (TOP - 1)) - lo
    }
}
// coder.hpp:74-80 / 93-100, the lane-serial renormalisation; byte() moves one byte: put(low >> 56) in an encoder,
// code = code << 8 | get() in a decoder.  The reference spins forever if the clamp yields range 0; every chain here must
// drain, so a symbol that is not done after RC_GUARD rounds sets err.  (Not unrolled: the guard bounds the trip count, and
// thirteen copies of byte() -- a decoder's refill with its end-of-stream byte loads -- per symbol site are what the
// compiler makes of that.)
template <typename BYTE>
__device__ __forceinline__ void rc_renorm(u64& low, u32& range, u32& err, BYTE&& byte) {
    int guard = 0;
#pragma nounroll
    while (range < RC_TOP) {
        range = rc_clamped(low, range);
        byte();
        range <<= 8;
        low <<= 8;
        if (++guard > RC_GUARD) { err = 1; range = 0xFFFFFFFFu; break; }
    }
}

template <typename SINK>
struct RcEncT {
    u64 low;
    u32 range;
    u32 err;
    __device__ __forceinline__ void init() { low = 0; range = 0xFFFFFFFFu; err = 0; }   // coder.hpp:34-39

    // coder.hpp:66-81
    __device__ __forceinline__ void encode(SINK& s, u32 cum, u32 freq, u32 tot) {
        u32 r = range / tot;
        low += (u64)(u32)(cum * r);
        range = r * freq;
        rc_renorm(low, range, err, [&] { s.put((u8)(low >> 56)); });
    }
    // coder.hpp:52-61
    __device__ __forceinline__ void done(SINK& s) {
        for (int i = 0; i < 8; i++) { s.put((u8)(low >> 56)); low <<= 8; }
    }
};
using RcEnc = RcEncT<ByteSink>;

struct RcDec {
    u64 low, code;
    u32 range;
    u32 err;
    // coder.hpp:41-49
    template <typename SRC>
    __device__ __forceinline__ void init(SRC& s) {
        low = 0; range = 0xFFFFFFFFu; code = 0; err = 0;
        for (int i = 0; i < 8; i++) code = (code << 8) | s.get();
    }
    // coder.hpp:83-86.  code < 2^32 in every well-formed stream; the 64-bit divide keeps corrupt ones defined.
    __device__ __forceinline__ u32 get_freq(u32 tot) {
        range /= tot;
        if (range == 0) { err = 1; range = 1; }
        if ((code >> 32) == 0) return (u32)code / range;
        return (u32)(code / range);
    }
    // coder.hpp:88-102
    template <typename SRC>
    __device__ __forceinline__ void decode(SRC& s, u32 cum, u32 freq) {
        u32 temp = cum * range;
        low += temp;
        code -= temp;
        range *= freq;
        rc_renorm(low, range, err, [&] { code = (code << 8) | s.get(); });
    }
};

// dev_lines.h -- a text read as aligned 16-byte units, a wavefront per SPAN: the device helpers of the passes that count the line
// ends themselves because they have no line index (qmap.hip, pair.hip, pick.hip).
// Spans are laid from the aligned 16-byte unit that holds the text's first byte.  A pass READS whole aligned units: up to 15 bytes in
// front of the text and behind it, inside the units of its first and last byte.
#pragma once
#include "dev_common.h"

namespace textspan {

constexpr u32 ROW = 1024;                      // bytes a wavefront reads with one load instruction (64 lanes x 16)
constexpr u32 SPAN_ROWS = 16;
constexpr u32 SPAN = ROW * SPAN_ROWS;          // 16 KiB: the text a wavefront takes at a time
constexpr u32 BATCH = 4;                       // rows a wavefront loads before it looks at the first
constexpr u32 MAX_WG = 2048;                   // workgroups of a launch; each strides over the tiles of 4 spans

__device__ __forceinline__ u32 wave_incl_add(u32 v, u32 lane) {
#pragma unroll
    for (u32 o = 1; o < 64; o <<= 1) { const u32 t = (u32)__shfl_up((int)v, o, 64); if (lane >= o) v += t; }
    return v;
}
__device__ __forceinline__ u32 wave_sum(u32 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (u32)__shfl_xor((int)v, o, 64);
    return v;
}
// bit 7 of every byte of x that is not zero (exact: no carry leaves a byte)
__device__ __forceinline__ u32 nonzero_bytes(u32 x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; }
// bits 7, 15, 23, 31 -> bits 0 .. 3 (the four partial products land on bits 21 .. 24, no two on one bit)
__device__ __forceinline__ u32 gather_bit7(u32 t) { return (((t >> 7) * 0x00204081u) >> 21) & 0xFu; }
// bit j: byte j of the unit is '\n'
__device__ __forceinline__ u32 newline_mask(uint4 v) {
    const u32 w[4] = { v.x, v.y, v.z, v.w };
    u32 m = 0;
#pragma unroll
    for (u32 i = 0; i < 4; i++) m |= gather_bit7(~nonzero_bytes(w[i] ^ 0x0A0A0A0Au) & 0x80808080u) << (4 * i);
    return m;
}
// bits 4 i .. 4 i + 3 of a 16-bit mask over the unit's bytes -> whole bytes of word i
__device__ __forceinline__ u32 byte_mask(u32 m, u32 i) {
    const u32 keep = ((m >> (4 * i)) & 0xFu) * 0x00204081u;            // bit b -> bits 0 / 8 / 16 / 24 ...
    return (keep & 0x01010101u) * 0xFFu;                               // ... -> whole bytes
}
// The unit of `lane` in the row that starts at text offset rb: *ub = its offset (negative in front of the text), the result
// the mask of its bytes that are text.  EDGE = false: the span lies inside the text, every byte of every unit is text.
template <bool EDGE>
__device__ __forceinline__ u32 unit_mask(i64 rb, i64 n, u32 lane, i64* ub) {
    *ub = rb + 16 * (i64)lane;
    if (!EDGE) return 0xFFFFu;
    if (*ub >= n || *ub + 16 <= 0) return 0u;
    const u32 jlo = *ub < 0 ? (u32)(-*ub) : 0u;
    const u32 jhi = n - *ub < 16 ? (u32)(n - *ub) : 16u;
    return ((1u << jhi) - 1u) & ~((1u << jlo) - 1u);
}
// NB rows from text offset rb0 on: the lane's unit of each (zeros where none of its bytes is text) and the mask of its bytes that are
template <bool EDGE, u32 NB>
__device__ __forceinline__ void load_rows(const u8* fq, i64 n, i64 rb0, u32 lane, uint4 (&v)[NB], u32 (&vm)[NB]) {
#pragma unroll
    for (u32 k = 0; k < NB; k++) {
        i64 ub;
        vm[k] = unit_mask<EDGE>(rb0 + (i64)k * ROW, n, lane, &ub);
        v[k] = make_uint4(0, 0, 0, 0);
        if (vm[k]) v[k] = *reinterpret_cast<const uint4*>(fq + ub);
    }
}
template <bool EDGE>
__device__ __forceinline__ void load_batch(const u8* fq, i64 n, i64 rb0, u32 lane, uint4 (&v)[BATCH], u32 (&vm)[BATCH]) {
    load_rows<EDGE, BATCH>(fq, n, rb0, lane, v, vm);
}

__device__ __forceinline__ u32 below(u32 j) { return (1u << j) - 1u; }          // the bytes in front of byte j (j <= 16)
// bit j: byte j of the unit is pat's byte (pat: one byte four times)
__device__ __forceinline__ u32 eq_mask(const u32 (&w)[4], u32 pat) {
    u32 m = 0;
#pragma unroll
    for (u32 i = 0; i < 4; i++) m |= gather_bit7(~nonzero_bytes(w[i] ^ pat) & 0x80808080u) << (4 * i);
    return m;
}
// the sum of the unit's bytes that m names
__device__ __forceinline__ u32 byte_sum(const u32 (&w)[4], u32 m) {
    u32 s = 0;
#pragma unroll
    for (u32 i = 0; i < 4; i++) s = __builtin_amdgcn_sad_u8(w[i] & byte_mask(m, i), 0u, s);
    return s;
}
// two bits a byte, (byte >> 1) & 3 -- A 0, C 1, T 2, G 3, either case -- byte j at bits 2 j (per word: the four fields land on bits
// 18 .. 25 of the product, no two partial products on one bit)
__device__ __forceinline__ u32 base_codes(const u32 (&w)[4]) {
    u32 c = 0;
#pragma unroll
    for (u32 i = 0; i < 4; i++) c |= (((((w[i] >> 1) & 0x03030303u) * 0x00041041u) >> 18) & 0xFFu) << (8 * i);
    return c;
}

// text[off, off + 8) from the aligned 8-byte words that hold it; a word without a byte of the text is not read (zeros)
__device__ __forceinline__ u64 load8(const u8* text, i64 off, u64 n) {
    const uintptr_t t0 = (uintptr_t)text, t1 = t0 + n, p = t0 + (uintptr_t)off, q = p & ~(uintptr_t)7;
    const u32 sh = 8 * (u32)(p & 7);
    u64 lo = 0, hi = 0;
    if (q + 8 > t0 && q < t1) lo = *reinterpret_cast<const u64*>(q);
    if (sh && q + 16 > t0 && q + 8 < t1) hi = *reinterpret_cast<const u64*>(q + 8);
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

}  // namespace textspan

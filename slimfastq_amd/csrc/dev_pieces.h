// dev_pieces.h -- what the passes that cut a record's lines 2 and 4 share (trim.hip, ovl.hip): the record's pieces for pick.hip's copy,
// and a report's counters summed over a wavefront before one atomic.
#pragma once
#include "dev_common.h"

namespace textspan {

// The record's pieces in order, the non-empty ones after merging: line 1 | bases [s, e) | '\n' line 3 '\n' | qualities [s, e) | the last
// '\n'.  a0 .. a3: where its lines begin, end: where it ends in the text, L: the length of lines 2 and 4.  emit(from, len) per piece.
template <class Emit>
__device__ __forceinline__ void record_pieces(u64 a0, u64 a1, u64 a3, u64 end, u64 L, u64 s, u64 e, Emit emit) {
    const u64 from[5] = { a0, a1 + s, a1 + L, a3 + s, a3 + L };
    const u64 len[5] = { a1 - a0, e - s, a3 - (a1 + L), e - s, end - (a3 + L) };
    const bool join[5] = { false, s == 0, e == L, s == 0, e == L };     // piece i begins where piece i - 1 ends
    u64 cf = from[0], cl = len[0];
#pragma unroll
    for (u32 i = 1; i < 5; i++) {
        if (join[i]) cl += len[i];
        else { if (cl) emit(cf, cl); cf = from[i]; cl = len[i]; }
    }
    if (cl) emit(cf, cl);
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
    u32 lo = (u32)v, hi = (u32)(v >> 32);
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const u32 l2 = (u32)__shfl_xor((int)lo, o, 64), h2 = (u32)__shfl_xor((int)hi, o, 64);
        v = (((u64)hi << 32) | lo) + (((u64)h2 << 32) | l2);
        lo = (u32)v; hi = (u32)(v >> 32);
    }
    return v;
}
__device__ __forceinline__ void add_to(u64* to, u64 v, u32 lane) {
    if (v && !lane) atomicAdd(reinterpret_cast<unsigned long long*>(to), (unsigned long long)v);
}

}  // namespace textspan

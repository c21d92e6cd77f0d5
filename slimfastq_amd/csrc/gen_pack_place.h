// gen_pack_place.h -- k_gen_pack_raw's arithmetic (chains.hip): which lanes take which record, which bytes of a lane's sixteen
// are its record's, where its thirty-two bits of codes land in the chain, and when the dwords they land in are complete.
// Plain C++, so that a host program can run it over hostile line lengths (scratch/host_pack_test.cpp).
//
// A wavefront packs a chain; its records come in chunks of up to 64.  A GROUP of P lanes owns a record, lane p of the group the
// record's bases 16 p .. 16 p + 15: a step of the wavefront takes 64 / P records (the lanes behind the last whole group idle), and
// no lane looks its record up.  P is chosen for the whole chunk from its longest line -- the pieces of sixteen that line has, 64 at
// the most --, so that every line of the chunk fits its group; a chunk with a line of more than 1024 bases runs a record per step,
// 1024 bases per turn.
// The codes of a piece start at bit 2 (first + 16 p) of the chain, first = the bases of the chain before the record: dword d with
// an even shift, and d + 1 for what the shift pushes out.  Both are ORed into a ring of GP_RING dwords (dword D at D % GP_RING;
// several records may share a dword), which starts as zeros; a row of 64 dwords, at a multiple of 64, is stored and zeroed as
// soon as every base below its end has been deposited.  A turn deposits at most 1024 bases from where the last one ended -- 64
// dwords and the one behind them -- on top of at most 63 complete dwords that wait for their row: never more than the ring
// holds, and never more than one row becomes complete in a turn.
#pragma once
#include "dev_common.h"

#define GP_RING 128u         // dwords per wavefront
#define GP_ROW 64u           // dwords per store: one per lane

// the lanes per record for a chunk whose longest line has max_len bases
__device__ __forceinline__ u32 gp_group_lanes(u32 max_len) { const u32 p = (max_len + 15u) >> 4; return p < 1u ? 1u : p > 64u ? 64u : p; }
// x / lanes for x = 0 .. 64 and lanes = 1 .. 64 without an integer division: (x + 0.5) / lanes is at least 1 / 128 away from the
// next whole number, the reciprocal's and the product's rounding errors are below 2^-20 of it
__device__ __forceinline__ u32 gp_div_lanes(u32 x, u32 lanes) { return (u32)(((float)x + 0.5f) * __builtin_amdgcn_rcpf((float)lanes)); }
// byte masks of a piece's four dwords: the first min(rem, 16) of its sixteen bytes (rem = the bases of the line from the piece's first on)
__device__ __forceinline__ u32 gp_valid1(u32 rem8, u32 i) {               // rem8 = 8 rem; dword i
    const u32 t = rem8 > 32u * i ? rem8 - 32u * i : 0u;                   // its valid bits, 32 and more: all
    return rem8 >= 32u * (i + 1u) ? ~0u : (1u << (t & 31u)) - 1u;
}
__device__ __forceinline__ uint4 gp_valid4(u32 rem) {
    const u32 rem8 = 8u * rem;                                            // (a line is far shorter than 2^29)
    return make_uint4(gp_valid1(rem8, 0u), gp_valid1(rem8, 1u), gp_valid1(rem8, 2u), gp_valid1(rem8, 3u));
}

// sixteen codes (two bits each, the first in the low bits) whose first base is base `pos` of the chain
struct GpPlace { u32 d, lo, hi; };                                        // chain dword d gets lo, d + 1 gets hi (0: nothing)
__device__ __forceinline__ GpPlace gp_place(u32 pos, u32 code) {
    GpPlace g;
    const u32 s = 2u * (pos & 15u);
    g.d = pos >> 4;
    g.lo = code << s;
    g.hi = s ? code >> (32u - s) : 0u;
    return g;
}
__device__ __forceinline__ u32 gp_ring_slot(u32 d) { return d & (GP_RING - 1u); }

// the ring's rows: `row` = the first dword not stored yet (a multiple of GP_ROW); next = the chain's first base not deposited yet.
// True when the row at `row` is complete; the caller stores it, zeroes it and moves `row` on by GP_ROW.
__device__ __forceinline__ bool gp_row_ready(u32 row, u32 next) { return row + GP_ROW <= (next >> 4); }
// the dwords left behind the last full row at the chain's end, `bases` in all (fewer than GP_ROW + 1, the last one padded)
__device__ __forceinline__ u32 gp_tail_dwords(u32 row, u32 bases) { return ((bases + 15u) >> 4) - row; }

// ---- the steps of a chunk ---------------------------------------------------------------------------------------------------
// With groups of `lanes` lanes a step takes per = 64 / lanes records: step s0 (a multiple of per) of a chunk of n records takes
// records s0 .. s0 + per - 1, as far as the chunk has them.  Lane `lane` belongs to group sub = lane / lanes and takes, in turn q0
// (0, 1024, .. -- more than one only for lines of more than 1024 bases), the bases of record s0 + sub from q0 + gp_lane_piece on.
#define GP_NO_PIECE 0x80000000u                                           // a lane behind the last whole group: past every line's end
__device__ __forceinline__ u32 gp_lane_piece(u32 lane, u32 sub, u32 lanes, u32 per) { return sub < per ? (lane - sub * lanes) << 4 : GP_NO_PIECE; }
// the last record of the step
__device__ __forceinline__ u32 gp_step_last(u32 s0, u32 n, u32 per) { const u32 e = s0 + per; return (e < n ? e : n) - 1u; }
// the first base of the chain not deposited after turn q0 of a step whose last record ends at base rec_end and has len bases
__device__ __forceinline__ u32 gp_turn_end(u32 rec_end, u32 len, u32 q0) { return q0 + 1024u < len ? rec_end - len + q0 + 1024u : rec_end; }

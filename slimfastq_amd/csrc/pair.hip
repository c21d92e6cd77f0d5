// pair.hip -- paired files: two FASTQ texts interleaved record by record (sfq_interleave, sfq_encode_pairs_host), and an interleaved
// text split into its even records followed by its odd ones (sfq_split_pairs, sfq_ctx_set_pair_split).  Text to text, in front of an
// encode's framing and behind a decode's assembly; like qmap.hip the passes have no line index and count the line ends themselves.
//   1. launch_newline_counts (qmap.hip) and launch_scan_u32 (frame.hip): the line ends in front of every SPAN of a text.
//   2. k_pair_starts: a wavefront per span again; per row one wave scan of the units' '\n' counts numbers every line end, and every
//      fourth one writes the offset behind it: starts[r] = where record r begins.
//   3. k_pair_check (one lane): lines and records of the texts, starts[0] and starts[records], and the rules (kernels.h PairStatus).
//      k_pair_lens: no record of 4 GiB or more; for a split the lengths of the even records, which launch_scan_u32 turns into offa[].
//   4. k_pair_copy, the one copy of both passes: 2 P pieces with contiguous destinations,
//        interleave: piece 2i = A's record i to sA[i] + sB[i], piece 2i + 1 = B's record i to sA[i + 1] + sB[i]
//        split:      piece k < P = record 2k to offa[k], piece P + k = record 2k + 1 to offa[P] + S[2k] - offa[k]
//      none of them stored: a piece's destination and source are two loads from the start arrays.
//      A window of records [r0, r0 + n) split (sfq_split_pairs_range) is the same copy over starts + r0: k_pair_check validates the range
//      and leaves the window's first source byte, its size and its pairs in PairInfo, where the copy reads them (the size is known
//      on the device alone; the host lays the grid over an upper bound).
//   5. k_pair_names (sfq_check_mates, sfq_ctx_set_mate_check): a lane per pair compares the names of two header lines found through
//      the start arrays, sixteen bytes a step.
// The copy is laid out over the OUTPUT, not over the pieces: a wavefront takes a span of 16 KiB of the output (a workgroup four of
// them), a lane an aligned 16-byte unit of it, so a record of 200 KB is copied by as many lanes as 600 records of 350 bytes, and no
// lane or wave walks a long record.  Per span one 64-way search over the destinations (4 steps for 2^23 pieces) finds the piece of
// the span's first byte; the destinations of the 64 pieces from there on sit one per lane (the WINDOW), and a lane finds the piece of
// its unit by a binary search over the lanes (6 shuffles).  A unit that lies inside one piece is two aligned 16-byte loads shifted
// into one store; a unit with a piece border in it takes one such step per piece and merges them by byte masks.  A window that ends
// inside the span (pieces under 260 bytes) is reloaded from the piece it ended in.
// Loads are whole aligned units that hold at least one byte that is copied: up to 15 bytes in front of a text and behind it.  Stores
// are whole units inside the output and single bytes in the (at most two) ragged units at its ends: nothing outside it is written.
// Every kernel after the check returns at once where the status is set, so a refused call writes nothing to the output.
#include "kernels.h"
#include "dev_lines.h"
#include "frame_masks.h"

namespace {
using namespace textspan;

// ---- 2. record starts ----------------------------------------------------------------------------------------------------------
// line: the line ends in front of the span
template <bool EDGE>
__device__ __forceinline__ void starts_span(const u8* fq, i64 n, i64 s0, u64 line, u64* __restrict__ starts, u64 cap, u32 lane) {
    for (u32 r0 = 0; r0 < SPAN_ROWS; r0 += BATCH) {
        uint4 v[BATCH]; u32 vm[BATCH];
        load_batch<EDGE>(fq, n, s0 + (i64)r0 * ROW, lane, v, vm);
#pragma unroll
        for (u32 k = 0; k < BATCH; k++) {
            u32 nl = newline_mask(v[k]) & vm[k];
            const u32 cnt = (u32)__popc(nl);
            const u32 icnt = wave_incl_add(cnt, lane);
            u64 ln = line + (icnt - cnt);                      // the line ends in front of the unit
            line += (u32)__shfl((int)icnt, 63, 64);
            const i64 ub = s0 + (i64)(r0 + k) * ROW + 16 * (i64)lane;
            while (nl) {
                const u32 j = (u32)__ffs((int)nl) - 1;
                nl &= nl - 1;
                ln++;
                if (!(ln & 3) && (ln >> 2) <= cap) starts[ln >> 2] = (u64)(ub + j + 1);
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_pair_starts(const u8* __restrict__ base /* 16-byte aligned */, u32 mis, u64 n, u64 nspans,
                                                     const u64* __restrict__ before, u64* __restrict__ starts, u64 cap) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u8* fq = base + mis;
    for (u64 s = (u64)blockIdx.x * 4 + wave; s < nspans; s += (u64)gridDim.x * 4) {
        const i64 s0 = (i64)(s * SPAN) - (i64)mis;
        if (s0 >= 0 && s0 + (i64)SPAN <= (i64)n) starts_span<false>(fq, (i64)n, s0, before[s], starts, cap, lane);
        else starts_span<true>(fq, (i64)n, s0, before[s], starts, cap, lane);
    }
}

// ---- 3. the rules --------------------------------------------------------------------------------------------------------------
struct CheckText { const u64* line_ends; const u8* last; u64 n; u64* starts; };       // line_ends: the scan's last entry; last: the text's last byte
// Also what the copy and the name pass work on: P pairs (of pieces, of records), the source offset of the first record that is
// copied, the output's bytes.  A window's (win.on, split only) are known here first; its range and its room are checked here.
__global__ void k_pair_check(PairInfo* info, u32 split, CheckText a, CheckText b, u64 cap, PairWindow win) {
    if (threadIdx.x || blockIdx.x) return;
    u32 st = PAIR_OK;
    const CheckText t[2] = { a, b };
    const u32 nt = split ? 1u : 2u;
    bool fits = true;
    for (u32 i = 0; i < nt; i++) {
        const u64 lines = *t[i].line_ends + (*t[i].last != '\n');      // a text without a final '\n' ends in a line all the same
        const u64 recs = lines >> 2;
        info->lines[i] = lines; info->recs[i] = recs;
        if ((lines & 3) && !st) st = i ? PAIR_LINES_B : PAIR_LINES_A;
        if (recs <= cap) { t[i].starts[0] = 0; t[i].starts[recs] = t[i].n; } else fits = false;
    }
    const u64 recs = info->recs[0];
    if (!st && !split && recs != info->recs[1]) st = PAIR_COUNTS;
    if (!st && !split && *a.last != '\n') st = PAIR_A_END;
    if (!st && split && !win.on && (recs & 1)) st = PAIR_ODD;
    if (!st && win.on && (win.r0 > recs || win.nr > recs - win.r0)) st = PAIR_RANGE;
    if (!st && !fits) st = PAIR_CAP;
    u64 P = split ? recs >> 1 : recs, win0 = 0, nout = split ? a.n : a.n + b.n;
    if (!st && win.on) {
        win0 = a.starts[win.r0]; nout = a.starts[win.r0 + win.nr] - win0; P = win.nr >> 1;
        if (nout > win.out_cap) st = PAIR_ROOM;
    }
    info->pieces = P; info->win0 = win0; info->nout = nout;
    info->mm_first = ~0ull;
    info->status = st;
}
// interleave (lens null): s = A's starts, s2 = B's; split: s = the starts from the first record that is copied on, lens[k] = the
// length of record 2k of those, 0 behind the last
__global__ __launch_bounds__(256) void k_pair_lens(PairInfo* info, const u64* __restrict__ s, const u64* __restrict__ s2, u32* __restrict__ lens, u64 nlens) {
    if (info->status) return;
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 P = info->pieces;
    u64 l0 = 0, l1 = 0;
    if (k < P) {
        if (lens) { l0 = s[2 * k + 1] - s[2 * k]; l1 = s[2 * k + 2] - s[2 * k + 1]; }
        else { l0 = s[k + 1] - s[k]; l1 = s2[k + 1] - s2[k]; }
    }
    if ((l0 | l1) >> 32) info->status = PAIR_LONG;
    if (lens && k < nlens) lens[k] = (u32)l0;
}

// ---- 4. the copy ---------------------------------------------------------------------------------------------------------------
struct PairJob {
    u32 split;
    const u64* s0; const u64* s1;       // interleave: A's starts, B's starts; split: the starts from the first record copied on, offa
    u64 src0, src1;                     // interleave: A, B; split: the text (addresses)
    u64 nout;                           // on the host an upper bound that sizes the grid; in the kernel what k_pair_check found
    u64 base;                           // split: the source offset of the first record copied (k_pair_check; 0 unless a window is cut)
};
// piece k of 2 P: where it goes in the output and the address it comes from; k >= 2 P: the output's end
__device__ __forceinline__ void piece(const PairJob& J, u64 P, u64 k, u64* dst, u64* src) {
    if (k >= 2 * P) { *dst = J.nout; *src = 0; return; }
    if (!J.split) {
        const u64 i = k >> 1, b = J.s1[i];
        if (k & 1) { *dst = J.s0[i + 1] + b; *src = J.src1 + b; }
        else { const u64 a = J.s0[i]; *dst = a + b; *src = J.src0 + a; }
    } else if (k < P) { *dst = J.s1[k]; *src = J.src0 + J.s0[2 * k]; }
    else { const u64 j = k - P; *dst = J.s1[P] + (J.s0[2 * j] - J.base) - J.s1[j]; *src = J.src0 + J.s0[2 * j + 1]; }
}
// the piece that holds output byte key (< nout): 64 probes a step, one per lane
__device__ __forceinline__ u64 find_piece(const PairJob& J, u64 P, u64 key, u32 lane) {
    u64 lo = 0, hi = 2 * P;             // dst(lo) <= key < dst(hi)
    for (;;) {
        const u64 step = hi - lo > 63 ? (hi - lo + 63) / 64 : 1;
        u64 idx = lo + (u64)lane * step, d, s;
        if (idx > hi) idx = hi;
        piece(J, P, idx, &d, &s);
        const u32 c = (u32)__popcll(__ballot(d <= key));        // lane 0 is one of them
        if (step == 1) return lo + c - 1;
        lo += (u64)(c - 1) * step;
        if (lo + step < hi) hi = lo + step;
    }
}
__device__ __forceinline__ u64 shfl64(u64 v, u32 src) {
    return ((u64)(u32)__shfl((int)(u32)(v >> 32), (int)src, 64) << 32) | (u32)__shfl((int)(u32)v, (int)src, 64);
}
// Up to 64 units from aligned output offset pos on, a lane each.  All offsets count from the aligned base of the output, whose bytes
// are [lo_out, hi_out).  d: the lane's window entry, where piece k0 + lane begins; delta: what turns such an offset into that piece's
// source address; rel: d from the window's base on, saturated -- all the search needs.
__device__ __forceinline__ void copy_units(u8* obase, u64 pos, u32 nun, u64 lo_out, u64 hi_out, u64 d, u64 delta, u32 rel, u64 wbase, u32 lane) {
    const u64 u = pos + 16 * (u64)lane;
    const u64 lo_v = u > lo_out ? u : lo_out, hi_v = u + 16 < hi_out ? u + 16 : hi_out;
    const bool active = lane < nun && lo_v < hi_v;
    const u32 ur = active ? (u32)(lo_v - wbase) : 0u;
    u32 j = 0;                                                 // the last entry at or below the unit's first byte (entry 0 is)
#pragma unroll
    for (u32 step = 32; step; step >>= 1) {
        const u32 t = (u32)__shfl((int)rel, (int)(j + step), 64);
        if (t <= ur) j += step;
    }
    u32 o[4] = { 0, 0, 0, 0 };
    u64 a = lo_v;
    bool go = active;
    while (__any(go)) {                                        // (every lane takes part in the shuffles)
        const u32 jj = go ? j : 0u;
        const u64 dn = shfl64(d, jj < 63 ? jj + 1 : 63), dl = shfl64(delta, jj);
        if (go) {
            const u64 b = dn < hi_v ? dn : hi_v;               // bytes [a, b) of the output come from piece jj
            const u64 S = dl + u;                              // where the unit's byte 0 would come from
            const u32 sh = (u32)S & 15u, x0 = (u32)(a - u), x1 = (u32)(b - u);
            const u8* lo_unit = reinterpret_cast<const u8*>(S - sh);
            uint4 L0 = make_uint4(0, 0, 0, 0), L1 = L0;
            if (sh + x0 < 16) L0 = *reinterpret_cast<const uint4*>(lo_unit);           // only units that hold a byte of [a, b)
            if (sh + x1 > 16) L1 = *reinterpret_cast<const uint4*>(lo_unit + 16);
            const u32 W[8] = { L0.x, L0.y, L0.z, L0.w, L1.x, L1.y, L1.z, L1.w };
            const u32 q = sh >> 2, r8 = (sh & 3u) * 8;
            u32 X[5];
#pragma unroll
            for (u32 i = 0; i < 5; i++) X[i] = q == 0 ? W[i] : q == 1 ? W[i + 1] : q == 2 ? W[i + 2] : W[i + 3];
            const u32 m = ((1u << x1) - 1u) & ~((1u << x0) - 1u);
#pragma unroll
            for (u32 i = 0; i < 4; i++) {
                const u32 w = (u32)((((u64)X[i + 1] << 32) | X[i]) >> r8), keep = byte_mask(m, i);
                o[i] = (w & keep) | (o[i] & ~keep);
            }
            a = b; j++;
            go = a < hi_v;
        }
    }
    if (!active) return;
    if (hi_v - lo_v == 16) *reinterpret_cast<uint4*>(obase + u) = make_uint4(o[0], o[1], o[2], o[3]);
    else {                                                     // a ragged unit at an end of the output: its own bytes alone
        for (u64 x = lo_v; x < hi_v; x++) { const u32 i = (u32)(x - u); obase[x] = (u8)(o[i >> 2] >> (8 * (i & 3))); }
    }
}
// nspans: laid over J.nout as the host knows it, an upper bound where a window is cut; the real end is k_pair_check's
__global__ __launch_bounds__(256) void k_pair_copy(PairJob J, PairInfo* info, u8* obase /* 16-byte aligned */, u32 mis /* the output starts at obase + mis */, u64 nspans) {
    if (info->status) return;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 P = info->pieces;
    J.nout = info->nout; J.base = info->win0;
    const u64 lo_out = mis, hi_out = (u64)mis + J.nout;
    const u64 end_all = (hi_out + 15) & ~15ull;
    if (J.split && !blockIdx.x && !threadIdx.x) info->split = J.s1[P];
    for (u64 s = (u64)blockIdx.x * 4 + wave; s < nspans; s += (u64)gridDim.x * 4) {
        u64 pos = s * SPAN;
        if (pos >= end_all) return;                             // (a window's output ends in front of its bound)
        const u64 end = pos + SPAN < end_all ? pos + SPAN : end_all;
        u64 k0 = find_piece(J, P, (pos > lo_out ? pos : lo_out) - mis, lane);
        while (pos < end) {
            // the window: piece k0 holds pos
            u64 d, src;
            piece(J, P, k0 + lane, &d, &src);
            d += mis;
            const u64 delta = src - d;
            const u32 rel = d <= pos ? 0u : d - pos > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)(d - pos);
            const u64 wbase = pos;
            const bool last = k0 + 63 >= 2 * P;                 // the window reaches the output's end
            const u64 lim = last ? end : shfl64(d, 63);         // the window's pieces cover the bytes below
            for (;;) {
                const u64 room = (lim < end ? lim : end) - pos;
                const u32 nun = room >= ROW ? 64u : (u32)(room >> 4);
                if (!nun) return;                               // (cannot be: a piece has four line ends, so a fresh window covers 15 units)
                copy_units(obase, pos, nun, lo_out, hi_out, d, delta, rel, wbase, lane);
                pos += 16ull * nun;
                if (pos >= end || pos + ROW > lim) break;
            }
            if (pos < end) k0 += (u64)__popcll(__ballot(d <= (pos > lo_out ? pos : lo_out))) - 1;
        }
    }
}

// ---- 5. mate names -------------------------------------------------------------------------------------------------------------
// A lane takes a pair and walks its two header lines sixteen bytes at a time, both from the line's first byte on: a side's sixteen
// bytes are two aligned units shifted into one (the upper unit stays for the next step, so a step is one load a side), their
// delimiters -- ' ', '\t', '\n', the text's end -- one 16-bit mask (frame_masks.h), the bytes that differ between the sides another.
// The walk keeps per side where its first delimiter is and the two bytes in front of it (a "/1" or "/2"), and for both where the first
// event is: a byte that differs or a side's delimiter.  The rule (slimfastq_amd.h) is then arithmetic on those five numbers.  The
// line's first byte is no part of a name: it counts as a delimiter only where it is a line end, and as equal otherwise.
constexpr u32 NAMES_MAX_WG = 4096;
struct NameSide {
    u64 line, left;         // the address of the line's first byte, the text's bytes from there on (at least one)
    uint4 carry;            // the aligned unit behind the one the last step began in
    u32 prev;               // the last four bytes of the last step
    u64 len; u32 tail; bool done;      // the first delimiter's offset in the line, the two bytes in front of it
};
// the sixteen bytes at pos of the line -> X, the mask of its delimiters -> the result.  Loads are aligned units that hold a byte of the text.
__device__ __forceinline__ u32 name_step(NameSide& s, u64 pos, u32 (&X)[4]) {
    const u64 S = s.line + pos, rem = s.left - pos;            // rem > 0: a text's end is a delimiter, and the walk ends at one
    const u32 sh = (u32)S & 15u;
    const u8* unit = reinterpret_cast<const u8*>(S - sh);
    uint4 L0 = s.carry, L1 = make_uint4(0, 0, 0, 0);
    if (!pos || !sh) L0 = *reinterpret_cast<const uint4*>(unit);
    if (sh && rem > 16 - sh) L1 = *reinterpret_cast<const uint4*>(unit + 16);
    s.carry = L1;
    const u32 W[8] = { L0.x, L0.y, L0.z, L0.w, L1.x, L1.y, L1.z, L1.w };
    const u32 q = sh >> 2, r8 = (sh & 3u) * 8;
    u32 Y[5];
#pragma unroll
    for (u32 i = 0; i < 5; i++) Y[i] = q == 0 ? W[i] : q == 1 ? W[i + 1] : q == 2 ? W[i + 2] : W[i + 3];
#pragma unroll
    for (u32 i = 0; i < 4; i++) X[i] = (u32)((((u64)Y[i + 1] << 32) | Y[i]) >> r8);
    if (!pos && (X[0] & 0xFFu) != 0x0Au) X[0] = (X[0] & ~0xFFu) | 0x40u;       // the line's first byte: '@' to both sides
    u32 f[4];
#pragma unroll
    for (u32 i = 0; i < 4; i++) {
        const TextDword d(X[i]);
        f[i] = ne_flags(d, 0x0a0a0a0au) & ne_flags(d, 0x20202020u) & ne_flags(d, 0x09090909u);      // 0x80: no delimiter
    }
    const u32 valid = rem < 16 ? (u32)rem : 16u;
    return (~gather16<7>(f[0], f[1], f[2], f[3]) | (0xFFFFu << valid)) & 0xFFFFu;
}
// bytes j - 2 and j - 1 of a step (j < 16), prev: the four bytes in front of it
__device__ __forceinline__ u32 two_before(u32 prev, const u32 (&X)[4], u32 j) {
    const u32 q = (j + 2) >> 2, r8 = ((j + 2) & 3u) * 8;
    const u32 lo = q == 0 ? prev : q == 1 ? X[0] : q == 2 ? X[1] : q == 3 ? X[2] : X[3];
    const u32 hi = q == 0 ? X[0] : q == 1 ? X[1] : q == 2 ? X[2] : X[3];     // (q == 4: both bytes lie in lo)
    return (u32)((((u64)hi << 32) | lo) >> r8) & 0xFFFFu;
}
__device__ __forceinline__ void name_end(NameSide& s, u64 pos, u32 dm, const u32 (&X)[4]) {
    if (!s.done && dm) {
        const u32 j = (u32)__ffs((int)dm) - 1;
        s.len = pos + j; s.tail = two_before(s.prev, X, j); s.done = true;
    }
    s.prev = X[3];
}
// a name's length from its line's: without the first byte, without a "/1" or "/2" at its end
__device__ __forceinline__ u64 name_bytes(const NameSide& s) {
    const u64 l = s.len ? s.len - 1 : 0;
    return l >= 2 && (s.tail == 0x312Fu || s.tail == 0x322Fu) ? l - 2 : l;
}
__device__ __forceinline__ bool names_differ(u64 la, u64 na, u64 lb, u64 nb) {
    NameSide A{ la, na, make_uint4(0, 0, 0, 0), 0, 0, 0, false }, B{ lb, nb, make_uint4(0, 0, 0, 0), 0, 0, 0, false };
    u64 first = 0; bool seen = false;                          // the first event's offset in the lines
    for (u64 pos = 0; !(A.done && B.done); pos += 16) {
        u32 XA[4] = { 0, 0, 0, 0 }, XB[4] = { 0, 0, 0, 0 }, dA = 0, dB = 0;
        if (!A.done) dA = name_step(A, pos, XA);
        if (!B.done) dB = name_step(B, pos, XB);
        if (!seen) {                                           // (neither side is done yet: a side's end is an event)
            const u32 ev = dA | dB | gather16<7>(nonzero_bytes(XA[0] ^ XB[0]), nonzero_bytes(XA[1] ^ XB[1]), nonzero_bytes(XA[2] ^ XB[2]), nonzero_bytes(XA[3] ^ XB[3]));
            if (ev) { first = pos + (u32)__ffs((int)ev) - 1; seen = true; }
        }
        name_end(A, pos, dA, XA);
        name_end(B, pos, dB, XB);
    }
    const u64 ea = name_bytes(A), eb = name_bytes(B), same = first ? first - 1 : 0;      // name bytes in front of the first event
    return ea != eb || same < ea;
}
// Pair i: the lines at sa[i * stride] of text ta and sb[i * stride] of tb (addresses; na, nb: the texts' bytes).  A wavefront takes
// 64 pairs at a time; what it found goes out in one atomic add and one atomic min per wavefront.
__global__ __launch_bounds__(256) void k_pair_names(PairInfo* info, const u64* __restrict__ sa, const u64* __restrict__ sb, u32 stride,
                                                    u64 ta, u64 na, u64 tb, u64 nb) {
    if (info->status) return;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 P = info->pieces;
    u64 count = 0, first = ~0ull;
    for (u64 i0 = ((u64)blockIdx.x * 4 + wave) * 64; i0 < P; i0 += (u64)gridDim.x * 256) {
        const u64 i = i0 + lane;
        bool bad = false;
        if (i < P) {
            const u64 oa = sa[i * stride], ob = sb[i * stride];
            bad = names_differ(ta + oa, na - oa, tb + ob, nb - ob);
        }
        const u64 m = __ballot(bad);
        if (m) { count += (u64)__popcll(m); if (first == ~0ull) first = i0 + (u32)__ffsll((long long)m) - 1; }
    }
    if (count && !lane) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&info->mm_count), (unsigned long long)count);
        atomicMin(reinterpret_cast<unsigned long long*>(&info->mm_first), (unsigned long long)first);
    }
}
// behind it (the kernel boundary orders them): where the first such pair's lines are
__global__ void k_pair_names_first(PairInfo* info, const u64* __restrict__ sa, const u64* __restrict__ sb, u32 stride) {
    if (threadIdx.x || blockIdx.x || info->status || !info->mm_count) return;
    const u64 i = info->mm_first;
    info->mm_off[0] = sa[i * stride]; info->mm_off[1] = sb[i * stride];
}

void starts_of(const PairText& t, u64 cap, hipStream_t st) {
    const QmapScratch q = qmap_scratch(t.d, t.n);
    const u32 mis = (u32)((uintptr_t)t.d & 15);
    u32* cnt = reinterpret_cast<u32*>(t.scratch + q.cnt_off);
    u64* before = reinterpret_cast<u64*>(t.scratch + q.before_off);
    const u64 tiles = (q.nspans + 3) / 4;
    launch_newline_counts(t.d, t.n, cnt, st);
    launch_scan_u32(cnt, before, q.nspans, reinterpret_cast<u64*>(t.scratch + q.tmp_off), st);
    hipLaunchKernelGGL(k_pair_starts, dim3((u32)(tiles < MAX_WG ? tiles : MAX_WG)), dim3(256), 0, st, t.d - mis, mis, t.n, q.nspans, (const u64*)before, t.starts, cap);
}
CheckText check_of(const PairText& t) {
    const QmapScratch q = qmap_scratch(t.d, t.n);
    return CheckText{ reinterpret_cast<const u64*>(t.scratch + q.before_off) + q.nspans, t.d + t.n - 1, t.n, t.starts };
}
// J.nout: at least the output's bytes
void launch_copy(const PairJob& J, u8* out, PairInfo* info, hipStream_t st) {
    const u32 mis = (u32)((uintptr_t)out & 15);
    const u64 nspans = (mis + J.nout + SPAN - 1) / SPAN, tiles = nspans ? (nspans + 3) / 4 : 1;
    hipLaunchKernelGGL(k_pair_copy, dim3((u32)(tiles < MAX_WG ? tiles : MAX_WG)), dim3(256), 0, st, J, info, out - mis, mis, nspans);
}
// pairs: at least the pairs there are; sb = sa + 1 and stride 2 for the records of one text
void launch_names(const u64* sa, const u64* sb, u32 stride, const PairText& a, const PairText& b, u64 pairs, PairInfo* info, hipStream_t st) {
    const u64 wg = (pairs + 255) / 256;
    hipLaunchKernelGGL(k_pair_names, dim3((u32)(wg < NAMES_MAX_WG ? (wg ? wg : 1) : NAMES_MAX_WG)), dim3(256), 0, st, info, sa, sb, stride,
                       (u64)(uintptr_t)a.d, a.n, (u64)(uintptr_t)b.d, b.n);
    hipLaunchKernelGGL(k_pair_names_first, dim3(1), dim3(64), 0, st, info, sa, sb, stride);
}
const PairWindow NO_WINDOW{ 0, 0, 0, 0, 0 };

}  // namespace

void launch_pair_interleave(const PairText& a, const PairText& b, u64 cap, bool names, u8* out, PairInfo* info, hipStream_t st) {
    starts_of(a, cap, st);
    starts_of(b, cap, st);
    hipLaunchKernelGGL(k_pair_check, dim3(1), dim3(64), 0, st, info, 0u, check_of(a), check_of(b), cap, NO_WINDOW);
    if (names) launch_names(a.starts, b.starts, 1, a, b, cap, info, st);
    hipLaunchKernelGGL(k_pair_lens, dim3((u32)((cap + 255) / 256)), dim3(256), 0, st, info, (const u64*)a.starts, (const u64*)b.starts, (u32*)nullptr, (u64)0);
    launch_copy(PairJob{ 0u, a.starts, b.starts, (u64)(uintptr_t)a.d, (u64)(uintptr_t)b.d, a.n + b.n, 0 }, out, info, st);
}

void launch_pair_split(const PairText& t, u64 cap, const PairWindow& win, u32* lens, u64* offa, u64* scan_tmp, u8* out, PairInfo* info, hipStream_t st) {
    // a window: the lengths and their scan cover its even records alone, the copy's grid what the output can hold of the text
    const u64 all = cap / 2 + 1, nlens = win.on && win.nr / 2 + 1 < all ? win.nr / 2 + 1 : all;
    const u64* s = t.starts + (win.on && win.r0 <= cap ? win.r0 : 0);         // (behind cap: the check refuses, nothing reads it)
    starts_of(t, cap, st);
    hipLaunchKernelGGL(k_pair_check, dim3(1), dim3(64), 0, st, info, 1u, check_of(t), check_of(t), cap, win);
    hipLaunchKernelGGL(k_pair_lens, dim3((u32)((nlens + 255) / 256)), dim3(256), 0, st, info, s, (const u64*)nullptr, lens, nlens);
    launch_scan_u32(lens, offa, nlens, scan_tmp, st);
    launch_copy(PairJob{ 1u, s, offa, (u64)(uintptr_t)t.d, 0, win.on && win.out_cap < t.n ? win.out_cap : t.n, 0 }, out, info, st);
}

void launch_pair_names(const PairText& a, const PairText& b, u64 cap, PairInfo* info, hipStream_t st) {
    starts_of(a, cap, st);
    if (b.d) starts_of(b, cap, st);
    hipLaunchKernelGGL(k_pair_check, dim3(1), dim3(64), 0, st, info, b.d ? 0u : 1u, check_of(a), check_of(b.d ? b : a), cap, NO_WINDOW);
    if (b.d) launch_names(a.starts, b.starts, 1, a, b, cap, info, st);
    else launch_names(a.starts, a.starts + 1, 2, a, a, cap / 2 + 1, info, st);
}

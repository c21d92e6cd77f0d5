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
__global__ void k_pair_check(PairInfo* info, u32 split, CheckText a, CheckText b, u64 cap) {
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
    if (!st && !split && info->recs[0] != info->recs[1]) st = PAIR_COUNTS;
    if (!st && !split && *a.last != '\n') st = PAIR_A_END;
    if (!st && split && (info->recs[0] & 1)) st = PAIR_ODD;
    if (!st && !fits) st = PAIR_CAP;
    info->status = st;
}
// interleave (lens null): s = A's starts, s2 = B's; split: s = the text's starts, lens[k] = the length of record 2k, 0 behind the last
__global__ __launch_bounds__(256) void k_pair_lens(PairInfo* info, const u64* __restrict__ s, const u64* __restrict__ s2, u32* __restrict__ lens, u64 nlens) {
    if (info->status) return;
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 P = lens ? info->recs[0] >> 1 : info->recs[0];
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
    const u64* s0; const u64* s1;       // interleave: A's starts, B's starts; split: the text's starts, offa
    u64 src0, src1;                     // interleave: A, B; split: the text (addresses)
    u64 nout;
};
// piece k of 2 P: where it goes in the output and the address it comes from; k >= 2 P: the output's end
__device__ __forceinline__ void piece(const PairJob& J, u64 P, u64 k, u64* dst, u64* src) {
    if (k >= 2 * P) { *dst = J.nout; *src = 0; return; }
    if (!J.split) {
        const u64 i = k >> 1, b = J.s1[i];
        if (k & 1) { *dst = J.s0[i + 1] + b; *src = J.src1 + b; }
        else { const u64 a = J.s0[i]; *dst = a + b; *src = J.src0 + a; }
    } else if (k < P) { *dst = J.s1[k]; *src = J.src0 + J.s0[2 * k]; }
    else { const u64 j = k - P; *dst = J.s1[P] + J.s0[2 * j] - J.s1[j]; *src = J.src0 + J.s0[2 * j + 1]; }
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
__global__ __launch_bounds__(256) void k_pair_copy(PairJob J, PairInfo* info, u8* obase /* 16-byte aligned */, u32 mis /* the output starts at obase + mis */, u64 nspans) {
    if (info->status) return;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 P = J.split ? info->recs[0] >> 1 : info->recs[0];
    const u64 lo_out = mis, hi_out = (u64)mis + J.nout;
    if (J.split && !blockIdx.x && !threadIdx.x) info->split = J.s1[P];
    for (u64 s = (u64)blockIdx.x * 4 + wave; s < nspans; s += (u64)gridDim.x * 4) {
        u64 pos = s * SPAN;
        const u64 end_all = (hi_out + 15) & ~15ull, end = pos + SPAN < end_all ? pos + SPAN : end_all;
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
void launch_copy(const PairJob& J, u8* out, PairInfo* info, hipStream_t st) {
    const u32 mis = (u32)((uintptr_t)out & 15);
    const u64 nspans = (mis + J.nout + SPAN - 1) / SPAN, tiles = (nspans + 3) / 4;
    hipLaunchKernelGGL(k_pair_copy, dim3((u32)(tiles < MAX_WG ? tiles : MAX_WG)), dim3(256), 0, st, J, info, out - mis, mis, nspans);
}

}  // namespace

void launch_pair_interleave(const PairText& a, const PairText& b, u64 cap, u8* out, PairInfo* info, hipStream_t st) {
    starts_of(a, cap, st);
    starts_of(b, cap, st);
    hipLaunchKernelGGL(k_pair_check, dim3(1), dim3(64), 0, st, info, 0u, check_of(a), check_of(b), cap);
    hipLaunchKernelGGL(k_pair_lens, dim3((u32)((cap + 255) / 256)), dim3(256), 0, st, info, (const u64*)a.starts, (const u64*)b.starts, (u32*)nullptr, (u64)0);
    launch_copy(PairJob{ 0u, a.starts, b.starts, (u64)(uintptr_t)a.d, (u64)(uintptr_t)b.d, a.n + b.n }, out, info, st);
}

void launch_pair_split(const PairText& t, u64 cap, u32* lens, u64* offa, u64* scan_tmp, u8* out, PairInfo* info, hipStream_t st) {
    const u64 nlens = cap / 2 + 1;
    starts_of(t, cap, st);
    hipLaunchKernelGGL(k_pair_check, dim3(1), dim3(64), 0, st, info, 1u, check_of(t), check_of(t), cap);
    hipLaunchKernelGGL(k_pair_lens, dim3((u32)((nlens + 255) / 256)), dim3(256), 0, st, info, (const u64*)t.starts, (const u64*)nullptr, lens, nlens);
    launch_scan_u32(lens, offa, nlens, scan_tmp, st);
    launch_copy(PairJob{ 1u, t.starts, offa, (u64)(uintptr_t)t.d, 0, t.n }, out, info, st);
}

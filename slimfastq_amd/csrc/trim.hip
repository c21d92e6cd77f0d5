// trim.hip -- trimmed records: every record of a FASTQ text with bytes [s, e) of its base line and of its quality line alone, where s
// and e come from fixed crops, quality cuts from either end, a sliding quality window and a 3' adapter (slimfastq_amd.h "trimmed
// records"; sfq_trim_records, sfq_ctx_set_trim).  Text to text behind a decode's assembly, in the layout of sel.hip:
//   1. launch_line_starts (sel.hip): the line ends in front of every SPAN, and ls[l] = where line l begins, ALL lines.
//   2. k_trim_check (one lane): lines % 4, the arrays' room.  k_trim_lens: a lane per record, lines 2 and 4 equally long (the smallest
//      offender by one atomic min per wavefront), no line of 4 GiB.
//   3. k_trim_terms: the text once more, a wavefront per span, a lane per unit.  Every term is a POSITION in a line: the first byte of a
//      quality line at or above a bound, the last such byte, the first window of the quality line whose sum is too small, the first place
//      of the base line where the adapter matches.  Per unit a term is a 16-bit mask of the bytes where its event happens (a window or
//      an adapter occurrence counts at the byte it ENDS at, so that it reaches at most 31 bytes back: into the two units in front,
//      which come from the lanes below, from a carried pair across rows and from a re-read across a span border); a segment of the
//      unit -- the bytes of one line -- turns its mask's first (last) bit into a line position.  What belongs to one line is combined IN
//      THE WAVEFRONT: per row a segmented min scan over the lanes (a segment begins at a unit with a line end in it; the last-byte term
//      goes in as its complement, so that all are minima), a wave-uniform register carries the open line from row to row, and one
//      atomic min per (line, span, term) reaches the record's entry.  The adapter is compared as two bits a base: mismatches are a
//      popcount of ((x | x >> 1) & 0x55..) | invalid, where invalid marks the bytes that are not ACGTacgt.  The partial overlaps at a
//      base line's end are tried in the unit that holds the line's '\n' alone, the longest first.
//      A term that is off is a template parameter: its instructions are not in the loop.  No lane walks a record.
//   4. k_trim_cut: a lane per record: s, e, the report's counts (kept in registers over many records, one wave sum and atomic per
//      wavefront and counter),
//      the number of the record's non-empty pieces and the bytes that are left of it.  launch_scan_u32 over either: where the record's
//      pieces go in the piece arrays, and where its bytes go in the output.  k_trim_room (one lane) checks the output's room.
//   5. k_trim_pieces: a lane per record writes its pieces' sources and destinations one behind the other -- only the NON-EMPTY ones,
//      because pick.hip's copy rests on no piece being empty.  A record is line 1 | the kept bases | '\n' line 3 '\n' | the kept
//      qualities | the last '\n'; neighbours merge where s == 0 or e == L, so an untouched record is one piece.  launch_pick_copy copies.
// Loads are whole aligned units that hold at least one byte of text.  Every index into ls[] and the per-record arrays is checked
// against the arrays' room (a text with more records than they were laid out for is found by the check and runs again).
#include "kernels.h"
#include "dev_lines.h"
#include "dev_wave.h"
#include "dev_pieces.h"

namespace {
using namespace textspan;

constexpr u32 NONE = 0xFFFFFFFFu;

// ---- 2. the rules ----------------------------------------------------------------------------------------------------------------
// line_ends: the scan's last entry; last: the text's last byte
__global__ void k_trim_check(TrimInfo* info, const u64* line_ends, const u8* last, u64 n, u64* ls, u64 cap) {
    if (threadIdx.x || blockIdx.x) return;
    const bool open = *last != '\n';                           // a text without a final '\n' ends in a line all the same
    const u64 lines = *line_ends + open;
    const u64 recs = lines >> 2;
    u32 st = TRIM_OK;
    info->lines = lines; info->recs = recs;
    if (lines & 3) st = TRIM_LINES;
    if (!st && recs > cap) st = TRIM_CAP;
    if (!st) { ls[0] = 0; ls[lines] = n + open; }
    info->bad_first = ~0ull;
    info->status = st; info->stop = st; info->copy.status = st;
}
// a lane per record: lines 2 and 4 are equally long, and no line holds 4 GiB
__global__ __launch_bounds__(256) void k_trim_lens(TrimInfo* info, const u64* __restrict__ ls) {
    if (info->stop) return;
    const u32 lane = threadIdx.x & 63;
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    bool bad = false, big = false;
    if (r < info->recs) {
        const u64 a0 = ls[4 * r], a1 = ls[4 * r + 1], a2 = ls[4 * r + 2], a3 = ls[4 * r + 3], a4 = ls[4 * r + 4];
        bad = a2 - a1 != a4 - a3;
        big = ((a1 - a0) | (a2 - a1) | (a3 - a2) | (a4 - a3)) >> 32 != 0;
    }
    if (big) info->toolong = 1;
    const u64 m = __ballot(bad);
    if (m && !lane) atomicMin(reinterpret_cast<unsigned long long*>(&info->bad_first), (unsigned long long)(r + (u32)__ffsll((long long)m) - 1));
    if ((m || __any(big)) && !lane) info->stop = 1;
}

// ---- 3. the terms ----------------------------------------------------------------------------------------------------------------
struct TrimTerms { const u64* ls; u64 lcap; u32* lead; u32* trail; u32* win; u32* ad; TrimJob job; };

// bit j: byte j of the unit is at least thr (1 .. 255), unsigned: the high bits decide, or where they agree the low seven bits' borrow
__device__ __forceinline__ u32 ge_mask(const u32 (&w)[4], u32 thr) {
    if (thr > 255) return 0u;
    const u32 T = thr * 0x01010101u, tl = T & 0x7F7F7F7Fu;
    u32 m = 0;
#pragma unroll
    for (u32 i = 0; i < 4; i++) {
        const u32 x = w[i], d = ((x & 0x7F7F7F7Fu) | 0x80808080u) - tl;
        m |= gather_bit7(((x & ~T) | (~(x ^ T) & d)) & 0x80808080u) << (4 * i);
    }
    return m;
}
// bit j of a 16-bit mask -> bit 2 j
__device__ __forceinline__ u32 spread2(u32 x) {
    x = (x | (x << 8)) & 0x00FF00FFu; x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u; x = (x | (x << 1)) & 0x55555555u;
    return x;
}
// the unit's bytes that are none of ACGTacgt
__device__ __forceinline__ u32 not_acgt(const u32 (&w)[4]) {
    const u32 lw[4] = { w[0] | 0x20202020u, w[1] | 0x20202020u, w[2] | 0x20202020u, w[3] | 0x20202020u };
    return ~(eq_mask(lw, 0x61616161u) | eq_mask(lw, 0x63636363u) | eq_mask(lw, 0x67676767u) | eq_mask(lw, 0x74747474u)) & 0xFFFFu;
}
// the mismatches of the bases in the low bits of W against the adapter's first ones; inv: bit 2 i where base i is no base; keep: the
// low two bits of every base compared
__device__ __forceinline__ u32 mismatches(u64 W, u64 inv, u64 adapter, u64 keep) {
    const u64 x = W ^ adapter;
    return (u32)__popcll((((x | (x >> 1)) & 0x5555555555555555ull) | inv) & keep);
}

// The events of one unit as 16-bit masks: g1 / g2 the bytes at or above the bound of the cut from the front / the back, wh the bytes
// where a quality window ends whose sum is too small, ah the bytes where the adapter's full length ends and matches.
struct Events { u32 g1, g2, wh, ah; };
// What the bytes m of a unit, all of one line of kind `kind`, give: v0 = the first cut position (quality line: the cut from the front;
// base line: the adapter), v1 = the complement of the cut from the back, v2 = the first failing window; NONE where there is none.
// pos0: the line position of the unit's byte 0, mod 2^32.
struct Cuts { u32 v0, v1, v2; };
__device__ __forceinline__ u32 first_at(u32 m, u32 pos0, u32 back) { return m ? pos0 + (u32)__ffs((int)m) - back : NONE; }
template <bool LQ, bool TQ, bool WN, bool AD>
__device__ __forceinline__ Cuts segment(const TrimJob& J, const Events& E, u32 kind, u32 m, u32 pos0) {
    const u32 lead = LQ ? first_at(E.g1 & m, pos0, 1) : NONE, adap = AD ? first_at(E.ah & m, pos0, J.ad_len) : NONE;
    const u32 g2 = E.g2 & m;
    const u32 trail = TQ && g2 ? ~(pos0 + (32u - (u32)__clz((int)g2))) : NONE;
    const u32 win = WN ? first_at(E.wh & m, pos0, J.win_len) : NONE;
    const bool q = kind == 3;
    return Cuts{ q ? lead : kind == 1 ? adap : NONE, q ? trail : NONE, q ? win : NONE };
}
template <bool LQ, bool TQ, bool WN, bool AD>
__device__ __forceinline__ void line_min(const TrimTerms& T, u64 l, u32 v0, u32 v1, u32 v2) {
    if (l >= T.lcap) return;
    const u64 r = l >> 2;
    const u32 kind = (u32)l & 3u;
    if (kind == 3) {
        if (LQ && v0 != NONE) atomicMin(T.lead + r, v0);
        if (TQ && v1 != NONE) atomicMin(T.trail + r, v1);
        if (WN && v2 != NONE) atomicMin(T.win + r, v2);
    } else if (AD && kind == 1 && v0 != NONE) atomicMin(T.ad + r, v0);
}
__device__ __forceinline__ u32 umin(u32 a, u32 b) { return a < b ? a : b; }

// line: the line ends in front of the span
template <bool EDGE, bool LQ, bool TQ, bool WN, bool AD>
__device__ __forceinline__ void trim_span(const u8* fq, i64 n, i64 s0, u64 line, const TrimTerms& T, u32 lane) {
    const TrimJob& J = T.job;
    constexpr bool BACK = WN || AD;                            // the terms that look at the two units in front
    u32 k0 = NONE, k1 = NONE, k2 = NONE;                       // what the span's units so far give line `line`, the open one
    u32 c1[4] = { 0, 0, 0, 0 }, c2[4] = { 0, 0, 0, 0 };        // the unit in front of the row and the one in front of that
    if (BACK) {                                                // the 32 bytes in front of the span, where they are text
        i64 ub;
        const u32 vm = lane < 2 ? unit_mask<true>(s0 - 32, n, lane, &ub) : 0u;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (vm) v = *reinterpret_cast<const uint4*>(fq + ub);
        const u32 w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
        for (u32 i = 0; i < 4; i++) { c2[i] = rl(w[i], 0); c1[i] = rl(w[i], 1); }
    }
    const u64 amask = J.ad_len >= 32 ? ~0ull : (1ull << (2 * J.ad_len)) - 1;
    // (with the window AND the adapter on, a unit's work is too long to be laid out four times over: those kernels take a row at a time)
    constexpr u32 NB = WN && AD ? 1 : BATCH;
    for (u32 r0 = 0; r0 < SPAN_ROWS; r0 += NB) {
        uint4 v[NB]; u32 vm[NB];
        load_rows<EDGE, NB>(fq, n, s0 + (i64)r0 * ROW, lane, v, vm);
#pragma unroll
        for (u32 k = 0; k < NB; k++) {
            const u32 w[4] = { v[k].x, v[k].y, v[k].z, v[k].w };
            const u32 nl = newline_mask(v[k]) & vm[k];
            const u32 cnt = (u32)__popc(nl);
            const u32 icnt = wave_incl_add(cnt, lane);
            const u64 ln = line + (icnt - cnt);                // the line ends in front of the unit: its first byte is line ln's
            const u64 line_next = line + rl(icnt, 63);
            const i64 ub = s0 + (i64)(r0 + k) * ROW + 16 * (i64)lane;
            const u32 pos_first = (u32)((u64)ub - (ln <= T.lcap ? T.ls[ln] : 0));      // the line position of the unit's byte 0
            // ql, bl: the unit's bytes that lie in a quality line, in a base line; endb: the line ends of base lines
            u32 ql = 0, bl = 0, endb = 0;
            {
                u32 rest = nl, at = 0;
                u64 l = ln;
                while (rest) {
                    const u32 j = (u32)__ffs((int)rest) - 1;
                    rest &= rest - 1;
                    const u32 seg = below(j) & ~below(at);
                    if (((u32)l & 3u) == 3) ql |= seg;
                    if (((u32)l & 3u) == 1) { bl |= seg; endb |= 1u << j; }
                    at = j + 1; l++;
                }
                if (((u32)l & 3u) == 3) ql |= 0xFFFFu & ~below(at);
                if (((u32)l & 3u) == 1) bl |= 0xFFFFu & ~below(at);
                ql &= vm[k]; bl &= vm[k];
            }
            Events E{ 0, 0, 0, 0 };
            if (LQ && ql) E.g1 = ge_mask(w, J.lead_thr) & ql;
            if (TQ && ql) E.g2 = ge_mask(w, J.trail_thr) & ql;
            if (BACK) {
                u32 p1[4], p2[4];                              // the unit in front and the one in front of that
#pragma unroll
                for (u32 i = 0; i < 4; i++) {
                    p1[i] = (u32)__shfl_up((int)w[i], 1, 64); p2[i] = (u32)__shfl_up((int)w[i], 2, 64);
                    if (lane == 0) { p1[i] = c1[i]; p2[i] = c2[i]; }
                    if (lane == 1) p2[i] = c1[i];
                    c1[i] = rl(w[i], 63); c2[i] = rl(w[i], 62);
                }
                // c: the bytes of its line in front of byte j
                if (WN && ql) {
                    const u32 tot1 = byte_sum(p1, 0xFFFFu);
                    u32 c = pos_first, run = 0;                // run: the unit's bytes up to byte j
#pragma unroll
                    for (u32 j = 0; j < 16; j++) {
                        run += (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                        c = (nl >> j) & 1u ? 0u : c + 1;
                        if (((ql >> j) & 1u) && c >= J.win_len) {
                            // the window's first byte, counted from the unit's byte 0 (wave-uniform): -31 .. 15
                            const int f = (int)j + 1 - (int)J.win_len;
                            u32 S = run;
                            if (f > 0) S -= byte_sum(w, below((u32)f));
                            else if (f < 0) {
                                if (f > -16) S += byte_sum(p1, 0xFFFFu & ~below((u32)(16 + f)));
                                else { S += tot1; if (f < -16) S += byte_sum(p2, 0xFFFFu & ~below((u32)(32 + f))); }
                            }
                            if (S < J.win_sum) E.wh |= 1u << j;
                        }
                    }
                }
                if (AD && (bl | endb)) {
                    // W: the ad_len bases that end in front of byte j, the first in the lowest bits; V: those that are no bases
                    const u32 code = base_codes(w), inv = spread2(not_acgt(w));
                    u64 W = (((u64)base_codes(p1) << 32) | base_codes(p2)) >> (2 * (32 - J.ad_len));
                    u64 V = (((u64)spread2(not_acgt(p1)) << 32) | spread2(not_acgt(p2))) >> (2 * (32 - J.ad_len));
                    u32 c = pos_first;
#pragma unroll
                    for (u32 j = 0; j < 16; j++) {
                        if ((endb >> j) & 1u) {
                            // (once a record) the base line ends in front of byte j and holds c bytes: the overlaps of fewer than ad_len bases
                            const u64 rec = (ln + (u32)__popc(nl & below(j))) >> 2;
                            for (u32 o = umin(J.ad_len - 1, c); o >= J.ad_min; o--) {
                                const u32 sh = 2 * (J.ad_len - o);
                                if (mismatches(W >> sh, V >> sh, J.adapter, (1ull << (2 * o)) - 1) <= J.ad_mm * o / J.ad_len) {
                                    if (4 * rec + 1 < T.lcap) atomicMin(T.ad + rec, c - o);
                                    break;
                                }
                            }
                        }
                        W = (W >> 2) | ((u64)((code >> (2 * j)) & 3u) << (2 * J.ad_len - 2));
                        V = (V >> 2) | ((u64)((inv >> (2 * j)) & 1u) << (2 * J.ad_len - 2));
                        c = (nl >> j) & 1u ? 0u : c + 1;
                        if (((bl >> j) & 1u) && c >= J.ad_len && mismatches(W, V, J.adapter, amask) <= J.ad_mm) E.ah |= 1u << j;
                    }
                }
            }
            // t: what the unit gives the line that is open behind it; head: the line that ends at its first line end
            const u32 first = nl ? (u32)__ffs((int)nl) - 1 : 16u, last = nl ? 31u - (u32)__clz((int)nl) : 0u;
            const Cuts H = segment<LQ, TQ, WN, AD>(J, E, (u32)ln & 3u, vm[k] & below(first), pos_first);
            const Cuts B = segment<LQ, TQ, WN, AD>(J, E, (u32)(ln + cnt) & 3u, vm[k] & ~below(last + 1), 0u - (last + 1));
            u32 t0 = nl ? B.v0 : H.v0, t1 = nl ? B.v1 : H.v1, t2 = nl ? B.v2 : H.v2;
            const u32 h0 = nl ? H.v0 : NONE, h1 = nl ? H.v1 : NONE, h2 = nl ? H.v2 : NONE;
            if (nl) {
                // lines that begin and end inside the unit
                u32 rest = nl & (nl - 1), at = first;
                u64 l = ln;
                while (rest) {
                    const u32 j = (u32)__ffs((int)rest) - 1;
                    rest &= rest - 1;
                    l++;
                    const Cuts X = segment<LQ, TQ, WN, AD>(J, E, (u32)l & 3u, vm[k] & below(j) & ~below(at + 1), 0u - (at + 1));
                    line_min<LQ, TQ, WN, AD>(T, l, X.v0, X.v1, X.v2);
                    at = j;
                }
            }
            // segmented inclusive min scan: a segment begins at a unit with a line end
            u32 f = nl ? 1u : 0u;
#pragma unroll
            for (u32 o = 1; o < 64; o <<= 1) {
                const u32 tf = (u32)__shfl_up((int)f, o, 64);
                const bool take = lane >= o && !f;
                if (LQ || AD) { const u32 x = (u32)__shfl_up((int)t0, o, 64); if (take) t0 = umin(t0, x); }
                if (TQ) { const u32 x = (u32)__shfl_up((int)t1, o, 64); if (take) t1 = umin(t1, x); }
                if (WN) { const u32 x = (u32)__shfl_up((int)t2, o, 64); if (take) t2 = umin(t2, x); }
                if (take) f = tf;
            }
            u32 q0 = (u32)__shfl_up((int)t0, 1, 64), q1 = (u32)__shfl_up((int)t1, 1, 64), q2 = (u32)__shfl_up((int)t2, 1, 64);
            u32 pf = (u32)__shfl_up((int)f, 1, 64);
            if (!lane) { q0 = NONE; q1 = NONE; q2 = NONE; pf = 0; }
            if (nl)                                            // line ln ends in this unit: one min a term for the span's share of it
                line_min<LQ, TQ, WN, AD>(T, ln, umin(umin(h0, q0), pf ? NONE : k0), umin(umin(h1, q1), pf ? NONE : k1), umin(umin(h2, q2), pf ? NONE : k2));
            const u32 f63 = rl(f, 63), e0 = rl(t0, 63), e1 = rl(t1, 63), e2 = rl(t2, 63);
            k0 = f63 ? e0 : umin(e0, k0); k1 = f63 ? e1 : umin(e1, k1); k2 = f63 ? e2 : umin(e2, k2);
            line = line_next;
        }
    }
    if (!lane) line_min<LQ, TQ, WN, AD>(T, line, k0, k1, k2);  // the line that is open at the span's end
}
template <bool LQ, bool TQ, bool WN, bool AD>
__global__ __launch_bounds__(256) void k_trim_terms(const TrimInfo* info, const u8* __restrict__ base /* 16-byte aligned */, u32 mis, u64 n, u64 nspans,
                                                    const u64* __restrict__ before, TrimTerms T) {
    if (info->stop) return;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u8* fq = base + mis;
    for (u64 s = (u64)blockIdx.x * 4 + wave; s < nspans; s += (u64)gridDim.x * 4) {
        const i64 s0 = (i64)(s * SPAN) - (i64)mis;
        if (s0 >= 0 && s0 + (i64)SPAN <= (i64)n) trim_span<false, LQ, TQ, WN, AD>(fq, (i64)n, s0, before[s], T, lane);
        else trim_span<true, LQ, TQ, WN, AD>(fq, (i64)n, s0, before[s], T, lane);
    }
}

// ---- 4, 5. the cut and the pieces ------------------------------------------------------------------------------------------------
// (record_pieces, wave_sum64, add_to: dev_pieces.h)
// a lane per record, a wavefront many records: the report's counts stay in registers and go out once a wavefront and counter (one
// atomic a wavefront of 64 records, eight counters on one cache line, is what the kernel would otherwise wait for);
// se[r], cnt[r], rlen[r] for every r < cap (0 behind the last record)
__global__ __launch_bounds__(256) void k_trim_cut(TrimInfo* info, TrimJob J, TrimArrays A, u64 n) {
    if (info->stop) return;
    const u32 lane = threadIdx.x & 63;
    const u64 recs = info->recs;
    u32 changed = 0, emptied = 0, ncut[4] = { 0, 0, 0, 0 };
    u64 bases_in = 0, bases_out = 0;
    bool big = false;
    for (u64 r = (u64)blockIdx.x * 256 + threadIdx.x; r < A.cap; r += (u64)gridDim.x * 256) {
        u64 s = 0, e = 0, left = 0;                            // left: the record's bytes in the output
        u32 pieces = 0;
        if (r < recs) {
            const u64 a0 = A.ls[4 * r], a1 = A.ls[4 * r + 1], a2 = A.ls[4 * r + 2], a3 = A.ls[4 * r + 3], a4 = A.ls[4 * r + 4];
            const u64 L = a2 - a1 - 1;
            const u64 a_head = J.head < L ? J.head : L, b_tail = L - (J.tail < L ? J.tail : L);
            u64 a_lead = 0, b_trail = L, b_win = L, b_ad = L;
            if (J.lead_thr) { const u32 x = A.lead[r]; a_lead = x < L ? x : L; }
            if (J.trail_thr) { const u32 x = ~A.trail[r]; b_trail = x < L ? x : L; }
            if (J.win_len) { const u32 x = A.win[r]; b_win = x < L ? x : L; }
            if (J.ad_len) { const u32 x = A.ad[r]; b_ad = x < L ? x : L; }
            s = a_head > a_lead ? a_head : a_lead;
            e = b_tail;
            if (b_trail < e) e = b_trail;
            if (b_win < e) e = b_win;
            if (b_ad < e) e = b_ad;
            if (e < s) e = s;
            if (J.max_len != ~0u && e > s + J.max_len) e = s + J.max_len;
            record_pieces(a0, a1, a3, a4 < n ? a4 : n, L, s, e, [&](u64, u64 len) { pieces++; left += len; });
            big |= left >> 32 != 0;
            changed += s != 0 || e != L; emptied += L > 0 && s == e;
            ncut[0] += a_lead > 0; ncut[1] += b_trail < L; ncut[2] += b_win < L; ncut[3] += b_ad < L;
            bases_in += L; bases_out += e - s;
        }
        A.se[r] = s | (e << 32); A.cnt[r] = pieces; A.rlen[r] = (u32)left;
    }
    if (__any(big) && !lane) { info->toolong = 1; info->stop = 1; }
    add_to(&info->n_changed, wave_sum(changed), lane);
    add_to(&info->n_emptied, wave_sum(emptied), lane);
#pragma unroll
    for (u32 i = 0; i < 4; i++) add_to(&info->n_cut[i], wave_sum(ncut[i]), lane);
    add_to(&info->bases_in, wave_sum64(bases_in), lane);
    add_to(&info->bases_out, wave_sum64(bases_out), lane);
}
// the pieces' sources and destinations, one behind the other
__global__ __launch_bounds__(256) void k_trim_pieces(const TrimInfo* info, TrimArrays A, u64 n) {
    if (info->stop) return;
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= info->recs || r >= A.cap) return;
    const u64 a0 = A.ls[4 * r], a1 = A.ls[4 * r + 1], a2 = A.ls[4 * r + 2], a3 = A.ls[4 * r + 3], a4 = A.ls[4 * r + 4];
    const u64 se = A.se[r];
    u64 p = A.at[r], d = A.rdst[r];
    const u64 room = 5 * A.cap;
    record_pieces(a0, a1, a3, a4 < n ? a4 : n, a2 - a1 - 1, se & 0xFFFFFFFFull, se >> 32, [&](u64 from, u64 len) {
        if (p < room) { A.from[p] = from; A.dst[p] = d; }
        p++; d += len;
    });
}
// behind the scans: what the copy is, and where the smallest unequal record begins
__global__ void k_trim_room(TrimInfo* info, TrimArrays A, u64 out_cap) {
    if (threadIdx.x || blockIdx.x) return;
    if (info->bad_first != ~0ull && !info->status) info->bad_off = A.ls[4 * info->bad_first];
    if (!info->stop) {
        info->copy.r0 = 0; info->copy.pieces = A.at[A.cap]; info->copy.nout = A.rdst[A.cap];
        if (info->copy.nout > out_cap) { info->status = TRIM_ROOM; info->stop = 1; }
    }
    info->copy.status = info->stop;
}

template <bool LQ, bool TQ, bool WN>
void launch_terms(bool ad, dim3 grid, hipStream_t st, const TrimInfo* info, const u8* base, u32 mis, u64 n, u64 nspans, const u64* before, const TrimTerms& T) {
    if (ad) hipLaunchKernelGGL((k_trim_terms<LQ, TQ, WN, true>), grid, dim3(256), 0, st, info, base, mis, n, nspans, before, T);
    else hipLaunchKernelGGL((k_trim_terms<LQ, TQ, WN, false>), grid, dim3(256), 0, st, info, base, mis, n, nspans, before, T);
}
template <bool LQ, bool TQ>
void launch_terms(bool wn, bool ad, dim3 grid, hipStream_t st, const TrimInfo* info, const u8* base, u32 mis, u64 n, u64 nspans, const u64* before, const TrimTerms& T) {
    if (wn) launch_terms<LQ, TQ, true>(ad, grid, st, info, base, mis, n, nspans, before, T);
    else launch_terms<LQ, TQ, false>(ad, grid, st, info, base, mis, n, nspans, before, T);
}

}  // namespace

void launch_trim(const PairText& t, const TrimArrays& A, const TrimJob& job, u8* out, TrimInfo* info, hipStream_t st) {
    const QmapScratch q = qmap_scratch(t.d, t.n);
    const u32 mis = (u32)((uintptr_t)t.d & 15);
    const u64* before = reinterpret_cast<const u64*>(t.scratch + q.before_off);
    const u64 tiles = (q.nspans + 3) / 4;
    const dim3 grid((u32)(tiles < MAX_WG ? tiles : MAX_WG)), per_rec((u32)((A.cap + 255) / 256));
    const u64 lcap = 4 * A.cap;
    launch_line_starts(t, A.ls, lcap, st);
    hipLaunchKernelGGL(k_trim_check, dim3(1), dim3(64), 0, st, info, before + q.nspans, t.d + t.n - 1, t.n, A.ls, A.cap);
    hipLaunchKernelGGL(k_trim_lens, per_rec, dim3(256), 0, st, info, (const u64*)A.ls);
    // the terms that are on: only their instructions run, and only their arrays are set
    const bool lq = job.lead_thr != 0, tq = job.trail_thr != 0, wn = job.win_len != 0, ad = job.ad_len != 0;
    if (lq || tq || wn || ad) {
        if (lq) (void)hipMemsetAsync(A.lead, 0xFF, A.cap * 4, st);
        if (tq) (void)hipMemsetAsync(A.trail, 0xFF, A.cap * 4, st);
        if (wn) (void)hipMemsetAsync(A.win, 0xFF, A.cap * 4, st);
        if (ad) (void)hipMemsetAsync(A.ad, 0xFF, A.cap * 4, st);
        const TrimTerms T{ A.ls, lcap, A.lead, A.trail, A.win, A.ad, job };
        if (lq && tq) launch_terms<true, true>(wn, ad, grid, st, info, t.d - mis, mis, t.n, q.nspans, before, T);
        else if (lq) launch_terms<true, false>(wn, ad, grid, st, info, t.d - mis, mis, t.n, q.nspans, before, T);
        else if (tq) launch_terms<false, true>(wn, ad, grid, st, info, t.d - mis, mis, t.n, q.nspans, before, T);
        else launch_terms<false, false>(wn, ad, grid, st, info, t.d - mis, mis, t.n, q.nspans, before, T);
    }
    hipLaunchKernelGGL(k_trim_cut, dim3(per_rec.x < MAX_WG ? per_rec.x : MAX_WG), dim3(256), 0, st, info, job, A, t.n);
    launch_scan_u32(A.cnt, A.at, A.cap, A.tmp, st);
    launch_scan_u32(A.rlen, A.rdst, A.cap, A.tmp, st);
    hipLaunchKernelGGL(k_trim_room, dim3(1), dim3(64), 0, st, info, A, job.out_cap);
    hipLaunchKernelGGL(k_trim_pieces, per_rec, dim3(256), 0, st, (const TrimInfo*)info, A, t.n);
    launch_pick_copy(A.dst, A.from, t.d, job.out_cap < t.n ? job.out_cap : t.n, out, &info->copy, st);
}

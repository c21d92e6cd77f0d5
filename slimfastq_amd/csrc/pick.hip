// pick.hip -- picked lines: of every record of a FASTQ text one contiguous piece (slimfastq_amd.h "picked lines": FASTA = lines 1 and 2
// with a '>' in front, the names, the base lines, the quality lines), the pieces written one behind the other (sfq_pick_lines,
// sfq_ctx_set_pick).  Text to text behind a decode's assembly, like pair.hip's split, whose layout the pass shares:
//   1. launch_newline_counts (qmap.hip) and launch_scan_u32 (frame.hip): the line ends in front of every SPAN of the text.
//   2. k_pick_starts: a wavefront per span; per row one wave scan of the units' '\n' counts numbers every line end.  The offset
//      behind line end number e is where line e begins; two of a record's four go out: from[r] = where record r's piece begins,
//      to[r] = the offset behind it (kernels.h PickLines).  What no line end gives -- from[0], and to[last] of a text that does not
//      end in one -- is the check's.
//   3. k_pick_check (one lane): lines and records, the range, the start arrays' room.  k_pick_lens: a lane per record of the range,
//      its piece's length (a u32), and for FASTA and NAMES the record's first byte; launch_scan_u32 turns the lengths into dst[].
//      k_pick_room (one lane): the smallest record without its '@', the result's size against the output's room, the mark.
//   4. k_pick_copy: P pieces, piece k = text[from[r0 + k], to[r0 + k]) to dst[k].  pair.hip's copy: laid out over the OUTPUT, a
//      wavefront a span of 16 KiB, a lane an aligned 16-byte unit; one 64-way search per span finds the piece of the span's first byte,
//      the destinations of the 64 pieces from there on sit one per lane (the WINDOW), a unit inside one piece is two aligned loads
//      shifted into one store, a unit with piece borders in it one such step per piece merged by byte masks.
// A piece here may be ONE byte (an empty base line is "\n"), where a pair's piece holds four line ends.  What the copy rests on is
// only that no piece is empty: the piece k0 of a fresh window holds pos, so the window's entry 1 lies behind pos and its entry 63 at
// least 62 bytes further -- a fresh window covers three whole units or reaches the output's end, and the loop always advances.
// Sixteen pieces in a unit are sixteen turns of the unit's merge loop; a window of small pieces is used for the units it covers
// (three, at one byte a piece) and reloaded.  Pieces of 17 bytes and more fill whole rows as in pair.hip.
// FASTA's '>' is written by the copy itself: the unit that holds a piece's first byte sets it in the register it stores.
// Loads are whole aligned units that hold at least one byte that is copied; stores are whole units inside the output and single bytes
// in the ragged units at its ends.  Every kernel after a check returns at once where the status is set: a refused call writes nothing.
#include "kernels.h"
#include "dev_lines.h"

namespace {
using namespace textspan;

// ---- 2. piece ends -------------------------------------------------------------------------------------------------------------
// the line (of its record, 0 .. 3) a piece begins at; it ends where line to_line(what) & 3 of the same record (of the next: QUALS) begins
__host__ __device__ __forceinline__ u32 from_line(u32 what) { return what == PICK_FASTA || what == PICK_NAMES ? 0u : what == PICK_BASES ? 1u : 3u; }
__host__ __device__ __forceinline__ u32 to_line(u32 what) { return what == PICK_FASTA || what == PICK_BASES ? 2u : what == PICK_NAMES ? 1u : 4u; }

// line: the line ends in front of the span
template <bool EDGE>
__device__ __forceinline__ void starts_span(const u8* fq, i64 n, i64 s0, u64 line, const PickLines& L, u32 lane) {
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
                ln++;                                          // line ln begins behind this line end
                const u64 off = (u64)(ub + j + 1);
                if ((ln & 3) == L.fl && (ln >> 2) < L.cap) L.from[ln >> 2] = off + L.skip;
                if (ln >= L.tl && ((ln - L.tl) & 3) == 0 && ((ln - L.tl) >> 2) < L.cap) L.to[(ln - L.tl) >> 2] = off;
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_pick_starts(const u8* __restrict__ base /* 16-byte aligned */, u32 mis, u64 n, u64 nspans,
                                                     const u64* __restrict__ before, PickLines L) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u8* fq = base + mis;
    for (u64 s = (u64)blockIdx.x * 4 + wave; s < nspans; s += (u64)gridDim.x * 4) {
        const i64 s0 = (i64)(s * SPAN) - (i64)mis;
        if (s0 >= 0 && s0 + (i64)SPAN <= (i64)n) starts_span<false>(fq, (i64)n, s0, before[s], L, lane);
        else starts_span<true>(fq, (i64)n, s0, before[s], L, lane);
    }
}

// ---- 3. the rules --------------------------------------------------------------------------------------------------------------
// line_ends: the scan's last entry; last: the text's last byte.  Leaves the range in info: r0, pieces.
__global__ void k_pick_check(PickInfo* info, const u64* line_ends, const u8* last, u64 n, PickLines L, PickJob job) {
    if (threadIdx.x || blockIdx.x) return;
    const u64 lines = *line_ends + (*last != '\n');            // a text without a final '\n' ends in a line all the same
    const u64 recs = lines >> 2;
    u32 st = PICK_OK;
    info->lines = lines; info->recs = recs;
    if (lines & 3) st = PICK_LINES;
    const bool to_end = job.nr == ~0ull;
    if (!st && (to_end ? job.r0 >= recs : (job.r0 > recs || job.nr > recs - job.r0))) st = PICK_RANGE;
    if (!st && recs > L.cap) st = PICK_CAP;
    if (!st) {
        if (!L.fl) L.from[0] = L.skip;
        if (L.tl == 4 && *last != '\n') L.to[recs - 1] = n;
    }
    info->r0 = job.r0; info->pieces = st ? 0 : to_end ? recs - job.r0 : job.nr;
    info->bad_first = ~0ull;
    info->status = st;
}
// lens[k] = the length of piece k, 0 behind the last.  first: the pieces begin with (FASTA) or behind (NAMES) a record's first byte,
// which is then looked at; what was found goes out in one atomic min per wavefront.
__global__ __launch_bounds__(256) void k_pick_lens(PickInfo* info, PickLines L, const u8* __restrict__ text, u32 first, u32* __restrict__ lens, u64 nlens) {
    if (info->status) return;
    const u32 lane = threadIdx.x & 63;
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 P = info->pieces, r = info->r0 + k;
    u64 len = 0;
    bool bad = false;
    if (k < P) {
        const u64 f = L.from[r];
        len = L.to[r] - f;
        if (first) bad = text[f - L.skip] != '@';
    }
    if (len >> 32) info->status = PICK_LONG;
    if (k < nlens) lens[k] = (u32)len;
    const u64 m = __ballot(bad);
    if (m && !lane) atomicMin(reinterpret_cast<unsigned long long*>(&info->bad_first), (unsigned long long)(k - lane + (u32)__ffsll((long long)m) - 1));
}
// behind the scan: what the copy is
__global__ void k_pick_room(PickInfo* info, PickLines L, const u64* __restrict__ dst, u64 out_cap, u64 mark) {
    if (threadIdx.x || blockIdx.x || info->status) return;
    const u64 P = info->pieces;
    info->nout = dst[P];
    info->mark_off = dst[mark < P ? mark : P];
    if (info->bad_first != ~0ull) {
        info->bad_first += info->r0;
        info->bad_off = L.from[info->bad_first] - L.skip;
        info->status = PICK_AT;
    } else if (info->nout > out_cap) info->status = PICK_ROOM;
}

// ---- 4. the copy (pair.hip "the copy", pieces of one byte and more) -----------------------------------------------------------------
struct CopyJob { const u64* dst; const u64* from; u64 src; u64 nout; };    // from: at the range's first record; src: the text (an address)
// piece k of P: where it goes in the output and the address it comes from; k >= P: the output's end
__device__ __forceinline__ void piece(const CopyJob& J, u64 P, u64 k, u64* dst, u64* src) {
    if (k >= P) { *dst = J.nout; *src = 0; return; }
    *dst = J.dst[k]; *src = J.src + J.from[k];
}
// the piece that holds output byte key (< nout): 64 probes a step, one per lane
__device__ __forceinline__ u64 find_piece(const CopyJob& J, u64 P, u64 key, u32 lane) {
    u64 lo = 0, hi = P;                 // dst(lo) <= key < dst(hi)
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
// source address; rel: d from the window's base on, saturated -- all the search needs.  The units lie below the window's last entry,
// so every piece of a unit has its end in the window.  GT: a piece's first byte is stored as '>'.
template <bool GT>
__device__ __forceinline__ void copy_units(u8* obase, u64 pos, u32 nun, u64 lo_out, u64 hi_out, u64 d, u64 delta, u32 rel, u64 wbase, u32 lane) {
    const u64 u = pos + 16 * (u64)lane;
    const u64 lo_v = u > lo_out ? u : lo_out, hi_v = u + 16 < hi_out ? u + 16 : hi_out;
    const bool active = lane < nun && lo_v < hi_v;
    const u32 ur = active ? (u32)(lo_v - wbase) : 0u;
    u32 j = 0, tj = (u32)__shfl((int)rel, 0, 64);              // the last entry at or below the unit's first byte (entry 0 is), its rel
#pragma unroll
    for (u32 step = 32; step; step >>= 1) {
        const u32 t = (u32)__shfl((int)rel, (int)(j + step), 64);
        if (t <= ur) { j += step; tj = t; }
    }
    // head: the piece begins at a.  At the unit's first byte: where entry j lies there -- rel 0 is every entry at or below pos, of which
    // j is the last, so there it takes an entry AT the window's base
    bool head = false;
    if (GT) { const bool at_base = __any(d == wbase); head = tj == ur && (ur || at_base); }       // (every lane takes part in the vote)
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
            if (GT && head) {                                  // (one unit in fourteen, at 150 bases a read)
                const u32 g = 0xFFu << (8 * (x0 & 3u));
#pragma unroll
                for (u32 i = 0; i < 4; i++) if ((x0 >> 2) == i) o[i] = (o[i] & ~g) | (0x3E3E3E3Eu & g);
            }
            a = b; j++;
            head = true;                                       // what follows in the unit begins where a piece begins
            go = a < hi_v;
        }
    }
    if (!active) return;
    if (hi_v - lo_v == 16) *reinterpret_cast<uint4*>(obase + u) = make_uint4(o[0], o[1], o[2], o[3]);
    else {                                                     // a ragged unit at an end of the output: its own bytes alone
        for (u64 x = lo_v; x < hi_v; x++) { const u32 i = (u32)(x - u); obase[x] = (u8)(o[i >> 2] >> (8 * (i & 3))); }
    }
}
// nspans: laid over an upper bound of the output's bytes; the real end is k_pick_room's
template <bool GT>
__global__ __launch_bounds__(256) void k_pick_copy(CopyJob J, PickInfo* info, u8* obase /* 16-byte aligned */, u32 mis /* the output starts at obase + mis */, u64 nspans,
                                                   const u64* shift /* may be null: ... and *shift bytes further */) {
    if (info->status) return;
    if (shift) { const uintptr_t o = (uintptr_t)obase + mis + *shift; obase = reinterpret_cast<u8*>(o & ~(uintptr_t)15); mis = (u32)(o & 15); }
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 P = info->pieces;
    J.nout = info->nout; J.from += info->r0;
    const u64 lo_out = mis, hi_out = (u64)mis + J.nout;
    const u64 end_all = (hi_out + 15) & ~15ull;
    for (u64 s = (u64)blockIdx.x * 4 + wave; s < nspans; s += (u64)gridDim.x * 4) {
        u64 pos = s * SPAN;
        if (pos >= end_all) return;                             // (the output ends in front of its bound)
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
            const bool last = k0 + 63 >= P;                     // the window reaches the output's end
            const u64 lim = last ? end : shfl64(d, 63);         // the window's pieces cover the bytes below
            for (;;) {
                const u64 room = (lim < end ? lim : end) - pos;
                const u32 nun = room >= ROW ? 64u : (u32)(room >> 4);
                if (!nun) return;                               // (cannot be: no piece is empty, so a fresh window covers three units)
                copy_units<GT>(obase, pos, nun, lo_out, hi_out, d, delta, rel, wbase, lane);
                pos += 16ull * nun;
                if (pos >= end || pos + ROW > lim) break;
            }
            if (pos < end) k0 += (u64)__popcll(__ballot(d <= (pos > lo_out ? pos : lo_out))) - 1;
        }
    }
}

PickLines pick_lines_of(u32 what, u64* from, u64* to, u64 cap) {
    return PickLines{ from, to, cap, from_line(what), to_line(what), what == PICK_NAMES ? 1u : 0u };
}

}  // namespace

// the copy's grid: over what the output can hold of the text
static void launch_pick_copy(const u64* dst, const u64* from, const u8* text, u64 bound, u8* out, PickInfo* info, hipStream_t st, bool gt, const u64* shift = nullptr) {
    const u32 omis = (u32)((uintptr_t)out & 15);
    const u64 ospans = ((shift ? 15 : omis) + bound + SPAN - 1) / SPAN, otiles = ospans ? (ospans + 3) / 4 : 1;
    const CopyJob J{ dst, from, (u64)(uintptr_t)text, bound };
    const dim3 grid((u32)(otiles < MAX_WG ? otiles : MAX_WG));
    if (gt) hipLaunchKernelGGL(k_pick_copy<true>, grid, dim3(256), 0, st, J, info, out - omis, omis, ospans, shift);
    else hipLaunchKernelGGL(k_pick_copy<false>, grid, dim3(256), 0, st, J, info, out - omis, omis, ospans, shift);
}
void launch_pick_copy_at(const u64* dst, const u64* from, const u8* text, u64 bound, u8* out, const u64* shift, PickInfo* info, hipStream_t st) {
    launch_pick_copy(dst, from, text, bound, out, info, st, false, shift);
}
void launch_pick_copy(const u64* dst, const u64* from, const u8* text, u64 bound, u8* out, PickInfo* info, hipStream_t st) {
    launch_pick_copy(dst, from, text, bound, out, info, st, false);
}

void launch_pick(const PairText& t, u64* to, u64 cap, const PickJob& job, u32* lens, u64* dst, u64* scan_tmp, u64 nlens, u8* out, PickInfo* info, hipStream_t st) {
    const QmapScratch q = qmap_scratch(t.d, t.n);
    const u32 mis = (u32)((uintptr_t)t.d & 15);
    u32* cnt = reinterpret_cast<u32*>(t.scratch + q.cnt_off);
    u64* before = reinterpret_cast<u64*>(t.scratch + q.before_off);
    const u64 tiles = (q.nspans + 3) / 4;
    const PickLines L = pick_lines_of(job.what, t.starts, to, cap);
    launch_newline_counts(t.d, t.n, cnt, st);
    launch_scan_u32(cnt, before, q.nspans, reinterpret_cast<u64*>(t.scratch + q.tmp_off), st);
    hipLaunchKernelGGL(k_pick_starts, dim3((u32)(tiles < MAX_WG ? tiles : MAX_WG)), dim3(256), 0, st, t.d - mis, mis, t.n, q.nspans, (const u64*)before, L);
    hipLaunchKernelGGL(k_pick_check, dim3(1), dim3(64), 0, st, info, (const u64*)before + q.nspans, t.d + t.n - 1, t.n, L, job);
    const u32 first = job.what == PICK_FASTA || job.what == PICK_NAMES ? 1u : 0u;
    hipLaunchKernelGGL(k_pick_lens, dim3((u32)((nlens + 255) / 256)), dim3(256), 0, st, info, L, t.d, first, lens, nlens);
    launch_scan_u32(lens, dst, nlens, scan_tmp, st);
    hipLaunchKernelGGL(k_pick_room, dim3(1), dim3(64), 0, st, info, L, (const u64*)dst, job.out_cap, job.mark);
    launch_pick_copy(dst, t.starts, t.d, job.out_cap < t.n ? job.out_cap : t.n, out, info, st, job.what == PICK_FASTA);
}

// sel.hip -- selected records: the records of a FASTQ text that pass a filter on their CONTENT (slimfastq_amd.h "selected records":
// the base line's length, its N count, the quality line's mean, a motif in the base line, a reproducible sample), whole and in order
// (sfq_select_records, sfq_ctx_set_select).  Text to text behind a decode's assembly, in the layout of pick.hip, whose copy it uses:
//   1. launch_newline_counts (qmap.hip) and launch_scan_u32 (frame.hip): the line ends in front of every SPAN of the text.
//   2. k_sel_starts: a wavefront per span numbers every line end (pick.hip's step); ls[l] = where line l begins, ALL lines, because a
//      record's verdict needs the lengths of its lines 2 and 4 and the copy its first and last byte.
//   3. k_sel_check (one lane): lines and records, the range, an odd count under pairs, the arrays' room.
//   4. k_sel_terms: the text once more, a wavefront per span, a lane per unit.  Per unit and line: the 'N' / 'n' bytes of a base line,
//      the byte sum of a quality line, the positions where the motif ends.  What belongs to one line is combined IN THE WAVEFRONT: per
//      row a segmented scan over the lanes (a segment begins at a unit with a line end in it), a wave-uniform register carries the open
//      line from row to row, and one atomic add per (line, span) reaches acc[].  A line of 150 bytes lies in one span or two, so the
//      adds are two or three per record, never one per unit or byte.  The motif is compared as two bits a base: a unit's 16 codes
//      are one u32, a 16-bit mask says which bytes are ACGTacgt (a '\n' or an 'N' breaks a window), the two units in front come from
//      the lanes below (a carried pair of registers across rows, a re-read of the 32 bytes in front across a span border), and the
//      window slides over the unit's 16 positions in registers.  A hit in a base line stores 1 to the record's flag (idempotent).
//      A term that is off is a template parameter: its instructions are not in the loop.
//   5. k_sel_verdict: a lane per record (per pair under pairs): the rule, the report's counts (a ballot and popcount per wavefront),
//      keep[] and the kept record's length.  launch_scan_u32 over keep[] numbers the kept records, k_sel_scatter compacts their starts
//      and lengths, launch_scan_u32 over the lengths gives dst[], k_sel_room (one lane) checks the output's room.
//   6. pick.hip's k_pick_copy<false> (launch_pick_copy): the kept records are its pieces.  Its window logic wants one piece at least:
//      where no record is kept k_sel_room leaves SEL_NOTHING in the status the copy reads, and every wavefront of it returns at once
//      (whether a record is kept is known on the device alone, and the call synchronises once).
// Loads are whole aligned units that hold at least one byte of text.  Every index into ls[], acc[], hit[] is checked against the
// arrays' room (a text with more records than they were laid out for is found by the check and runs again).
#include "kernels.h"
#include "dev_lines.h"

namespace {
using namespace textspan;

// ---- 2. line starts --------------------------------------------------------------------------------------------------------------
// line: the line ends in front of the span; ls holds lcap + 1 entries
template <bool EDGE>
__device__ __forceinline__ void sel_starts_span(const u8* fq, i64 n, i64 s0, u64 line, u64* __restrict__ ls, u64 lcap, u32 lane) {
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
                if (ln <= lcap) ls[ln] = (u64)(ub + j + 1);
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_sel_starts(const u8* __restrict__ base /* 16-byte aligned */, u32 mis, u64 n, u64 nspans,
                                                    const u64* __restrict__ before, u64* __restrict__ ls, u64 lcap) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u8* fq = base + mis;
    for (u64 s = (u64)blockIdx.x * 4 + wave; s < nspans; s += (u64)gridDim.x * 4) {
        const i64 s0 = (i64)(s * SPAN) - (i64)mis;
        if (s0 >= 0 && s0 + (i64)SPAN <= (i64)n) sel_starts_span<false>(fq, (i64)n, s0, before[s], ls, lcap, lane);
        else sel_starts_span<true>(fq, (i64)n, s0, before[s], ls, lcap, lane);
    }
}

// ---- 3. the rules ----------------------------------------------------------------------------------------------------------------
// line_ends: the scan's last entry; last: the text's last byte.  Leaves the range in info: r0, nr.
__global__ void k_sel_check(SelInfo* info, const u64* line_ends, const u8* last, u64 n, u64* ls, u64 cap, SelJob job) {
    if (threadIdx.x || blockIdx.x) return;
    const bool open = *last != '\n';                           // a text without a final '\n' ends in a line all the same
    const u64 lines = *line_ends + open;
    const u64 recs = lines >> 2;
    u32 st = SEL_OK;
    info->lines = lines; info->recs = recs;
    if (lines & 3) st = SEL_LINES;
    const bool to_end = job.nr == ~0ull;
    if (!st && (to_end ? job.r0 >= recs : (job.r0 > recs || job.nr > recs - job.r0))) st = SEL_RANGE;
    const u64 nr = st ? 0 : to_end ? recs - job.r0 : job.nr;
    if (!st && job.pairs && (nr & 1)) st = SEL_ODD;
    if (!st && recs > cap) st = SEL_CAP;
    if (!st) { ls[0] = 0; ls[lines] = n + open; }
    info->r0 = job.r0; info->nr = st ? 0 : nr;
    info->status = st; info->copy.status = st;
}

// ---- 4. the terms ----------------------------------------------------------------------------------------------------------------
struct SelTerms { u64* acc; u64 lcap; u8* hit; u64 cap; u64 motif, motif_rev; u32 mlen; };

// what the bytes m of a unit add to line l: the 'N' / 'n' bytes of a base line, the byte sum of a quality line
template <bool WN, bool WQ>
__device__ __forceinline__ u32 line_value(const u32 (&w)[4], u32 nmask, u32 m, u64 l) {
    const u32 kind = (u32)l & 3u;
    if (WN && kind == 1) return (u32)__popc(nmask & m);
    if (WQ && kind == 3) return byte_sum(w, m);
    return 0;
}
__device__ __forceinline__ void line_add(const SelTerms& T, u64 l, u32 x) {
    if (x && l < T.lcap) atomicAdd(reinterpret_cast<unsigned long long*>(T.acc + (l >> 1)), (unsigned long long)x);
}

// line: the line ends in front of the span
template <bool EDGE, bool WN, bool WQ, bool MOT>
__device__ __forceinline__ void terms_span(const u8* fq, i64 n, i64 s0, u64 line, const SelTerms& T, u32 lane) {
    u32 carry = 0;                                             // what the span's units so far add to line `line`, the open one
    u32 c1 = 0, c2 = 0, m1 = 0, m2 = 0;                        // the unit in front of the row and the one in front of that: codes, ACGT masks
    if (MOT) {                                                 // the 32 bytes in front of the span, where they are text
        i64 ub;
        const u32 vm = lane < 2 ? unit_mask<true>(s0 - 32, n, lane, &ub) : 0u;
        u32 c = 0, m = 0;
        if (vm) {
            const uint4 v = *reinterpret_cast<const uint4*>(fq + ub);
            const u32 w[4] = { v.x, v.y, v.z, v.w };
            const u32 lw[4] = { v.x | 0x20202020u, v.y | 0x20202020u, v.z | 0x20202020u, v.w | 0x20202020u };
            c = base_codes(w);
            m = (eq_mask(lw, 0x61616161u) | eq_mask(lw, 0x63636363u) | eq_mask(lw, 0x67676767u) | eq_mask(lw, 0x74747474u)) & vm;
        }
        c2 = (u32)__shfl((int)c, 0, 64); m2 = (u32)__shfl((int)m, 0, 64);
        c1 = (u32)__shfl((int)c, 1, 64); m1 = (u32)__shfl((int)m, 1, 64);
    }
    for (u32 r0 = 0; r0 < SPAN_ROWS; r0 += BATCH) {
        uint4 v[BATCH]; u32 vm[BATCH];
        load_batch<EDGE>(fq, n, s0 + (i64)r0 * ROW, lane, v, vm);
#pragma unroll
        for (u32 k = 0; k < BATCH; k++) {
            const u32 w[4] = { v[k].x, v[k].y, v[k].z, v[k].w };
            const u32 lw[4] = { w[0] | 0x20202020u, w[1] | 0x20202020u, w[2] | 0x20202020u, w[3] | 0x20202020u };
            const u32 nl = newline_mask(v[k]) & vm[k];
            const u32 cnt = (u32)__popc(nl);
            const u32 icnt = wave_incl_add(cnt, lane);
            const u64 ln = line + (icnt - cnt);                // the line ends in front of the unit: its first byte is line ln's
            const u64 line_next = line + (u32)__shfl((int)icnt, 63, 64);
            if (WN || WQ) {
                const u32 nmask = WN ? eq_mask(lw, 0x6E6E6E6Eu) : 0u;
                // t: what the unit adds to the line that is open behind it; head: to the line that ends at its first line end
                u32 t, head = 0;
                if (!nl) t = line_value<WN, WQ>(w, nmask, vm[k], ln);
                else {
                    const u32 first = (u32)__ffs((int)nl) - 1, last = 31u - (u32)__clz((int)nl);
                    head = line_value<WN, WQ>(w, nmask, vm[k] & below(first), ln);
                    t = line_value<WN, WQ>(w, nmask, vm[k] & ~below(last + 1), ln + cnt);
                    // lines that begin and end inside the unit
                    u32 rest = nl & (nl - 1), at = first;
                    u64 l = ln;
                    while (rest) {
                        const u32 j = (u32)__ffs((int)rest) - 1;
                        rest &= rest - 1;
                        l++;
                        line_add(T, l, line_value<WN, WQ>(w, nmask, vm[k] & below(j) & ~below(at + 1), l));
                        at = j;
                    }
                }
                // segmented inclusive scan: a segment begins at a unit with a line end
                u32 f = nl ? 1u : 0u;
#pragma unroll
                for (u32 o = 1; o < 64; o <<= 1) {
                    const u32 tv = (u32)__shfl_up((int)t, o, 64), tf = (u32)__shfl_up((int)f, o, 64);
                    if (lane >= o && !f) { t += tv; f = tf; }
                }
                u32 pt = (u32)__shfl_up((int)t, 1, 64), pf = (u32)__shfl_up((int)f, 1, 64);
                if (!lane) { pt = 0; pf = 0; }
                if (nl) line_add(T, ln, head + pt + (pf ? 0u : carry));        // line ln ends in this unit: one add for the span's share of it
                const u32 t63 = (u32)__shfl((int)t, 63, 64), f63 = (u32)__shfl((int)f, 63, 64);
                carry = t63 + (f63 ? 0u : carry);
            }
            if (MOT) {
                const u32 code = base_codes(w);
                const u32 ok = (eq_mask(lw, 0x61616161u) | eq_mask(lw, 0x63636363u) | eq_mask(lw, 0x67676767u) | eq_mask(lw, 0x74747474u)) & vm[k];
                u32 p1c = (u32)__shfl_up((int)code, 1, 64), p1m = (u32)__shfl_up((int)ok, 1, 64);
                u32 p2c = (u32)__shfl_up((int)code, 2, 64), p2m = (u32)__shfl_up((int)ok, 2, 64);
                if (lane == 0) { p1c = c1; p1m = m1; p2c = c2; p2m = m2; }
                if (lane == 1) { p2c = c1; p2m = m1; }
                c1 = (u32)__shfl((int)code, 63, 64); m1 = (u32)__shfl((int)ok, 63, 64);
                c2 = (u32)__shfl((int)code, 62, 64); m2 = (u32)__shfl((int)ok, 62, 64);
                // bl: the unit's bytes that lie in a base line
                u32 bl;
                if (!nl) bl = ((u32)ln & 3u) == 1 ? 0xFFFFu : 0u;
                else {
                    bl = 0;
                    u32 rest = nl, at = 0;
                    u64 l = ln;
                    while (rest) {
                        const u32 j = (u32)__ffs((int)rest) - 1;
                        rest &= rest - 1;
                        if (((u32)l & 3u) == 1) bl |= below(j) & ~below(at);
                        at = j + 1; l++;
                    }
                    if (((u32)l & 3u) == 1) bl |= 0xFFFFu & ~below(at);
                }
                if (bl & ok) {
                    // W: the mlen bases that end at the position, the first in the lowest bits; run: the ACGT bytes that end there
                    const u64 P = ((u64)p1c << 32) | p2c;
                    u64 W = P >> (2 * (32 - T.mlen));
                    u32 run = (u32)__clz((int)~((p1m << 16) | p2m));
                    u32 hits = 0;
#pragma unroll
                    for (u32 j = 0; j < 16; j++) {
                        W = (W >> 2) | ((u64)((code >> (2 * j)) & 3u) << (2 * T.mlen - 2));
                        run = (ok >> j) & 1u ? run + 1 : 0u;
                        if (run >= T.mlen && (W == T.motif || W == T.motif_rev)) hits |= 1u << j;
                    }
                    hits &= bl;
                    while (hits) {                             // (rare) the record of the position's line
                        const u32 j = (u32)__ffs((int)hits) - 1;
                        hits &= hits - 1;
                        const u64 rec = (ln + (u32)__popc(nl & below(j))) >> 2;
                        if (rec < T.cap) T.hit[rec] = 1;
                    }
                }
            }
            line = line_next;
        }
    }
    if ((WN || WQ) && !lane) line_add(T, line, carry);         // the line that is open at the span's end
}
template <bool WN, bool WQ, bool MOT>
__global__ __launch_bounds__(256) void k_sel_terms(const SelInfo* info, const u8* __restrict__ base /* 16-byte aligned */, u32 mis, u64 n, u64 nspans,
                                                   const u64* __restrict__ before, SelTerms T) {
    if (info->status) return;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u8* fq = base + mis;
    for (u64 s = (u64)blockIdx.x * 4 + wave; s < nspans; s += (u64)gridDim.x * 4) {
        const i64 s0 = (i64)(s * SPAN) - (i64)mis;
        if (s0 >= 0 && s0 + (i64)SPAN <= (i64)n) terms_span<false, WN, WQ, MOT>(fq, (i64)n, s0, before[s], T, lane);
        else terms_span<true, WN, WQ, MOT>(fq, (i64)n, s0, before[s], T, lane);
    }
}

// ---- 5. verdicts, lengths, destinations ------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 sample_hash(u64 seed, u64 i) {
    u64 h = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 27; h *= 0x94D049BB133111EBull;
    h ^= h >> 31;
    return h;
}
// a lane per record, under pairs a lane per pair (G = 2 records); keep[k], rlen[k] for every k < nlens (0 behind the range)
template <u32 G>
__global__ __launch_bounds__(256) void k_sel_verdict(SelInfo* info, SelJob job, SelArrays A, u64 n) {
    if (info->status) return;
    const u32 lane = threadIdx.x & 63;
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 P = info->nr, r0 = info->r0;
    const bool on_len = job.min_len != 0 || job.max_len != ~0u, on_n = job.max_n != ~0u, on_q = job.min_q != 0, on_m = job.motif_len != 0;
    bool ok[G], in[G];
    u64 len[G];
#pragma unroll
    for (u32 g = 0; g < G; g++) {
        const u64 k = t * G + g, r = r0 + k;
        in[g] = k < P;
        bool bad[4] = { false, false, false, false };
        len[g] = 0;
        if (in[g]) {
            const u64 a0 = A.ls[4 * r], a1 = A.ls[4 * r + 1], a2 = A.ls[4 * r + 2], a3 = A.ls[4 * r + 3], a4 = A.ls[4 * r + 4];
            const u64 l2 = a2 - a1 - 1, l4 = a4 - a3 - 1;
            len[g] = (a4 < n ? a4 : n) - a0;
            if (on_len) bad[0] = l2 < job.min_len || l2 > job.max_len;
            if (on_n) bad[1] = A.acc[2 * r] > job.max_n;
            if (on_q) bad[2] = 100 * ((i64)A.acc[2 * r + 1] - (i64)job.qual_base * (i64)l4) < (i64)job.min_q * (i64)l4;
            if (on_m) bad[3] = !A.hit[r];
            if (len[g] >> 32) { info->status = SEL_LONG; info->copy.status = SEL_LONG; }
        }
        ok[g] = !(bad[0] || bad[1] || bad[2] || bad[3]);
        if (job.invert) ok[g] = !ok[g];
#pragma unroll
        for (u32 i = 0; i < 4; i++) {
            const u64 m = __ballot(bad[i]);
            if (m && !lane) atomicAdd(reinterpret_cast<unsigned long long*>(&info->n_fail[i]), (unsigned long long)__popcll(m));
        }
    }
    bool content = ok[0];
    if (G == 2) content = job.pairs == 1 ? ok[0] && ok[G - 1] : ok[0] || ok[G - 1];
    u64 i = job.index_base + r0 + t * G;
    if (G == 2) i >>= 1;
    const bool sampled = !job.sample || (sample_hash(job.seed, i) >> 32) < job.sample;
#pragma unroll
    for (u32 g = 0; g < G; g++) {
        const u64 k = t * G + g;
        const bool keep = in[g] && sampled && content;
        if (k < A.nlens) { A.keep[k] = keep ? 1u : 0u; A.rlen[k] = keep ? (u32)len[g] : 0u; }
    }
}
// the kept records' starts and lengths, one behind the other (lens[] was zeroed)
__global__ __launch_bounds__(256) void k_sel_scatter(const SelInfo* info, SelArrays A) {
    if (info->status) return;
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= info->nr || k >= A.nlens || !A.keep[k]) return;
    const u64 p = A.pos[k];
    A.from[p] = A.ls[4 * (info->r0 + k)];
    A.lens[p] = A.rlen[k];
}
// behind the scans: what the copy is
__global__ void k_sel_room(SelInfo* info, SelArrays A, u64 out_cap) {
    if (threadIdx.x || blockIdx.x || info->status) return;
    const u64 kept = A.pos[A.nlens], nout = A.dst[A.nlens];
    info->copy.r0 = 0; info->copy.pieces = kept; info->copy.nout = nout;
    if (nout > out_cap) { info->status = SEL_ROOM; info->copy.status = SEL_ROOM; }
    else if (!kept) info->copy.status = SEL_NOTHING;
}

template <bool WN, bool WQ>
void launch_terms(bool mot, dim3 grid, hipStream_t st, const SelInfo* info, const u8* base, u32 mis, u64 n, u64 nspans, const u64* before, const SelTerms& T) {
    if (mot) hipLaunchKernelGGL((k_sel_terms<WN, WQ, true>), grid, dim3(256), 0, st, info, base, mis, n, nspans, before, T);
    else hipLaunchKernelGGL((k_sel_terms<WN, WQ, false>), grid, dim3(256), 0, st, info, base, mis, n, nspans, before, T);
}

}  // namespace

void launch_line_starts(const PairText& t, u64* ls, u64 lcap, hipStream_t st) {
    const QmapScratch q = qmap_scratch(t.d, t.n);
    const u32 mis = (u32)((uintptr_t)t.d & 15);
    u32* cnt = reinterpret_cast<u32*>(t.scratch + q.cnt_off);
    u64* before = reinterpret_cast<u64*>(t.scratch + q.before_off);
    const u64 tiles = (q.nspans + 3) / 4;
    launch_newline_counts(t.d, t.n, cnt, st);
    launch_scan_u32(cnt, before, q.nspans, reinterpret_cast<u64*>(t.scratch + q.tmp_off), st);
    hipLaunchKernelGGL(k_sel_starts, dim3((u32)(tiles < MAX_WG ? tiles : MAX_WG)), dim3(256), 0, st, t.d - mis, mis, t.n, q.nspans, (const u64*)before, ls, lcap);
}

void launch_select(const PairText& t, const SelArrays& A, const SelJob& job, u8* out, SelInfo* info, hipStream_t st) {
    const QmapScratch q = qmap_scratch(t.d, t.n);
    const u32 mis = (u32)((uintptr_t)t.d & 15);
    u64* before = reinterpret_cast<u64*>(t.scratch + q.before_off);
    const u64 tiles = (q.nspans + 3) / 4;
    const dim3 grid((u32)(tiles < MAX_WG ? tiles : MAX_WG));
    const u64 lcap = 4 * A.cap;
    launch_line_starts(t, A.ls, lcap, st);
    hipLaunchKernelGGL(k_sel_check, dim3(1), dim3(64), 0, st, info, (const u64*)before + q.nspans, t.d + t.n - 1, t.n, A.ls, A.cap, job);
    // the terms that are on: only their instructions run, and only their arrays are cleared
    const bool wn = job.max_n != ~0u, wq = job.min_q != 0, mot = job.motif_len != 0;
    if (wn || wq || mot) {
        if (wn || wq) (void)hipMemsetAsync(A.acc, 0, 2 * A.cap * 8, st);
        if (mot) (void)hipMemsetAsync(A.hit, 0, A.cap, st);
        const SelTerms T{ A.acc, lcap, A.hit, A.cap, job.motif, job.motif_rev, job.motif_len };
        if (wn && wq) launch_terms<true, true>(mot, grid, st, info, t.d - mis, mis, t.n, q.nspans, before, T);
        else if (wn) launch_terms<true, false>(mot, grid, st, info, t.d - mis, mis, t.n, q.nspans, before, T);
        else if (wq) launch_terms<false, true>(mot, grid, st, info, t.d - mis, mis, t.n, q.nspans, before, T);
        else launch_terms<false, false>(mot, grid, st, info, t.d - mis, mis, t.n, q.nspans, before, T);
    }
    (void)hipMemsetAsync(A.lens, 0, A.nlens * 4, st);
    if (job.pairs) hipLaunchKernelGGL(k_sel_verdict<2>, dim3((u32)(((A.nlens + 1) / 2 + 255) / 256)), dim3(256), 0, st, info, job, A, t.n);
    else hipLaunchKernelGGL(k_sel_verdict<1>, dim3((u32)((A.nlens + 255) / 256)), dim3(256), 0, st, info, job, A, t.n);
    launch_scan_u32(A.keep, A.pos, A.nlens, A.tmp, st);
    hipLaunchKernelGGL(k_sel_scatter, dim3((u32)((A.nlens + 255) / 256)), dim3(256), 0, st, (const SelInfo*)info, A);
    launch_scan_u32(A.lens, A.dst, A.nlens, A.tmp, st);
    hipLaunchKernelGGL(k_sel_room, dim3(1), dim3(64), 0, st, info, A, job.out_cap);
    launch_pick_copy(A.dst, A.from, t.d, job.out_cap < t.n ? job.out_cap : t.n, out, &info->copy, st);
}

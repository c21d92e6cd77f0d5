// ovl.hip -- overlapping mates: for every pair (X, Y) of a range of records the offset d at which a = line 2 of X and b' = the reverse
// complement of line 2 of Y agree best, the insert I = d + Lb, the inserts' histogram, and with `cut` the text with everything behind
// the insert cut off lines 2 and 4 of both mates (slimfastq_amd.h "overlapping mates"; sfq_overlap_pairs, sfq_ctx_set_overlap).  Text
// to text behind a decode's assembly, in the layout of trim.hip:
//   1. launch_line_starts (sel.hip): ls[l] = where line l begins, ALL lines.
//   2. k_ovl_check (one lane): lines % 4, the range, an odd count, the arrays' room.  k_ovl_lens: a lane per record, lines 2 and 4 of
//      the range's records equally long (the smallest offender by one atomic min per wavefront), no line of 4 GiB.
//   3. k_ovl_search, the hot kernel: ONE WAVEFRONT A PAIR (a group of lanes a pair would leave a 2 x 150 pair's ~270 offsets to 16 lanes
//      and 17 rounds; a wavefront takes the default rule's 241 in at most four, and most pairs end in the first).
//      Packing: lane l turns bases 8 l .. 8 l + 7 of a, and of b', into 16 bits of codes -- (byte >> 1) & 3, so A 0, C 1, T 2, G 3,
//      either case, and the complement is the code XOR 2 -- and 16 bits that mark the bytes that are none of ACGTacgt or lie behind the
//      line's end.  The eight bytes come from the one or two aligned 8-byte words that hold them (only words that hold a byte of the
//      text are read); for b' they are the line's bytes counted from its END, byte-swapped.  The halfwords go to LDS, where 32 bases
//      make a u64: 16 words a line, 544 bytes a pair with b's two guard words.
//      Search: the offsets in order of falling overlap, among equal overlaps the larger d first -- rank t is d = D1 - t on the plateau
//      [D0, D1] = [min(0, La - Lb), max(0, La - Lb)] where the overlap is min(La, Lb), and behind it D1 + i, D0 - i, D1 + i + 1, ... whose
//      overlap falls by one every two ranks.  A lane takes a rank, 64 ranks a round: it walks the words of a that its overlap covers,
//      funnel-shifts b' to its offset, and counts popcll((((x | x >> 1) & 0x55..) | invalid) & the overlap's mask).  Because the ranks
//      ARE the order (overlap, d), the winner is the first accepted lane of the first round that has one: a ballot ends the search.  The
//      ranks end where the overlap falls below min_overlap; max_mm and max_mm_pct are looked at once a round, behind the word loop, so
//      a threshold that is off costs nothing in it.  No lane walks a record byte by byte.
//   4. k_ovl_cut: a lane per record: what is left of lines 2 and 4, the report's counts (in registers over many records, one wave sum
//      and atomic per wavefront and counter; the histogram in LDS, one atomic per workgroup and non-empty bin), the record's non-empty
//      pieces and bytes.  launch_scan_u32 over either, k_ovl_room (one lane) checks the output's room.
//   5. k_ovl_pieces: trim.hip's piece layout with s = 0 (dev_pieces.h): an untouched record is one piece.  launch_pick_copy copies.
//   With cut off the pass ends behind k_ovl_cut: nothing is scanned, laid out or copied.
// Every index into ls[] and the per-record arrays is checked against the arrays' room, as in trim.hip.
#include "kernels.h"
#include "dev_lines.h"
#include "dev_wave.h"
#include "dev_pieces.h"

namespace {
using namespace textspan;

constexpr u64 LOW = 0x5555555555555555ull;                     // the low bit of every base
constexpr u32 WORDS = OVL_MAX_LEN / 32;                        // the u64 words of a line's bases
constexpr u32 NHIST = 2 * OVL_MAX_LEN + 1;

// ---- 2. the rules ----------------------------------------------------------------------------------------------------------------
// line_ends: the scan's last entry; last: the text's last byte.  Leaves the range in info: r0, nr.
__global__ void k_ovl_check(OvlInfo* info, const u64* line_ends, const u8* last, u64 n, u64* ls, u64 cap, OvlJob job) {
    if (threadIdx.x || blockIdx.x) return;
    const bool open = *last != '\n';                           // a text without a final '\n' ends in a line all the same
    const u64 lines = *line_ends + open;
    const u64 recs = lines >> 2;
    u32 st = OVL_OK;
    info->lines = lines; info->recs = recs;
    if (lines & 3) st = OVL_LINES;
    const bool to_end = job.nr == ~0ull;
    if (!st && (job.r0 > recs || (!to_end && job.nr > recs - job.r0))) st = OVL_RANGE;
    const u64 nr = st ? 0 : to_end ? recs - job.r0 : job.nr;
    if (!st && (nr & 1)) st = OVL_ODD;
    if (!st && recs > cap) st = OVL_CAP;
    if (!st) { ls[0] = 0; ls[lines] = n + open; }
    info->r0 = job.r0; info->nr = st ? 0 : nr;
    info->bad_first = ~0ull;
    info->status = st; info->stop = st; info->copy.status = st;
}
// a lane per record: lines 2 and 4 of the range's records are equally long, and no line holds 4 GiB
__global__ __launch_bounds__(256) void k_ovl_lens(OvlInfo* info, const u64* __restrict__ ls) {
    if (info->stop) return;
    const u32 lane = threadIdx.x & 63;
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    bool bad = false, big = false;
    if (r < info->recs) {
        const u64 a0 = ls[4 * r], a1 = ls[4 * r + 1], a2 = ls[4 * r + 2], a3 = ls[4 * r + 3], a4 = ls[4 * r + 4];
        bad = a2 - a1 != a4 - a3 && r >= info->r0 && r - info->r0 < info->nr;
        big = ((a1 - a0) | (a2 - a1) | (a3 - a2) | (a4 - a3)) >> 32 != 0;
    }
    if (big) info->toolong = 1;
    const u64 m = __ballot(bad);
    if (m && !lane) atomicMin(reinterpret_cast<unsigned long long*>(&info->bad_first), (unsigned long long)(r + (u32)__ffsll((long long)m) - 1));
    if ((m || __any(big)) && !lane) info->stop = 1;
}

// ---- 3. the search ---------------------------------------------------------------------------------------------------------------
// a pair's bases in LDS: word w of a / av = bases 32 w .. 32 w + 31 of a, two bits a base / bit 2 i where base i is no base; b, bv the
// same of b', word j at index j + 1 between two guard words that hold no base
struct PairBases { u64 a[WORDS], av[WORDS], b[WORDS + 2], bv[WORDS + 2]; };

// (byte >> 1) & 3 of the eight bytes, byte j at bits 2 j (dev_lines.h base_codes, a word at a time)
__device__ __forceinline__ u32 codes8(u64 w) {
    const u32 x[2] = { (u32)w, (u32)(w >> 32) };
    u32 c = 0;
#pragma unroll
    for (u32 i = 0; i < 2; i++) c |= (((((x[i] >> 1) & 0x03030303u) * 0x00041041u) >> 18) & 0xFFu) << (8 * i);
    return c;
}
// bit 2 j: byte j of the eight is one of ACGTacgt
__device__ __forceinline__ u32 bases8(u64 w) {
    const u32 x[2] = { (u32)w | 0x20202020u, (u32)(w >> 32) | 0x20202020u };
    u32 m = 0;
#pragma unroll
    for (u32 i = 0; i < 2; i++) {
        const u32 no = nonzero_bytes(x[i] ^ 0x61616161u) & nonzero_bytes(x[i] ^ 0x63636363u) & nonzero_bytes(x[i] ^ 0x67676767u) & nonzero_bytes(x[i] ^ 0x74747474u);
        m |= gather_bit7(~no & 0x80808080u) << (4 * i);
    }
    m = (m | (m << 4)) & 0x0F0Fu; m = (m | (m << 2)) & 0x3333u; m = (m | (m << 1)) & 0x5555u;
    return m;
}
// the lane's 16 bits of codes and of invalid marks for bases 8 lane .. 8 lane + 7 of a line of L bases that begins at text offset
// `at`; REV: of the line's reverse complement
template <bool REV>
__device__ __forceinline__ void pack8(const u8* text, u64 n, u64 at, u32 L, u32 lane, u32* codes, u32* inv) {
    *codes = 0; *inv = 0x5555u;
    if (8 * lane >= L) return;
    const u32 have = L - 8 * lane < 8 ? L - 8 * lane : 8;
    u64 w = REV ? load8(text, (i64)at + (i64)L - 8 - 8 * (i64)lane, n) : load8(text, (i64)(at + 8 * lane), n);
    if (REV) w = __builtin_bswap64(w);
    const u32 in_line = (1u << (2 * have)) - 1u;               // (have = 8: 0xFFFF)
    *codes = codes8(w) ^ (REV ? 0xAAAAu : 0u);                 // the complement: A <-> T, C <-> G is the code XOR 2
    *inv = 0x5555u & ~(bases8(w) & in_line);
}

// rank t of the search order -> the offset d
__device__ __forceinline__ int rank_offset(u32 t, u32 P, int D0, int D1) {
    if (t < P) return D1 - (int)t;
    const u32 u = t - P, i = (u >> 1) + 1;
    return u & 1 ? D0 - (int)i : D1 + (int)i;
}
// mm(d): the mismatches of a[lo, hi) against b'[lo - d, hi - d), hi > lo
__device__ __forceinline__ u32 offset_mismatches(const PairBases& S, int d, u32 lo, u32 hi) {
    const u32 w0 = lo >> 5, w1 = (hi - 1) >> 5;
    u32 mm = 0;
    for (u32 w = w0; w <= w1; w++) {
        const int s = 32 * (int)w - d;                         // word w of a lies against bases s .. s + 31 of b': -31 .. 511
        const u32 j = (u32)((s >> 5) + 1), r = 2 * ((u32)s & 31u);
        u64 B = S.b[j], V = S.bv[j];
        if (r) { B = (B >> r) | (S.b[j + 1] << (64 - r)); V = (V >> r) | (S.bv[j + 1] << (64 - r)); }
        const u64 x = S.a[w] ^ B;
        u64 keep = ~0ull;
        if (w == w0) keep <<= 2 * (lo & 31u);
        if (w == w1) keep &= ~0ull >> (62 - 2 * ((hi - 1) & 31u));
        mm += (u32)__popcll((((x | (x >> 1)) & LOW) | S.av[w] | V) & keep);
    }
    return mm;
}

__global__ __launch_bounds__(256) void k_ovl_search(const OvlInfo* info, const u8* __restrict__ text, u64 n, OvlJob J, OvlArrays A) {
    if (info->stop) return;
    __shared__ PairBases lds[4];
    const u32 lane = threadIdx.x & 63, wave = rfl(threadIdx.x >> 6);
    PairBases& S = lds[wave];
    if (!lane) { S.b[0] = 0; S.bv[0] = LOW; S.b[WORDS + 1] = 0; S.bv[WORDS + 1] = LOW; }
    const u64 r0 = info->r0, npairs = info->nr >> 1;
    const u64 lcap = 4 * A.cap;
    // (every wavefront of a workgroup runs the same rounds: the barriers are met by all)
    for (u64 k0 = (u64)blockIdx.x * 4; k0 < npairs; k0 += (u64)gridDim.x * 4) {
        const u64 k = k0 + wave, l = 4 * (r0 + 2 * k);         // the pair and its first line
        const bool on = k < npairs && l + 6 <= lcap && k <= A.cap / 2;
        u64 a1 = 0, b1 = 0, La = 0, Lb = 0;
        if (on) { a1 = A.ls[l + 1]; La = A.ls[l + 2] - a1 - 1; b1 = A.ls[l + 5]; Lb = A.ls[l + 6] - b1 - 1; }
        const bool searched = on && La <= OVL_MAX_LEN && Lb <= OVL_MAX_LEN;
        if (searched) {
            u32 c, v;
            pack8<false>(text, n, a1, (u32)La, lane, &c, &v);
            reinterpret_cast<unsigned short*>(S.a)[lane] = (unsigned short)c;
            reinterpret_cast<unsigned short*>(S.av)[lane] = (unsigned short)v;
            pack8<true>(text, n, b1, (u32)Lb, lane, &c, &v);
            reinterpret_cast<unsigned short*>(S.b + 1)[lane] = (unsigned short)c;
            reinterpret_cast<unsigned short*>(S.bv + 1)[lane] = (unsigned short)v;
        }
        __syncthreads();
        if (searched) {
            const u32 la = (u32)La, lb = (u32)Lb, m = la < lb ? la : lb;
            const int D0 = la < lb ? (int)la - (int)lb : 0, D1 = la < lb ? 0 : (int)la - (int)lb;
            const u32 P = (u32)(D1 - D0) + 1;
            const u32 T = m >= J.min_ov ? P + 2 * (m - J.min_ov) : 0;  // the ranks whose overlap is at least min_overlap
            u32 ins = 0, mis = 0;
            for (u32 t0 = 0; t0 < T; t0 += 64) {
                const u32 t = t0 + lane;
                const int d = rank_offset(t, P, D0, D1);
                const u32 lo = d > 0 ? (u32)d : 0u, end = (u32)(d + (int)lb), hi = end < la ? end : la;
                bool ok = false;
                u32 mm = 0;
                if (t < T) {
                    mm = offset_mismatches(S, d, lo, hi);
                    ok = mm <= J.max_mm && 100 * mm <= J.max_pct * (hi - lo);
                }
                const u64 won = __ballot(ok);
                if (won) {
                    const int first = __ffsll((long long)won) - 1;
                    ins = (u32)(__shfl(d, first, 64) + (int)lb);
                    mis = (u32)__shfl((int)mm, first, 64);
                    break;
                }
            }
            if (!lane) { A.ins[k] = ins; A.mm[k] = mis; }
        } else if (on && !lane) { A.ins[k] = OVL_SKIPPED; A.mm[k] = 0; }
        __syncthreads();
    }
}

// ---- 4, 5. the cut and the pieces ------------------------------------------------------------------------------------------------
// a lane per record, a wavefront many records; keep[r], cnt[r], rlen[r] for every r < cap (0 behind the last record)
__global__ __launch_bounds__(256) void k_ovl_cut(OvlInfo* info, OvlJob J, OvlArrays A, u64 n) {
    if (info->stop) return;
    __shared__ u32 hist[NHIST];
    for (u32 i = threadIdx.x; i < NHIST; i += 256) hist[i] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63;
    const u64 recs = info->recs, r0 = info->r0, nr = info->nr;
    u32 pairs = 0, skipped = 0, overlap = 0, ncut = 0;
    u64 bases_in = 0, bases_out = 0, mism = 0;
    bool big = false;
    for (u64 r = (u64)blockIdx.x * 256 + threadIdx.x; r < A.cap; r += (u64)gridDim.x * 256) {
        u64 e = 0, left = 0;                                   // e: what is left of lines 2 and 4; left: the record's bytes in the output
        u32 pieces = 0;
        if (r < recs) {
            const u64 a0 = A.ls[4 * r], a1 = A.ls[4 * r + 1], a2 = A.ls[4 * r + 2], a3 = A.ls[4 * r + 3], a4 = A.ls[4 * r + 4];
            const u64 L = a2 - a1 - 1;
            e = L;
            if (r >= r0 && r - r0 < nr) {
                const u64 k = (r - r0) >> 1;
                const bool first = !((r - r0) & 1);
                const u32 ins = k <= A.cap / 2 ? A.ins[k] : OVL_SKIPPED;
                const bool found = ins != 0 && ins != OVL_SKIPPED;
                const u64 kept = found && ins < L ? ins : L;
                if (first) {                                   // the pair's counts, once
                    pairs++;
                    if (ins == OVL_SKIPPED) skipped++;
                    else {
                        atomicAdd(&hist[ins < NHIST ? ins : 0], 1u);
                        if (found) {
                            const u64 Lb = 4 * r + 6 <= 4 * A.cap ? A.ls[4 * r + 6] - A.ls[4 * r + 5] - 1 : 0;
                            overlap++; mism += A.mm[k];
                            ncut += ins < L || ins < Lb;
                        }
                    }
                }
                if (J.cut) e = kept;
                bases_in += L; bases_out += e;
            }
            record_pieces(a0, a1, a3, a4 < n ? a4 : n, L, 0, e, [&](u64, u64 len) { pieces++; left += len; });
            big |= left >> 32 != 0;
        }
        A.keep[r] = (u32)e; A.cnt[r] = pieces; A.rlen[r] = (u32)left;
    }
    if (__any(big) && !lane) { info->toolong = 1; info->stop = 1; }
    add_to(&info->n_pairs, wave_sum(pairs), lane);
    add_to(&info->n_skipped, wave_sum(skipped), lane);
    add_to(&info->n_overlap, wave_sum(overlap), lane);
    add_to(&info->n_cut, wave_sum(ncut), lane);
    add_to(&info->bases_in, wave_sum64(bases_in), lane);
    add_to(&info->bases_out, wave_sum64(bases_out), lane);
    add_to(&info->mismatches, wave_sum64(mism), lane);
    __syncthreads();
    for (u32 i = threadIdx.x; i < NHIST; i += 256)
        if (hist[i]) atomicAdd(reinterpret_cast<unsigned long long*>(&info->hist[i]), (unsigned long long)hist[i]);
}
// the pieces' sources and destinations, one behind the other
__global__ __launch_bounds__(256) void k_ovl_pieces(const OvlInfo* info, OvlArrays A, u64 n) {
    if (info->stop) return;
    const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
    if (r >= info->recs || r >= A.cap) return;
    const u64 a0 = A.ls[4 * r], a1 = A.ls[4 * r + 1], a2 = A.ls[4 * r + 2], a3 = A.ls[4 * r + 3], a4 = A.ls[4 * r + 4];
    u64 p = A.at[r], d = A.rdst[r];
    const u64 room = 3 * A.cap;
    record_pieces(a0, a1, a3, a4 < n ? a4 : n, a2 - a1 - 1, 0, A.keep[r], [&](u64 from, u64 len) {
        if (p < room) { A.from[p] = from; A.dst[p] = d; }
        p++; d += len;
    });
}
// behind the lengths' check: where the smallest unequal record begins
__global__ void k_ovl_bad(OvlInfo* info, const u64* ls) {
    if (threadIdx.x || blockIdx.x) return;
    if (info->bad_first != ~0ull && !info->status) info->bad_off = ls[4 * info->bad_first];
}
// behind the scans: what the copy is
__global__ void k_ovl_room(OvlInfo* info, OvlArrays A, u64 out_cap) {
    if (threadIdx.x || blockIdx.x) return;
    if (!info->stop) {
        info->copy.r0 = 0; info->copy.pieces = A.at[A.cap]; info->copy.nout = A.rdst[A.cap];
        if (info->copy.nout > out_cap) { info->status = OVL_ROOM; info->stop = 1; }
    }
    info->copy.status = info->stop;
}

}  // namespace

void launch_overlap_search(const PairText& t, const OvlArrays& A, const OvlJob& job, OvlInfo* info, hipStream_t st) {
    const QmapScratch q = qmap_scratch(t.d, t.n);
    const u64* before = reinterpret_cast<const u64*>(t.scratch + q.before_off);
    const dim3 per_rec((u32)((A.cap + 255) / 256)), per_pair((u32)((A.cap / 2 + 4) / 4));
    launch_line_starts(t, A.ls, 4 * A.cap, st);
    hipLaunchKernelGGL(k_ovl_check, dim3(1), dim3(64), 0, st, info, before + q.nspans, t.d + t.n - 1, t.n, A.ls, A.cap, job);
    hipLaunchKernelGGL(k_ovl_lens, per_rec, dim3(256), 0, st, info, (const u64*)A.ls);
    hipLaunchKernelGGL(k_ovl_bad, dim3(1), dim3(64), 0, st, info, (const u64*)A.ls);
    hipLaunchKernelGGL(k_ovl_search, dim3(per_pair.x < 16 * MAX_WG ? per_pair.x : 16 * MAX_WG), dim3(256), 0, st, (const OvlInfo*)info, t.d, t.n, job, A);
}
void launch_overlap(const PairText& t, const OvlArrays& A, const OvlJob& job, u8* out, OvlInfo* info, hipStream_t st) {
    const dim3 per_rec((u32)((A.cap + 255) / 256));
    launch_overlap_search(t, A, job, info, st);
    hipLaunchKernelGGL(k_ovl_cut, dim3(per_rec.x < MAX_WG ? per_rec.x : MAX_WG), dim3(256), 0, st, info, job, A, t.n);
    if (!job.cut) return;
    launch_scan_u32(A.cnt, A.at, A.cap, A.tmp, st);
    launch_scan_u32(A.rlen, A.rdst, A.cap, A.tmp, st);
    hipLaunchKernelGGL(k_ovl_room, dim3(1), dim3(64), 0, st, info, A, job.out_cap);
    hipLaunchKernelGGL(k_ovl_pieces, per_rec, dim3(256), 0, st, (const OvlInfo*)info, A, t.n);
    launch_pick_copy(A.dst, A.from, t.d, job.out_cap < t.n ? job.out_cap : t.n, out, &info->copy, st);
}

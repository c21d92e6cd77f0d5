// dmx.hip -- demultiplexed records: the units (records, or pairs) of a range of a FASTQ text sorted by the SAMPLE whose barcode their
// observed bytes match -- bytes of the header's index field or of the read's first bases --, every sample's units one behind the
// other in their original order, the unassigned units last (slimfastq_amd.h "demultiplexed records": sfq_demux_records,
// sfq_ctx_set_demux).  Text to text in the layout of dd.hip, with sel.hip's line starts and pick.hip's copy.  The one pass that does
// not keep or drop records in place: a STABLE MULTI-WAY PARTITION into up to 8194 classes.
//   1. launch_line_starts (sel.hip): ls[l] = where line l begins; k_dmx_check (one lane): lines and records, the final '\n', the range,
//      an odd count under pairs, the arrays' room.
//   2. k_dmx_assign: a lane per unit.  The barcode table is staged once per workgroup in LDS, a u64 per sample, two bits a base.  The
//      lane finds its parts' observed bytes -- in a header behind the line's last ':' and around the first '+' behind that, both
//      searched eight bytes at a time in the aligned words of the line, from its END --, packs them two bits a base with a mask of the
//      bytes that are no base (eight bytes a step, no byte loop), and compares: per sample an XOR, a fold to one bit a base, an OR with
//      the mask, a popcount.  It keeps the minimum, the first sample that attains it and whether another does.  cls[] takes the class
//      of the unit's records; the verdicts are counted per wavefront by ballot, per workgroup in LDS, and go out in one atomic a
//      counter and workgroup.  A record of 4 GiB or more and, with clip, the smallest record whose lines 2 and 4 differ are found
//      here; k_dmx_settle (one lane) turns them into the call's status.
//   3. The partition: an LSD radix sort of the records by class over digits of 8 bits -- one digit pass where there are at most 256
//      classes, two otherwise.  A pass: k_dmx_hist counts, per tile of DMX_TILE records, the records of every digit (LDS) into hist[],
//      laid out digit-major; launch_scan_u32 over hist[] gives, per digit and tile, where the tile's first record of that digit goes;
//      k_dmx_rank gives every record its place: that offset + the records of its digit in front of it in the tile -- found by matching
//      the digit across the wavefront with eight ballots, the wavefronts' counts summed in LDS, the tile taken in four rounds of 256
//      in order.  No atomic decides a place: ord[] is a function of cls[] alone.  Memory: 256 counters a tile, whatever the classes.
//   4. k_dmx_count / k_dmx_pieces: per sorted position the record's pieces -- the record, or with clip, for a record of an assigned
//      unit that loses bytes, three: line 1 | the rest of line 2, line 3 | the rest of line 4 -- scans number them and their bytes;
//      k_dmx_bounds: where the class changes between two sorted neighbours the parts between begin: part_off[] and the parts'
//      first sorted positions; k_dmx_room (one lane) checks the output's room.
//   5. pick.hip's k_pick_copy<false> (launch_pick_copy): the pieces in output order.
// Loads of the text are whole aligned 8-byte words that hold at least one byte of the line they belong to.  Every index into ls[] and
// the per-record arrays is below what k_dmx_check admitted; a place the rank computes is checked against the arrays' size all the same.
#include "kernels.h"
#include "dev_lines.h"

namespace {
using textspan::MAX_WG;

constexpr u32 DMX_HEADER = 1;                                  // sfq_demux_part.src: the header's field; 2: the bases
constexpr u64 ONES = 0x0101010101010101ull;

// bit 7 of every byte of x that is zero (exact: no carry leaves a byte)
__device__ __forceinline__ u64 zero_bytes(u64 x) {
    return ~(((x & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | x) & 0x8080808080808080ull;
}
// the aligned word at q, which holds a byte of [lo, hi); the bytes outside are zeroed
__device__ __forceinline__ u64 word_in(uintptr_t q, uintptr_t lo, uintptr_t hi) {
    u64 w = *reinterpret_cast<const u64*>(q);
    if (lo > q) w &= ~0ull << (8 * (lo - q));
    if (hi < q + 8) w &= ~0ull >> (8 * (q + 8 - hi));
    return w;
}
// the address of the last byte c in [lo, hi), 0 where there is none: from the end, a word a step
__device__ __forceinline__ uintptr_t last_byte(uintptr_t lo, uintptr_t hi, u32 c) {
    if (lo >= hi) return 0;
    for (uintptr_t q = (hi - 1) & ~(uintptr_t)7;; q -= 8) {
        const u64 z = zero_bytes(word_in(q, lo, hi) ^ (c * ONES));
        if (z) return q + ((63u - (u32)__clzll((long long)z)) >> 3);
        if (q <= lo) return 0;
    }
}
// the address of the first byte c in [lo, hi), 0 where there is none
__device__ __forceinline__ uintptr_t first_byte(uintptr_t lo, uintptr_t hi, u32 c) {
    if (lo >= hi) return 0;
    for (uintptr_t q = lo & ~(uintptr_t)7; q < hi; q += 8) {
        const u64 z = zero_bytes(word_in(q, lo, hi) ^ (c * ONES));
        if (z) return q + (((u32)__ffsll((long long)z) - 1u) >> 3);
    }
    return 0;
}
// eight bytes: (byte >> 1) & 3 of byte i in bits 2 i, 2 i + 1
__device__ __forceinline__ u64 pack_codes(u64 w) {
    u64 x = (w >> 1) & 0x0303030303030303ull;
    x = (x | (x >> 6)) & 0x000F000F000F000Full;
    x = (x | (x >> 12)) & 0x000000FF000000FFull;
    return (x | (x >> 24)) & 0xFFFFull;
}
// eight bytes: bit i where byte i is none of ACGTacgt
__device__ __forceinline__ u32 invalid_bytes(u64 w) {
    const u64 u = w & 0xDFDFDFDFDFDFDFDFull;
    const u64 v = zero_bytes(u ^ (0x41 * ONES)) | zero_bytes(u ^ (0x43 * ONES)) | zero_bytes(u ^ (0x47 * ONES)) | zero_bytes(u ^ (0x54 * ONES));
    const u64 t = ~v & 0x8080808080808080ull;
    return (u32)(((t >> 7) * 0x0102040810204080ull) >> 56);   // bits 8 i -> bits 56 + i: no two products on one bit
}
// bit i -> bit 2 i
__device__ __forceinline__ u64 spread32(u32 v) {
    u64 x = v;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    return (x | (x << 1)) & 0x5555555555555555ull;
}
// the len (1 .. 32) bytes at a: their codes, base i in bits 2 i, 2 i + 1, and bit i of inv where byte i is no base.  Reads the aligned
// words that hold one of the bytes, no other.
struct Obs { u64 code; u32 inv; };
__device__ __forceinline__ Obs observe(uintptr_t a, u32 len) {
    const uintptr_t q = a & ~(uintptr_t)7;
    const u32 s = (u32)(a & 7);
    Obs o{ 0, 0 };
    u64 lo = *reinterpret_cast<const u64*>(q);
#pragma unroll
    for (u32 j = 0; j < 4; j++) {
        if (8 * j < len) {
            u64 hi = 0;
            if (8 * (j + 1) - s < len) hi = *reinterpret_cast<const u64*>(q + 8 * (j + 1));      // it holds one of the bytes
            u64 w = s ? (lo >> (8 * s)) | (hi << (64 - 8 * s)) : lo;
            const u32 rem = len - 8 * j;
            if (rem < 8) w &= (1ull << (8 * rem)) - 1;
            o.code |= pack_codes(w) << (16 * j);
            o.inv |= invalid_bytes(w) << (8 * j);
            lo = hi;
        }
    }
    if (len < 32) o.inv &= (1u << len) - 1;
    return o;
}

// ---- 1. the rules ----------------------------------------------------------------------------------------------------------------
__global__ void k_dmx_check(DmxInfo* info, const u64* line_ends, const u8* last, u64 n, u64* ls, u64 cap, DmxJob job) {
    if (threadIdx.x || blockIdx.x) return;
    const bool open = *last != '\n';                           // a text without a final '\n' ends in a line all the same
    const u64 lines = *line_ends + open;
    const u64 recs = lines >> 2;
    u32 st = DMX_OK;
    info->lines = lines; info->recs = recs;
    if (lines & 3) st = DMX_LINES;
    if (!st && open) st = DMX_END;
    const bool to_end = job.nr == ~0ull;
    if (!st && (to_end ? job.r0 >= recs : (job.r0 > recs || job.nr > recs - job.r0))) st = DMX_RANGE;
    const u64 nr = st ? 0 : to_end ? recs - job.r0 : job.nr;
    if (!st && job.pairs && (nr & 1)) st = DMX_ODD;
    if (!st && recs > cap) st = DMX_CAP;
    if (!st) { ls[0] = 0; ls[lines] = n; }
    info->r0 = job.r0; info->nr = st ? 0 : nr; info->units = st ? 0 : job.pairs ? nr >> 1 : nr;
    info->bad_first = ~0ull;
    info->status = st; info->copy.status = st;
}

// ---- 2. the classes --------------------------------------------------------------------------------------------------------------
// a header's subfields: F = what lies behind the line's last ':', cut at its first '+'
struct Field { uintptr_t colon, plus, end; };
__device__ __forceinline__ Field parse_header(const u8* text, const u64* ls, u64 r) {
    const uintptr_t lo = (uintptr_t)(text + ls[4 * r]), hi = (uintptr_t)(text + ls[4 * r + 1] - 1);
    Field f{ last_byte(lo, hi, ':'), 0, hi };
    if (f.colon) f.plus = first_byte(f.colon + 1, hi, '+');
    return f;
}
template <u32 G>
__global__ __launch_bounds__(256) void k_dmx_assign(DmxInfo* info, const u8* __restrict__ text, DmxArrays A, DmxJob job) {
    extern __shared__ u64 tab[];                               // the barcodes
    __shared__ u32 sums[5];
    if (info->status) return;
    if ((u64)blockIdx.x * 256 >= info->units) return;          // (the grid is laid over the arrays: a workgroup behind the units stages no table)
    const u32 ns = job.n_samples, lane = threadIdx.x & 63;
    for (u32 i = threadIdx.x; i < ns; i += 256) tab[i] = A.codes[i];
    if (threadIdx.x < 5) sums[threadIdx.x] = 0;
    __syncthreads();
    const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
    const bool in = u < info->units && (u + 1) * G <= A.nlens;
    const u64 r0 = info->r0;
    bool shrt = false, toolong = false, bad = false;
    u64 code = 0, badrec = ~0ull;
    u32 inv = 0;
    if (in) {
#pragma unroll
        for (u32 g = 0; g < G; g++) {                          // the record's own checks
            const u64 r = r0 + u * G + g;
            const u64 a0 = A.ls[4 * r], a1 = A.ls[4 * r + 1], a2 = A.ls[4 * r + 2], a3 = A.ls[4 * r + 3], a4 = A.ls[4 * r + 4];
            toolong |= ((a4 - a0) >> 32) != 0;
            if (job.clip && a2 - a1 != a4 - a3 && !bad) { bad = true; badrec = r; }
        }
        Field f{ 0, 0, 0 };
        u32 fmate = ~0u, at = 0;
#pragma unroll
        for (u32 p = 0; p < 2; p++) {
            const DmxPart P = job.part[p];
            if (!P.len) continue;                              // (part 1 alone: absent)
            const u32 mate = G == 2 ? P.mate : 0u;
            const u64 r = r0 + u * G + mate, need = (u64)P.pos + P.len;
            uintptr_t from = 0;
            if (P.src == DMX_HEADER) {
                if (fmate != mate) { f = parse_header(text, A.ls, r); fmate = mate; }
                if (f.colon && (!P.sub || f.plus)) {
                    const uintptr_t sa = P.sub ? f.plus + 1 : f.colon + 1, se = P.sub || !f.plus ? f.end : f.plus;
                    if (se - sa >= need) from = sa + P.pos;
                }
            } else {
                const u64 a1 = A.ls[4 * r + 1], len2 = A.ls[4 * r + 2] - a1 - 1;
                if (len2 >= need) from = (uintptr_t)(text + a1) + P.pos;
            }
            if (!from) { shrt = true; continue; }
            const Obs o = observe(from, P.len);
            code |= o.code << (2 * at);
            inv |= o.inv << at;
            at += P.len;
        }
    }
    u32 best = 64, bi = 0;
    bool uniq = false;
    if (in && !shrt) {
        const u64 invs = spread32(inv);
        for (u32 s = 0; s < ns; s++) {
            const u64 x = code ^ tab[s];
            const u32 d = (u32)__popcll(((x | (x >> 1)) & 0x5555555555555555ull) | invs);
            if (d < best) { best = d; bi = s; uniq = true; }
            else if (d == best) uniq = false;
        }
    }
    const bool far = in && !shrt && best > job.max_mm, amb = in && !shrt && !far && !uniq;
    const bool asg = in && !shrt && !far && uniq, perfect = asg && best == 0;
    if (in) {
        const u32 part = asg ? bi : ns;
#pragma unroll
        for (u32 g = 0; g < G; g++) A.cls[u * G + g] = job.split ? 2 * part + g : part;
    }
    // the verdicts: a ballot per wavefront, LDS per workgroup, one atomic per counter
    const u64 m[5] = { __ballot(asg), __ballot(perfect), __ballot(in && shrt), __ballot(far), __ballot(amb) };
    if (!lane) {
#pragma unroll
        for (u32 i = 0; i < 5; i++) if (m[i]) atomicAdd(&sums[i], (u32)__popcll(m[i]));
    }
    if (__any(toolong) && !lane) info->pad = 1;
    const u64 mb = __ballot(bad);
    if (mb) {                                                  // the smallest bad record of the wavefront: its first bad lane's
        const u64 first = ((u64)(u32)__shfl((int)(u32)(badrec >> 32), __ffsll((long long)mb) - 1, 64) << 32) | (u32)__shfl((int)(u32)badrec, __ffsll((long long)mb) - 1, 64);
        if (!lane) atomicMin(reinterpret_cast<unsigned long long*>(&info->bad_first), (unsigned long long)first);
    }
    __syncthreads();
    if (threadIdx.x < 5 && sums[threadIdx.x]) {
        u64* to = threadIdx.x == 0 ? &info->n_assigned : threadIdx.x == 1 ? &info->n_perfect : threadIdx.x == 2 ? &info->n_short : threadIdx.x == 3 ? &info->n_far : &info->n_ambiguous;
        atomicAdd(reinterpret_cast<unsigned long long*>(to), (unsigned long long)sums[threadIdx.x]);
    }
}
// behind the classes: what the lanes found that refuses the call
__global__ void k_dmx_settle(DmxInfo* info, const u64* ls) {
    if (threadIdx.x || blockIdx.x || info->status) return;
    u32 st = DMX_OK;
    if (info->pad) st = DMX_LONG;
    else if (info->bad_first != ~0ull) { st = DMX_CLIP; info->bad_off = ls[4 * info->bad_first]; }
    info->pad = 0;
    if (st) { info->status = st; info->copy.status = st; }
}

// ---- 3. the partition ------------------------------------------------------------------------------------------------------------
// the record at sorted position i of a digit pass's input: in[] behind the first pass.  (Below nlens always: a pass fills every place.)
__device__ __forceinline__ u64 record_at(const u64* in, u64 i, u64 nlens) {
    const u64 rec = in ? in[i] : i;
    return rec < nlens ? rec : 0;
}
__global__ __launch_bounds__(256) void k_dmx_hist(const DmxInfo* info, DmxArrays A, const u64* __restrict__ in, u32 shift) {
    __shared__ u32 h[256];
    if (info->status) return;
    const u64 nr = info->nr < A.nlens ? info->nr : A.nlens, tile = blockIdx.x;
    h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (u32 k = 0; k < DMX_TILE / 256; k++) {
        const u64 i = tile * DMX_TILE + k * 256 + threadIdx.x;
        if (i < nr) atomicAdd(&h[(A.cls[record_at(in, i, A.nlens)] >> shift) & 255u], 1u);
    }
    __syncthreads();
    A.hist[(u64)threadIdx.x * A.ntiles + tile] = h[threadIdx.x];         // (a tile behind the range: zeros, which the scan wants)
}
__global__ __launch_bounds__(256) void k_dmx_rank(const DmxInfo* info, DmxArrays A, const u64* __restrict__ in, u64* __restrict__ out, u32 shift) {
    __shared__ u32 wcnt[4][256];
    __shared__ u64 base[256];
    if (info->status) return;
    const u64 nr = info->nr < A.nlens ? info->nr : A.nlens, tile = blockIdx.x;
    if (tile * DMX_TILE >= nr) return;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    base[threadIdx.x] = A.hoff[(u64)threadIdx.x * A.ntiles + tile];
    for (u32 k = 0; k < DMX_TILE / 256; k++) {
#pragma unroll
        for (u32 w = 0; w < 4; w++) wcnt[w][threadIdx.x] = 0;
        __syncthreads();
        const u64 i = tile * DMX_TILE + k * 256 + threadIdx.x;
        const bool valid = i < nr;
        const u64 rec = valid ? record_at(in, i, A.nlens) : 0;
        const u32 d = valid ? (A.cls[rec] >> shift) & 255u : 0u;
        u64 same = __ballot(valid);                            // the wavefront's lanes with this lane's digit
#pragma unroll
        for (u32 b = 0; b < 8; b++) {
            const u64 bal = __ballot((d >> b) & 1u);
            same &= (d >> b) & 1u ? bal : ~bal;
        }
        const u32 before = (u32)__popcll(same & ((1ull << lane) - 1));
        if (valid && !before) wcnt[wave][d] = (u32)__popcll(same);
        __syncthreads();
        if (valid) {
            u64 at = base[d] + before;
#pragma unroll
            for (u32 w = 0; w < 3; w++) if (w < wave) at += wcnt[w][d];
            if (at < A.nlens) out[at] = rec;                   // (always: the places of a pass are the range's positions)
        }
        __syncthreads();
        base[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];      // (its own column: the next round's barrier publishes it)
    }
}

// ---- 4. pieces, bounds, room -----------------------------------------------------------------------------------------------------
// what the record at sorted position i loses in front of its lines 2 and 4
__device__ __forceinline__ u32 clip_of(const DmxJob& job, const DmxArrays& A, u64 rec) {
    const u32 c = A.cls[rec], part = job.split ? c >> 1 : c;
    if (!job.clip || part >= job.n_samples) return 0;
    return job.pairs && (rec & 1) ? job.clip1 : job.clip0;
}
__global__ __launch_bounds__(256) void k_dmx_count(const DmxInfo* info, DmxArrays A, DmxJob job, const u64* __restrict__ ord) {
    if (info->status) return;
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= info->nr || i >= A.nlens) return;
    A.cnt[i] = clip_of(job, A, record_at(ord, i, A.nlens)) ? 3u : 1u;
}
// lens[] was zeroed; at: null without clip (piece i is the record at position i)
__global__ __launch_bounds__(256) void k_dmx_pieces(const DmxInfo* info, DmxArrays A, DmxJob job, const u64* __restrict__ ord, const u64* __restrict__ at) {
    if (info->status) return;
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= info->nr || i >= A.nlens) return;
    const u64 rec = record_at(ord, i, A.nlens), r = info->r0 + rec;
    const u64 a0 = A.ls[4 * r], a4 = A.ls[4 * r + 4];
    const u64 p = at ? at[i] : i;
    const u32 c = clip_of(job, A, rec);
    if (!c) { if (p < A.pcap) { A.from[p] = a0; A.lens[p] = (u32)(a4 - a0); } return; }
    const u64 a1 = A.ls[4 * r + 1], a3 = A.ls[4 * r + 3];     // (lines 2 and 4 hold c bytes: an assigned unit's parts are not short)
    if (p + 2 >= A.pcap) return;
    A.from[p] = a0; A.lens[p] = (u32)(a1 - a0);
    A.from[p + 1] = a1 + c; A.lens[p + 1] = (u32)(a3 - a1 - c);
    A.from[p + 2] = a3 + c; A.lens[p + 2] = (u32)(a4 - a3 - c);
}
// a lane per sorted position and one behind the last: the parts that begin there
__global__ __launch_bounds__(256) void k_dmx_bounds(const DmxInfo* info, DmxArrays A, DmxJob job, const u64* __restrict__ ord, const u64* __restrict__ at) {
    if (info->status) return;
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x, nr = info->nr;
    if (i > nr || nr > A.nlens) return;
    const u32 ci = i < nr ? A.cls[record_at(ord, i, A.nlens)] : job.np, first = i ? A.cls[record_at(ord, i - 1, A.nlens)] + 1 : 0u;
    if (first > ci) return;
    const u64 off = A.dst[at ? at[i] : i];
    for (u32 c = first; c <= ci && c <= job.np; c++) { A.bounds[c] = off; A.bounds[job.np + 1 + c] = i; }     // (the empty parts in front of ci begin here too)
}
__global__ void k_dmx_room(DmxInfo* info, DmxArrays A, DmxJob job, const u64* at) {
    if (threadIdx.x || blockIdx.x || info->status) return;
    const u64 pieces = at ? at[info->nr] : info->nr, nout = A.dst[pieces];
    info->copy.r0 = 0; info->copy.pieces = pieces; info->copy.nout = nout;
    if (nout > job.out_cap) { info->status = DMX_ROOM; info->copy.status = DMX_ROOM; }
}

void digit_pass(const DmxArrays& A, const u64* in, u64* out, u32 shift, const DmxInfo* info, hipStream_t st) {
    hipLaunchKernelGGL(k_dmx_hist, dim3((u32)A.ntiles), dim3(256), 0, st, info, A, in, shift);
    launch_scan_u32(A.hist, A.hoff, 256 * A.ntiles, A.tmp, st);
    hipLaunchKernelGGL(k_dmx_rank, dim3((u32)A.ntiles), dim3(256), 0, st, info, A, in, out, shift);
}

}  // namespace

void launch_demux(const PairText& t, const DmxArrays& A, const DmxJob& job, u8* out, DmxInfo* info, hipStream_t st) {
    const QmapScratch q = qmap_scratch(t.d, t.n);
    u64* before = reinterpret_cast<u64*>(t.scratch + q.before_off);
    launch_line_starts(t, A.ls, 4 * A.cap, st);
    hipLaunchKernelGGL(k_dmx_check, dim3(1), dim3(64), 0, st, info, (const u64*)before + q.nspans, t.d + t.n - 1, t.n, A.ls, A.cap, job);
    const dim3 ugrid((u32)((A.ucap + 255) / 256)), rgrid((u32)((A.nlens + 255) / 256));
    const size_t lds = (size_t)job.n_samples * 8;
    if (job.pairs) hipLaunchKernelGGL(k_dmx_assign<2>, ugrid, dim3(256), lds, st, info, t.d, A, job);
    else hipLaunchKernelGGL(k_dmx_assign<1>, ugrid, dim3(256), lds, st, info, t.d, A, job);
    hipLaunchKernelGGL(k_dmx_settle, dim3(1), dim3(64), 0, st, info, (const u64*)A.ls);
    digit_pass(A, nullptr, A.ord_a, 0, info, st);
    const u64* ord = A.ord_a;
    if (job.np > 256) { digit_pass(A, A.ord_a, A.ord_b, 8, info, st); ord = A.ord_b; }
    const u64* at = nullptr;
    if (job.clip) {
        (void)hipMemsetAsync(A.cnt, 0, A.nlens * 4, st);
        hipLaunchKernelGGL(k_dmx_count, rgrid, dim3(256), 0, st, (const DmxInfo*)info, A, job, ord);
        launch_scan_u32(A.cnt, A.at, A.nlens, A.tmp, st);
        at = A.at;
    }
    (void)hipMemsetAsync(A.lens, 0, A.pcap * 4, st);
    hipLaunchKernelGGL(k_dmx_pieces, rgrid, dim3(256), 0, st, (const DmxInfo*)info, A, job, ord, at);
    launch_scan_u32(A.lens, A.dst, A.pcap, A.tmp, st);
    hipLaunchKernelGGL(k_dmx_bounds, dim3((u32)((A.nlens + 256) / 256)), dim3(256), 0, st, (const DmxInfo*)info, A, job, ord, at);
    hipLaunchKernelGGL(k_dmx_room, dim3(1), dim3(64), 0, st, info, A, job, at);
    launch_pick_copy(A.dst, A.from, t.d, job.out_cap < t.n ? job.out_cap : t.n, out, &info->copy, st);
}

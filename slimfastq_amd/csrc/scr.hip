// scr.hip -- screened records: the units (records, or pairs) of a range of a FASTQ text whose line 2 shares enough k-mers with a set of
// reference k-mers, dropped (decontamination) or kept alone (baits) (slimfastq_amd.h "screened records": sfq_screen_records,
// sfq_screen_set_add, sfq_ctx_set_screen).  Text to text in the layout of dd.hip, with sel.hip's line starts and pick.hip's copy.
//   The set: an open-addressed table of 64-bit slots in device memory, 0 (empty) or SCR_OCC | the k-mer's canonical value, WHOLE: no
//      fingerprint, membership is exact.  A k-mer's home slot is the top bits of canonical * 0x9E3779B97F4A7C15 (scr_home); probing is
//      linear, every probe loop bounded by the slot count.  What the table says of a value does not depend on the order of the inserts.
//   k_scr_add: a lane per 64 bytes of a sequence text; it warms up on the k - 1 bytes in front of its stretch (more where that is
//      cheaper: any byte in front may be taken, a window is COUNTED only where it ends inside the stretch, so every window is formed
//      once), rolls the forward and the reverse-complement value from byte to byte and inserts the smaller with compare-and-swap.  A
//      device counter counts the slots claimed: the distinct k-mers.
//   1. launch_line_starts (sel.hip): ls[l] = where line l begins; k_scr_check (one lane): lines and records, the range, an odd count
//      under pairs, the arrays' room.
//   2. k_scr_count, the hot kernel: G lanes a record (8), each a contiguous stretch of the aligned 8-byte words that hold line 2, with
//      the same warm-up; H = the windows whose canonical value the set holds, W = all windows, summed across the group.  A record of
//      4 GiB or more is refused here, before its line is walked.  The set is only read.
//   3. k_scr_verdict: a lane per unit: matched = H >= min_hits and 100 H >= min_pct W (64-bit), either or both mates under pairs; kept =
//      matched == keep_matched; the report's sums, keep[] and rlen[] per record.  Scans number the kept records and their bytes;
//      k_scr_scatter compacts starts and lengths; k_scr_room (one lane) checks the output's room.
//   4. pick.hip's k_pick_copy<false> (launch_pick_copy): the kept records are its pieces.
// Loads are whole aligned 8-byte words that hold at least one byte of a line 2 (of the sequence text: of its buffer, which the library
// pads), never another.  A byte outside the line that such a word holds does no harm: in front of line 2 stands a '\n', a break, and
// behind the stretch nothing is counted.  Every index into ls[] and the per-record arrays is below what k_scr_check admitted.
#include "kernels.h"

namespace {

__device__ __forceinline__ u64 scr_home(u64 canon, const ScrSetDev& S) { return (canon * 0x9E3779B97F4A7C15ull) >> S.shift; }

// the rolling state of one lane: the last k codes as a forward value and as the reverse complement's, and how many bytes since the last break
struct Roll {
    u64 fwd = 0, rev = 0; u32 run = 0;
    // takes a byte; true where a window ends at it, *canon its canonical value
    __device__ __forceinline__ bool push(u32 c, u32 k, u64 kmask, u32 top, u64* canon) {
        const u32 t = (c & 0xDFu) - 0x41u;                     // 'A' 'a' 0, 'C' 'c' 2, 'G' 'g' 6, 'T' 't' 19: every other byte is a break
        const bool base = t < 20u && ((0x80045u >> t) & 1u);
        const u64 code = ((c >> 1) ^ (c >> 2)) & 3u;           // A 0, C 1, G 2, T 3, either case
        fwd = ((fwd << 2) | code) & kmask;
        rev = (rev >> 2) | ((3 - code) << top);
        run = base ? run + 1 : 0;                              // (behind a break k codes are shifted in before a window counts: no reset)
        *canon = fwd < rev ? fwd : rev;
        return run >= k;
    }
};

__device__ __forceinline__ bool scr_has(const ScrSetDev& S, u64 canon) {
    const u64 want = SCR_OCC | canon;
    u64 i = scr_home(canon, S);
    for (u64 probe = 0; probe <= S.smask; probe++, i = (i + 1) & S.smask) {
        const u64 cur = S.slots[i];
        if (cur == want) return true;
        if (!cur) return false;
    }
    return false;                                              // (a table without an empty slot cannot be: it holds twice max_kmers)
}

// ---- the set, written ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_scr_add(const u8* __restrict__ seq, u64 n, ScrSetDev S, u64 max_kmers, ScrAddInfo* info) {
    const u64 s = ((u64)blockIdx.x * 256 + threadIdx.x) * 64;  // the lane counts the windows that end in [s, e)
    if (s >= n) return;
    const u64 e = s + 64 < n ? s + 64 : n;
    const u32 k = S.k, top = 2 * (k - 1);
    const u64 kmask = (1ull << (2 * k)) - 1;
    const u64 ws = s >= 32 ? s - 32 : 0;                       // the aligned words that hold the k - 1 <= 30 bytes in front (seq is 16-byte aligned)
    unsigned long long* T = reinterpret_cast<unsigned long long*>(S.slots);
    unsigned long long* count = reinterpret_cast<unsigned long long*>(&info->kmers);
    Roll r;
    for (u64 at = ws; at < e; at += 8) {
        const u64 word = *reinterpret_cast<const u64*>(seq + at);
#pragma unroll
        for (u32 b = 0; b < 8; b++) {
            u64 canon;
            const bool win = r.push((u32)(word >> (8 * b)) & 0xFFu, k, kmask, top, &canon);
            const u64 pos = at + b;
            if (!win || pos < s || pos >= e) continue;
            if (__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > max_kmers) return;      // the call is refused already
            const u64 want = SCR_OCC | canon;
            u64 i = scr_home(canon, S), probe = 0;
            for (; probe <= S.smask; probe++, i = (i + 1) & S.smask) {
                u64 cur = __hip_atomic_load(&T[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (!cur) {
                    cur = atomicCAS(&T[i], 0ull, (unsigned long long)want);
                    if (!cur) { atomicAdd(count, 1ull); break; }
                }
                if (cur == want) break;                        // a slot that holds the value already: done
            }
            if (probe > S.smask) info->full = 1;
        }
    }
}

// ---- 1. the rules ----------------------------------------------------------------------------------------------------------------
__global__ void k_scr_check(ScrInfo* info, const u64* line_ends, const u8* last, u64 n, u64* ls, u64 cap, ScrJob job) {
    if (threadIdx.x || blockIdx.x) return;
    const bool open = *last != '\n';                           // a text without a final '\n' ends in a line all the same
    const u64 lines = *line_ends + open;
    const u64 recs = lines >> 2;
    u32 st = SCR_OK;
    info->lines = lines; info->recs = recs;
    if (lines & 3) st = SCR_LINES;
    const bool to_end = job.nr == ~0ull;
    if (!st && (to_end ? job.r0 >= recs : (job.r0 > recs || job.nr > recs - job.r0))) st = SCR_RANGE;
    const u64 nr = st ? 0 : to_end ? recs - job.r0 : job.nr;
    if (!st && job.pairs && (nr & 1)) st = SCR_ODD;
    if (!st && recs > cap) st = SCR_CAP;
    if (!st) { ls[0] = 0; ls[lines] = n + open; }
    info->r0 = job.r0; info->nr = st ? 0 : nr; info->units = st ? 0 : job.pairs ? nr >> 1 : nr;
    info->status = st; info->copy.status = st;
}

// ---- 2. hits and windows ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 shfl_xor32(u32 v, int o) { return (u32)__shfl_xor((int)v, o, 64); }
// G lanes a record: the aligned words that hold line 2 are dealt out in G contiguous stretches; a lane reads the words that hold the
// k - 1 bytes in front of its stretch too and counts the windows that end inside the stretch.  G = 1 is a lane a record.
template <u32 G>
__global__ __launch_bounds__(256) void k_scr_count(ScrInfo* info, const u8* __restrict__ text, ScrArrays A, ScrSetDev S, u64 n) {
    if (info->status) return;
    const u32 sub = threadIdx.x % G;
    const u64 idx = ((u64)blockIdx.x * 256 + threadIdx.x) / G; // a record of the range
    const bool in = idx < info->nr;                            // (every lane takes part in the shuffles)
    u64 at = 0, len = 0;
    if (in) {
        const u64 r = info->r0 + idx, a0 = A.ls[4 * r], a1 = A.ls[4 * r + 1], a2 = A.ls[4 * r + 2], a4 = A.ls[4 * r + 4];
        at = a1; len = a2 - a1 - 1;
        // a record of 4 GiB or more: refused HERE, in front of the walk over its line (the counts behind this kernel are 32-bit)
        if ((((a4 < n ? a4 : n) - a0) >> 32) != 0) {
            if (!sub) { info->status = SCR_LONG; info->copy.status = SCR_LONG; }
            len = 0;
        }
    }
    const u32 k = S.k, top = 2 * (k - 1);
    const u64 kmask = (1ull << (2 * k)) - 1;
    const uintptr_t p = (uintptr_t)(text + at), q = p & ~(uintptr_t)7;
    const i64 sh = (i64)(p & 7);                               // byte b of word j is the line's byte 8 j + b - sh
    const u64 nw = len ? ((u64)sh + len + 7) >> 3 : 0, per = (nw + G - 1) / G;
    const u64 w0 = sub * per < nw ? sub * per : nw, w1 = w0 + per < nw ? w0 + per : nw;
    i64 s = 8 * (i64)w0 - sh, e = 8 * (i64)w1 - sh;
    if (s < 0) s = 0;
    if (e > (i64)len) e = (i64)len;
    const u64 back = (u64)(k - 1 + 7) >> 3;                    // the words that hold the k - 1 bytes in front of an aligned stretch
    u32 H = 0, W = 0;
    Roll r;
    for (u64 j = w0 == w1 ? w1 : w0 > back ? w0 - back : 0; j < w1; j++) {
        const u64 word = *reinterpret_cast<const u64*>(q + 8 * j);
        const i64 pos0 = 8 * (i64)j - sh;
#pragma unroll
        for (u32 b = 0; b < 8; b++) {
            u64 canon;
            const bool win = r.push((u32)(word >> (8 * b)) & 0xFFu, k, kmask, top, &canon);
            const i64 pos = pos0 + b;
            if (win && pos >= s && pos < e) { W++; H += scr_has(S, canon) ? 1u : 0u; }
        }
    }
#pragma unroll
    for (u32 o = 1; o < G; o <<= 1) { H += shfl_xor32(H, (int)o); W += shfl_xor32(W, (int)o); }
    if (in && !sub && idx < A.nlens) { A.hits[idx] = H; A.wins[idx] = W; }
}

// ---- 3. verdicts, lengths, destinations --------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += ((u64)shfl_xor32((u32)(v >> 32), o) << 32) | shfl_xor32((u32)v, o);
    return v;
}
template <u32 G>
__global__ __launch_bounds__(256) void k_scr_verdict(ScrInfo* info, ScrJob job, ScrArrays A, u64 n) {
    if (info->status) return;
    const u32 lane = threadIdx.x & 63;
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 U = info->units, r0 = info->r0;
    const bool in = t < U;
    u64 nm = 0, sw = 0, sh = 0, len[G];
#pragma unroll
    for (u32 g = 0; g < G; g++) {
        len[g] = 0;
        if (!in) continue;
        const u64 k = t * G + g, r = r0 + k, a0 = A.ls[4 * r], a4 = A.ls[4 * r + 4];
        const u64 H = A.hits[k], W = A.wins[k];
        len[g] = (a4 < n ? a4 : n) - a0;                       // (below 4 GiB: k_scr_count refused the call otherwise)
        nm += H >= job.min_hits && 100 * H >= (u64)job.min_pct * W ? 1 : 0;
        sw += W; sh += H;
    }
    const bool matched = job.pairs == 2 ? nm == G : nm != 0;   // a record; either mate; both mates
    const bool keep = in && matched == (job.keep_matched != 0);
    const u64 mk = __ballot(keep);
    nm = wave_sum64(nm); sw = wave_sum64(sw); sh = wave_sum64(sh);
    if (!lane) {
        if (mk) atomicAdd(reinterpret_cast<unsigned long long*>(&info->kept), (unsigned long long)__popcll(mk));
        if (nm) atomicAdd(reinterpret_cast<unsigned long long*>(&info->matched), (unsigned long long)nm);
        if (sw) atomicAdd(reinterpret_cast<unsigned long long*>(&info->windows), (unsigned long long)sw);
        if (sh) atomicAdd(reinterpret_cast<unsigned long long*>(&info->hits), (unsigned long long)sh);
    }
#pragma unroll
    for (u32 g = 0; g < G; g++) {
        const u64 k = t * G + g;
        if (k < A.nlens) { A.keep[k] = keep ? 1u : 0u; A.rlen[k] = keep ? (u32)len[g] : 0u; }
    }
}
// the kept records' starts and lengths, one behind the other (lens[] was zeroed)
__global__ __launch_bounds__(256) void k_scr_scatter(const ScrInfo* info, ScrArrays A) {
    if (info->status) return;
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= info->nr || k >= A.nlens || !A.keep[k]) return;
    const u64 p = A.pos[k];
    A.from[p] = A.ls[4 * (info->r0 + k)];
    A.lens[p] = A.rlen[k];
}
// behind the scans: what the copy is
__global__ void k_scr_room(ScrInfo* info, ScrArrays A, ScrJob job) {
    if (threadIdx.x || blockIdx.x || info->status) return;
    const u64 kept = A.pos[A.nlens], nout = A.dst[A.nlens];
    info->copy.r0 = 0; info->copy.pieces = kept; info->copy.nout = nout;
    if (nout > job.out_cap) { info->status = SCR_ROOM; info->copy.status = SCR_ROOM; }
    else if (!kept) info->copy.status = SCR_NOTHING;
}

template <u32 G>
void launch_count(const PairText& t, const ScrArrays& A, const ScrSetDev& S, ScrInfo* info, hipStream_t st) {
    hipLaunchKernelGGL(k_scr_count<G>, dim3((u32)((G * A.nlens + 255) / 256)), dim3(256), 0, st, info, t.d, A, S, t.n);
}

}  // namespace

void launch_screen_add(const u8* seq, u64 n, const ScrSetDev& S, u64 max_kmers, ScrAddInfo* info, hipStream_t st) {
    if (n < S.k) return;
    hipLaunchKernelGGL(k_scr_add, dim3((u32)(((n + 63) / 64 + 255) / 256)), dim3(256), 0, st, seq, n, S, max_kmers, info);
}

void launch_screen(const PairText& t, const ScrArrays& A, const ScrJob& job, const ScrSetDev& S, u32 lanes, u8* out, ScrInfo* info, hipStream_t st) {
    const QmapScratch q = qmap_scratch(t.d, t.n);
    u64* before = reinterpret_cast<u64*>(t.scratch + q.before_off);
    launch_line_starts(t, A.ls, 4 * A.cap, st);
    hipLaunchKernelGGL(k_scr_check, dim3(1), dim3(64), 0, st, info, (const u64*)before + q.nspans, t.d + t.n - 1, t.n, A.ls, A.cap, job);
    switch (lanes) {
    case 1: launch_count<1>(t, A, S, info, st); break;
    case 4: launch_count<4>(t, A, S, info, st); break;
    case 16: launch_count<16>(t, A, S, info, st); break;
    default: launch_count<8>(t, A, S, info, st); break;
    }
    const dim3 grid((u32)((A.nlens + 255) / 256));
    if (job.pairs) hipLaunchKernelGGL(k_scr_verdict<2>, dim3((u32)(((A.nlens + 1) / 2 + 255) / 256)), dim3(256), 0, st, info, job, A, t.n);
    else hipLaunchKernelGGL(k_scr_verdict<1>, grid, dim3(256), 0, st, info, job, A, t.n);
    (void)hipMemsetAsync(A.lens, 0, A.nlens * 4, st);
    launch_scan_u32(A.keep, A.pos, A.nlens, A.tmp, st);
    hipLaunchKernelGGL(k_scr_scatter, grid, dim3(256), 0, st, (const ScrInfo*)info, A);
    launch_scan_u32(A.lens, A.dst, A.nlens, A.tmp, st);
    hipLaunchKernelGGL(k_scr_room, dim3(1), dim3(64), 0, st, info, A, job);
    launch_pick_copy(A.dst, A.from, t.d, job.out_cap < t.n ? job.out_cap : t.n, out, &info->copy, st);
}

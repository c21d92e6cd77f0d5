// dd.hip -- distinct records: the units (records, or pairs) of a range of a FASTQ text whose KEY -- line 2 with 'a'..'z' folded to
// 'A'..'Z', under pairs the ordered pair of both mates' -- no earlier unit of the range has and, with a set, no unit that an earlier
// call kept (slimfastq_amd.h "distinct records": sfq_dedup_records, sfq_ctx_set_dedup).  Text to text in the layout of sel.hip, whose
// line starts it uses, and with pick.hip's copy.  The one pass in which a record's verdict depends on every other record:
//   1. launch_line_starts (sel.hip): ls[l] = where line l begins; k_dd_check (one lane): lines and records, the range, an odd count
//      under pairs, the arrays' room, the units U of the range and the call's table: the smallest power of two of at least 2 U slots.
//   2. k_dd_clear empties that table; k_dd_hash: eight lanes per unit, each taking aligned 16-byte units of the key (a line begins
//      at any byte: two neighbouring units are shifted together, the last word masked), folded eight bytes at a time; the hash is a
//      SUM of per-word mixes keyed by the word's position, so the lanes' shares are combined in any order.  A record of 4 GiB or
//      more, or a pair whose keys hold as much together, is refused here, before its key is walked.
//   3. k_dd_insert: a lane per unit, linear probing over 64-bit slots with device-scope compare-and-swap.  A slot is 0 (empty) or
//      occupied | a 23-bit fingerprint of the hash | a 40-bit payload, in the call's table the number of a unit.  An empty slot is
//      claimed; a slot with the unit's fingerprint is COMPARED, key against key in the text, and where they are equal the unit's
//      number goes in with atomicMin: the slot ends up naming the EARLIEST unit with that key, whatever the scheduling was.  Slots are
//      never emptied while the kernel runs, so all units of one key meet in one slot.  Every probe loop is bounded by the slot count.
//   4. with a set, k_dd_probe: every unit that won its slot looks its key up in the set's table (payload: the key's number in the set;
//      koff[], klen[] and the arena hold the keys); the set is only READ here, so a call that is refused leaves it as it was.
//   5. k_dd_verdict: a lane per unit: kept = it won its slot and its key is not in the set; the report's counts (a ballot and a
//      popcount per wavefront), keep[] and rlen[] per record, kb[] = the key bytes a kept unit adds to the set.  Scans number the
//      kept records, their bytes and the new keys' bytes; k_dd_scatter compacts starts and lengths; k_dd_room (one lane) checks the
//      output's room and the set's, keys and bytes.
//   6. with a set, and only where nothing was refused, k_dd_commit: every kept unit writes its lengths, its offset and its folded key
//      into the set's arrays and claims the first empty slot of its probe sequence (kept units have distinct keys, none of them in
//      the set: no compare is needed).  Keys fit because k_dd_room said so; the loop is bounded all the same.
//   7. pick.hip's k_pick_copy<false> (launch_pick_copy): the kept records are its pieces.
// Loads are whole aligned words that hold at least one byte of a key, so of the text.  Every index into ls[] and the per-unit arrays
// is below what k_dd_check admitted.
#include "kernels.h"
#include "dev_lines.h"

namespace {

constexpr u64 DD_OCC = 1ull << 63, DD_PAY = (1ull << 40) - 1;
__device__ __forceinline__ u64 dd_fp(u64 h) { return (h >> 41) << 40 & ~DD_OCC; }      // 23 bits, in place
__device__ __forceinline__ u64 mix64(u64 x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// 'a'..'z' of eight bytes to 'A'..'Z'; every other byte stands
__device__ __forceinline__ u64 fold8(u64 x) {
    const u64 h = x & 0x7F7F7F7F7F7F7F7Full;
    const u64 ge_a = h + 0x1F1F1F1F1F1F1F1Full, gt_z = h + 0x0505050505050505ull;      // bit 7: the byte's low seven bits are >= 0x61, > 0x7A
    const u64 m = ge_a & ~gt_z & ~x & 0x8080808080808080ull;
    return x ^ (m >> 2);
}
__device__ __forceinline__ u8 fold1(u8 c) { return c >= 'a' && c <= 'z' ? (u8)(c - 32) : c; }

// the bytes [b, b + len) eight at a time from the aligned words that hold them; no word without a byte of them is read
struct KeyWords {
    uintptr_t q; u32 s; u64 len, j, lo;
    __device__ __forceinline__ KeyWords(const u8* b, u64 l) {
        const uintptr_t p = (uintptr_t)b;
        q = p & ~(uintptr_t)7; s = (u32)(p & 7); len = l; j = 0;
        lo = l ? *reinterpret_cast<const u64*>(q) : 0;
    }
    __device__ __forceinline__ u64 next() {                  // bytes 8 j .. of the key, zeros behind its end
        u64 hi = 0;
        if (8 * (j + 1) - s < len) hi = *reinterpret_cast<const u64*>(q + 8 * (j + 1));       // the next word holds a byte of the key
        u64 w = s ? (lo >> (8 * s)) | (hi << (64 - 8 * s)) : lo;
        const u64 rem = len - 8 * j;
        if (rem < 8) w &= (1ull << (8 * rem)) - 1;
        lo = hi; j++;
        return w;
    }
};
// what word j of a key (its bytes 8 j .., zeros behind its end) adds to the key's hash: the words may be added in any order
__device__ __forceinline__ u64 word_mix(u64 w, u64 j) {
    u64 x = fold8(w) + (j + 1) * 0x9E3779B97F4A7C15ull;
    x *= 0xD6E8FEB86659FD93ull; x ^= x >> 32;
    return x * 0xBF58476D1CE4E5B9ull;
}
// either side folded: a key of the text against one of the text, or against one of the set's arena (folding a folded key changes nothing)
__device__ __forceinline__ bool lines_equal(const u8* a, const u8* b, u64 len) {
    KeyWords x(a, len), y(b, len);
    for (u64 j = 0; j < (len + 7) / 8; j++)
        if (fold8(x.next()) != fold8(y.next())) return false;
    return true;
}

// line 2 of record r: where it begins and its length
__device__ __forceinline__ void base_line(const u64* ls, u64 r, u64* at, u64* len) {
    const u64 a1 = ls[4 * r + 1], a2 = ls[4 * r + 2];
    *at = a1; *len = a2 - a1 - 1;
}
template <u32 G>
__device__ __forceinline__ bool units_equal(const u8* text, const u64* ls, u64 r0, u64 u, u64 v) {
    u64 au[G], lu[G], av[G], lv[G];
#pragma unroll
    for (u32 g = 0; g < G; g++) { base_line(ls, r0 + u * G + g, &au[g], &lu[g]); base_line(ls, r0 + v * G + g, &av[g], &lv[g]); }
#pragma unroll
    for (u32 g = 0; g < G; g++) if (lu[g] != lv[g]) return false;
#pragma unroll
    for (u32 g = 0; g < G; g++) if (!lines_equal(text + au[g], text + av[g], lu[g])) return false;
    return true;
}

// ---- 1. the rules ----------------------------------------------------------------------------------------------------------------
__global__ void k_dd_check(DdInfo* info, const u64* line_ends, const u8* last, u64 n, u64* ls, u64 cap, u64 tcap, DdJob job) {
    if (threadIdx.x || blockIdx.x) return;
    const bool open = *last != '\n';                           // a text without a final '\n' ends in a line all the same
    const u64 lines = *line_ends + open;
    const u64 recs = lines >> 2;
    u32 st = DD_OK;
    info->lines = lines; info->recs = recs;
    if (lines & 3) st = DD_LINES;
    const bool to_end = job.nr == ~0ull;
    if (!st && (to_end ? job.r0 >= recs : (job.r0 > recs || job.nr > recs - job.r0))) st = DD_RANGE;
    const u64 nr = st ? 0 : to_end ? recs - job.r0 : job.nr;
    if (!st && job.pairs && (nr & 1)) st = DD_ODD;
    if (!st && recs > cap) st = DD_CAP;
    const u64 units = job.pairs ? nr >> 1 : nr;
    u64 slots = 2;
    while (slots < 2 * units && slots < tcap) slots <<= 1;
    if (!st && slots < 2 * units) st = DD_CAP;                 // (cannot be: the table was laid out for the arrays' units)
    if (!st) { ls[0] = 0; ls[lines] = n + open; }
    info->r0 = job.r0; info->nr = st ? 0 : nr; info->units = st ? 0 : units; info->tmask = slots - 1;
    info->status = st; info->copy.status = st;
}
__global__ __launch_bounds__(256) void k_dd_clear(const DdInfo* info, u64* table) {
    if (info->status) return;
    const u64 slots = info->tmask + 1;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < slots; i += (u64)gridDim.x * 256) table[i] = 0;
}

// ---- 2. the hashes ---------------------------------------------------------------------------------------------------------------
// a key's hash: mix64(its length + a constant) + the sum of word_mix over its words; a pair's: its mates' in order, mixed between.
// Eight lanes a unit: a lane takes the key sixteen bytes at a time from the two aligned 16-byte units that hold them, so that a
// wavefront's loads fall into a few contiguous runs; the lanes' sums are added across the group.  (A lane per unit, walking the key
// as 8-byte words, gives the same hashes and took 0.59 ms where this takes 0.22 ms, 2 M reads of 150 bases: DESIGN.md 4.20.)
__device__ __forceinline__ u64 shfl_xor64(u64 v, int o) {
    return ((u64)(u32)__shfl_xor((int)(u32)(v >> 32), o, 64) << 32) | (u32)__shfl_xor((int)(u32)v, o, 64);
}
template <u32 G>
__global__ __launch_bounds__(256) void k_dd_hash(DdInfo* info, const u8* __restrict__ text, DdArrays A, u64 n) {
    if (info->status) return;
    const u32 sub = threadIdx.x & 7;
    const u64 u = ((u64)blockIdx.x * 256 + threadIdx.x) >> 3;
    const bool in = u < info->units;                           // (every lane takes part in the shuffles)
    // a record of 4 GiB or more, or a unit whose keys hold as much together: refused HERE, in front of the walk over its key (the
    // lengths behind this kernel are 32-bit), and the key is not walked
    u64 ats[G], lens[G], kbytes = 0;
    bool toolong = false;
#pragma unroll
    for (u32 g = 0; g < G; g++) {
        ats[g] = 0; lens[g] = 0;
        if (in) {
            const u64 r = info->r0 + u * G + g, a0 = A.ls[4 * r], a4 = A.ls[4 * r + 4];
            base_line(A.ls, r, &ats[g], &lens[g]);
            kbytes += lens[g];
            toolong |= (((a4 < n ? a4 : n) - a0) >> 32) != 0;
        }
    }
    toolong |= (kbytes >> 32) != 0;
    if (toolong && !sub) { info->status = DD_LONG; info->copy.status = DD_LONG; }
    u64 h = 0;
#pragma unroll
    for (u32 g = 0; g < G; g++) {
        const u64 at = ats[g], len = toolong ? 0 : lens[g];
        const uintptr_t p = (uintptr_t)(text + at), q = p & ~(uintptr_t)15;
        const u32 s = (u32)(p & 15), s8 = 8 * (s & 7);
        u64 part = 0;
        for (u64 k = sub; 16 * k < len; k += 8) {              // key bytes [16 k, 16 k + 16): aligned units k and k + 1 from q on
            const uint4 lo = *reinterpret_cast<const uint4*>(q + 16 * k);
            uint4 hi = make_uint4(0, 0, 0, 0);
            if (s && 16 * (k + 1) - s < len) hi = *reinterpret_cast<const uint4*>(q + 16 * (k + 1));      // it holds a byte of the key
            const u64 L0 = ((u64)lo.y << 32) | lo.x, L1 = ((u64)lo.w << 32) | lo.z, H0 = ((u64)hi.y << 32) | hi.x, H1 = ((u64)hi.w << 32) | hi.z;
            const u64 a0 = s & 8 ? L1 : L0, a1 = s & 8 ? H0 : L1, a2 = s & 8 ? H1 : H0;
            u64 w0 = s8 ? (a0 >> s8) | (a1 << (64 - s8)) : a0, w1 = s8 ? (a1 >> s8) | (a2 << (64 - s8)) : a1;
            const u64 rem = len - 16 * k;
            if (rem < 8) w0 &= (1ull << (8 * rem)) - 1;
            if (rem < 16 && rem > 8) w1 &= (1ull << (8 * (rem - 8))) - 1;
            part += word_mix(w0, 2 * k);
            if (rem > 8) part += word_mix(w1, 2 * k + 1);
        }
        part += shfl_xor64(part, 1); part += shfl_xor64(part, 2); part += shfl_xor64(part, 4);
        const u64 hl = mix64(len + 0x9E3779B97F4A7C15ull) + part;
        h = g ? mix64(h + 0x632BE59BD9B4E019ull) + hl : hl;
    }
    if (in && !sub) A.hash[u] = mix64(h);
}

// ---- 3. the call's table ---------------------------------------------------------------------------------------------------------
template <u32 G>
__global__ __launch_bounds__(256) void k_dd_insert(DdInfo* info, const u8* __restrict__ text, DdArrays A) {
    if (info->status) return;
    const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
    if (u >= info->units) return;
    const u64 h = A.hash[u], mask = info->tmask, mine = DD_OCC | dd_fp(h) | u, r0 = info->r0;
    unsigned long long* T = reinterpret_cast<unsigned long long*>(A.table);
    u64 i = h & mask;
    for (u64 probe = 0; probe <= mask; probe++, i = (i + 1) & mask) {
        u64 cur = __hip_atomic_load(&T[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!cur) {
            cur = atomicCAS(&T[i], 0ull, (unsigned long long)mine);
            if (!cur) { A.slot[u] = i; return; }
        }
        if (((cur ^ mine) & ~DD_PAY) == 0) {                   // the fingerprint is a filter only: the keys decide
            const u64 v = cur & DD_PAY;                        // a unit of the slot's key (a smaller one may take its place meanwhile: the same key)
            if (v == u || units_equal<G>(text, A.ls, r0, u, v)) {
                atomicMin(&T[i], (unsigned long long)mine);
                A.slot[u] = i;
                return;
            }
        }
    }
    atomicMax(&info->status, (u32)DD_PROBE);                   // (cannot be: the table holds twice the units)
    atomicMax(&info->copy.status, (u32)DD_PROBE);
}

// ---- 4. the set, read -------------------------------------------------------------------------------------------------------------
template <u32 G>
__device__ __forceinline__ bool unit_is_key(const u8* text, const u64* ls, u64 r, const DdSetDev& S, u64 k) {
    u64 at[G], len[G];
#pragma unroll
    for (u32 g = 0; g < G; g++) { base_line(ls, r + g, &at[g], &len[g]); if (len[g] != S.klen[k * G + g]) return false; }
    u64 ao = S.koff[k];
#pragma unroll
    for (u32 g = 0; g < G; g++) { if (!lines_equal(text + at[g], S.arena + ao, len[g])) return false; ao += len[g]; }
    return true;
}
template <u32 G>
__global__ __launch_bounds__(256) void k_dd_probe(DdInfo* info, const u8* __restrict__ text, DdArrays A, DdSetDev S) {
    if (info->status) return;
    const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
    if (u >= info->units) return;
    if ((A.table[A.slot[u]] & DD_PAY) != u) return;            // the earliest unit of a key answers for all of them
    const u64 h = A.hash[u], fp = DD_OCC | dd_fp(h);
    u8 in = 0;
    u64 i = h & S.smask, probe = 0;
    for (; probe <= S.smask; probe++, i = (i + 1) & S.smask) {
        const u64 cur = S.slots[i];
        if (!cur) break;
        const u64 k = cur & DD_PAY;
        if ((cur & ~DD_PAY) == fp && k < S.keys && unit_is_key<G>(text, A.ls, info->r0 + u * G, S, k)) { in = 1; break; }
    }
    A.inset[u] = in;                                           // (a table without an empty slot cannot be: it holds twice max_keys)
}

// ---- 5. verdicts, lengths, destinations --------------------------------------------------------------------------------------------
template <u32 G>
__global__ __launch_bounds__(256) void k_dd_verdict(DdInfo* info, DdJob job, DdArrays A, u64 n) {
    if (info->status) return;
    const u32 lane = threadIdx.x & 63;
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 U = info->units, r0 = info->r0;
    const bool in = t < U;
    u64 w = 0;
    if (in) w = A.table[A.slot[t]] & DD_PAY;
    const bool known = in && job.use_set && A.inset[w];
    const bool again = in && !known && w != t;
    const bool keep = in && !known && w == t;
    const u64 mk = __ballot(known), ma = __ballot(again);
    if (!lane) {
        if (mk) atomicAdd(reinterpret_cast<unsigned long long*>(&info->n_dup_set), (unsigned long long)__popcll(mk));
        if (ma) atomicAdd(reinterpret_cast<unsigned long long*>(&info->n_dup_call), (unsigned long long)__popcll(ma));
    }
    u64 kbytes = 0;
#pragma unroll
    for (u32 g = 0; g < G; g++) {
        const u64 k = t * G + g, r = r0 + k;
        u64 len = 0;
        if (in) {
            const u64 a0 = A.ls[4 * r], a4 = A.ls[4 * r + 4];
            len = (a4 < n ? a4 : n) - a0;
            kbytes += A.ls[4 * r + 2] - A.ls[4 * r + 1] - 1;  // (below 4 GiB, as len: k_dd_hash refused the call otherwise)
        }
        if (k < A.nlens) { A.keep[k] = keep ? 1u : 0u; A.rlen[k] = keep ? (u32)len : 0u; }
    }
    if (t < A.ucap) A.kb[t] = keep && job.use_set ? (u32)kbytes : 0u;
}
// the kept records' starts and lengths, one behind the other (lens[] was zeroed)
__global__ __launch_bounds__(256) void k_dd_scatter(const DdInfo* info, DdArrays A) {
    if (info->status) return;
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    if (k >= info->nr || k >= A.nlens || !A.keep[k]) return;
    const u64 p = A.pos[k];
    A.from[p] = A.ls[4 * (info->r0 + k)];
    A.lens[p] = A.rlen[k];
}
// behind the scans: what the copy is, and whether the set holds what the call adds
__global__ void k_dd_room(DdInfo* info, DdArrays A, DdJob job, DdSetDev S) {
    if (threadIdx.x || blockIdx.x || info->status) return;
    const u64 kept = A.pos[A.nlens], nout = A.dst[A.nlens];
    info->copy.r0 = 0; info->copy.pieces = kept; info->copy.nout = nout;
    info->new_keys = job.pairs ? kept >> 1 : kept;
    info->new_bytes = job.use_set ? A.koffs[A.ucap] : 0;
    if (nout > job.out_cap) { info->status = DD_ROOM; info->copy.status = DD_ROOM; }
    else if (job.use_set && (info->new_keys > S.max_keys - S.keys || info->new_bytes > S.max_bytes - S.bytes)) { info->status = DD_NOMEM; info->copy.status = DD_NOMEM; }
    else if (!kept) info->copy.status = DD_NOTHING;
}

// ---- 6. the set, written ------------------------------------------------------------------------------------------------------------
template <u32 G>
__global__ __launch_bounds__(256) void k_dd_commit(DdInfo* info, const u8* __restrict__ text, DdArrays A, DdSetDev S) {
    if (info->status) return;
    const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
    if (u >= info->units || !A.keep[u * G]) return;
    const u64 k = S.keys + A.pos[u * G] / G;                   // the key's number in the set
    u64 ao = S.bytes + A.koffs[u];
    if (k >= S.max_keys) return;                               // (cannot be: k_dd_room)
    S.koff[k] = ao;
#pragma unroll
    for (u32 g = 0; g < G; g++) {
        u64 at, len;
        base_line(A.ls, info->r0 + u * G + g, &at, &len);
        S.klen[k * G + g] = (u32)len;
        if (ao + len > S.max_bytes) return;                    // (cannot be)
        const u8* src = text + at;
        u8* dst = S.arena + ao;
        u64 i = 0;
        for (; i < len && ((uintptr_t)(dst + i) & 7); i++) dst[i] = fold1(src[i]);
        KeyWords kw(src + i, len - i);
        for (; i + 8 <= len; i += 8) *reinterpret_cast<u64*>(dst + i) = fold8(kw.next());
        if (i < len) {
            const u64 w = fold8(kw.next());
            for (u32 b = 0; i < len; i++, b++) dst[i] = (u8)(w >> (8 * b));
        }
        ao += len;
    }
    const u64 h = A.hash[u], mine = DD_OCC | dd_fp(h) | k;
    unsigned long long* T = reinterpret_cast<unsigned long long*>(S.slots);
    u64 i = h & S.smask;
    for (u64 probe = 0; probe <= S.smask; probe++, i = (i + 1) & S.smask)
        if (!atomicCAS(&T[i], 0ull, (unsigned long long)mine)) return;
    atomicMax(&info->status, (u32)DD_PROBE);                   // (cannot be: the table holds twice max_keys)
    atomicMax(&info->copy.status, (u32)DD_PROBE);
}

template <u32 G>
void launch_units(const PairText& t, const DdArrays& A, const DdJob& job, const DdSetDev& S, DdInfo* info, hipStream_t st, bool commit) {
    const dim3 grid((u32)((A.ucap + 255) / 256));
    if (commit) { hipLaunchKernelGGL(k_dd_commit<G>, grid, dim3(256), 0, st, info, t.d, A, S); return; }
    hipLaunchKernelGGL(k_dd_hash<G>, dim3((u32)((8 * A.ucap + 255) / 256)), dim3(256), 0, st, info, t.d, A, t.n);
    hipLaunchKernelGGL(k_dd_insert<G>, grid, dim3(256), 0, st, info, t.d, A);
    if (job.use_set) hipLaunchKernelGGL(k_dd_probe<G>, grid, dim3(256), 0, st, info, t.d, A, S);
    hipLaunchKernelGGL(k_dd_verdict<G>, grid, dim3(256), 0, st, info, job, A, t.n);
}

}  // namespace

void launch_dedup(const PairText& t, const DdArrays& A, const DdJob& job, const DdSetDev& S, u8* out, DdInfo* info, hipStream_t st) {
    const QmapScratch q = qmap_scratch(t.d, t.n);
    u64* before = reinterpret_cast<u64*>(t.scratch + q.before_off);
    launch_line_starts(t, A.ls, 4 * A.cap, st);
    hipLaunchKernelGGL(k_dd_check, dim3(1), dim3(64), 0, st, info, (const u64*)before + q.nspans, t.d + t.n - 1, t.n, A.ls, A.cap, A.tcap, job);
    const u64 cw = (A.tcap + 255) / 256;
    hipLaunchKernelGGL(k_dd_clear, dim3((u32)(cw < textspan::MAX_WG ? cw : textspan::MAX_WG)), dim3(256), 0, st, (const DdInfo*)info, A.table);
    if (job.pairs) launch_units<2>(t, A, job, S, info, st, false);
    else launch_units<1>(t, A, job, S, info, st, false);
    (void)hipMemsetAsync(A.lens, 0, A.nlens * 4, st);
    launch_scan_u32(A.keep, A.pos, A.nlens, A.tmp, st);
    hipLaunchKernelGGL(k_dd_scatter, dim3((u32)((A.nlens + 255) / 256)), dim3(256), 0, st, (const DdInfo*)info, A);
    launch_scan_u32(A.lens, A.dst, A.nlens, A.tmp, st);
    if (job.use_set) launch_scan_u32(A.kb, A.koffs, A.ucap, A.tmp, st);
    hipLaunchKernelGGL(k_dd_room, dim3(1), dim3(64), 0, st, info, A, job, S);
    if (job.use_set) {
        if (job.pairs) launch_units<2>(t, A, job, S, info, st, true);
        else launch_units<1>(t, A, job, S, info, st, true);
    }
    launch_pick_copy(A.dst, A.from, t.d, job.out_cap < t.n ? job.out_cap : t.n, out, &info->copy, st);
}

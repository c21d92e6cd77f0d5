// stats.hip -- the statistics of a FASTQ text (sfq_text_stats, include/slimfastq_amd.h) from the text and its line index, while
// both are resident for an encode.  Three kernels on the caller's stream, into one zeroed accumulator (StatsAcc):
//   1. k_stats_records: what the line index alone tells, a record per lane: the record count, the sums of the four lines' lengths,
//      the shortest and longest base line, and the quality lines counted by length (cyc_n is a function of those lengths alone).
//   2. k_stats_text: the byte histograms of the base and quality lines and the per-cycle sums of the quality bytes.  A wavefront
//      takes SPAN contiguous bytes of text: it finds the line that holds the span's first byte with one 64-ary search of the
//      line index, then reads the span a ROW at a time -- one aligned 16-byte unit per lane, a load instruction covers 1 KiB of
//      contiguous text -- and carries (line number, start of the line) from unit to unit by counting the '\n' it reads: two wave
//      scans per row, no further look at the index.  A lane then knows of each of its 16 bytes the line kind (line number & 3)
//      and the position in the line.  It reads whole aligned units like crc.hip: up to 15 bytes before the text and behind it
//      are read and masked, never past the aligned unit of the last byte.
//   3. k_stats_finish: cyc_n from the length counts, seq_len_min from its complement.
// Contention: a binned file has four quality values, bases are four letters.  A lane counts RUNS of equal bytes in registers and
// adds a run to LDS when the byte changes (at the latest at the end of its span), into one of HIST_COPIES copies of the
// histograms picked by its lane number; the copies of one value lie in adjacent banks.  Quality bytes past cycle 511 are summed
// in a register.  The per-cycle sums below that are LDS adds at addresses 16 apart from lane to lane within one line.
// No global atomic sits in a per-byte loop: a workgroup adds its non-zero LDS counters to the accumulator with 64-bit global
// atomics once, at its end (the launch gives it at most FLUSH_TILES tiles).  Integer sums do not depend on their order: the
// result is deterministic.
#include "kernels.h"

namespace {

constexpr u32 ROW = 1024;                      // bytes a wavefront reads with one load instruction (64 lanes x 16)
constexpr u32 SPAN_ROWS = 16;
constexpr u32 SPAN = ROW * SPAN_ROWS;          // 16 KiB: the text a wavefront takes at a time
constexpr u32 WG_TILE = 4 * SPAN;              // 64 KiB: the four wavefronts of a workgroup
// The LDS counters and the lanes' partial sums are u32, added to the accumulator once per workgroup.  launch_text_stats gives a
// workgroup at most FLUSH_TILES tiles, i.e. FLUSH_TILES * WG_TILE = 2^22 bytes: a histogram counter stays <= 2^22 and a sum of
// quality bytes (a cyc_qsum entry, a lane's or the workgroup's tail sum) <= 255 * 2^22 < 2^30: neither can wrap.
constexpr u32 FLUSH_TILES = 64;
constexpr u32 HIST_COPIES = 8;
constexpr u32 CYC = SFQ_STATS_CYCLES;

struct StatsAcc {
    sfq_text_stats s;                          // (seq_len_min holds the largest complement of a length until k_stats_finish)
    u64 qlen[CYC + 1];                         // quality lines by length; [CYC]: that long or longer
};

__device__ __forceinline__ void add64(u64* p, u64 v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
__device__ __forceinline__ u32 wave_incl_add(u32 v, u32 lane) {
#pragma unroll
    for (u32 o = 1; o < 64; o <<= 1) { const u32 t = (u32)__shfl_up((int)v, o, 64); if (lane >= o) v += t; }
    return v;
}
__device__ __forceinline__ u32 wave_incl_max(u32 v, u32 lane) {
#pragma unroll
    for (u32 o = 1; o < 64; o <<= 1) { const u32 t = (u32)__shfl_up((int)v, o, 64); if (lane >= o && t > v) v = t; }
    return v;
}
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (u64)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

// ---- 1. the line index alone ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_stats_records(const u64* __restrict__ line_off, u64 nrec, StatsAcc* __restrict__ acc) {
    __shared__ u32 s_len[CYC + 1];
    __shared__ unsigned long long s_sum[6];    // records, the four lines' bytes, quality bytes past cycle CYC - 1
    __shared__ u32 s_min, s_max;               // ~(shortest base line), longest
    for (u32 i = threadIdx.x; i <= CYC; i += 256) s_len[i] = 0;
    if (threadIdx.x < 6) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_min = 0; s_max = 0; }
    __syncthreads();
    const u32 lane = threadIdx.x & 63;
    u64 cnt = 0, hb = 0, sb = 0, pb = 0, qb = 0, tail = 0;
    u32 mn = 0, mx = 0;
    for (u64 r0 = (u64)blockIdx.x * 256 + (threadIdx.x & ~63u); r0 < nrec; r0 += (u64)gridDim.x * 256) {       // (r0: the wavefront's first record)
        const u64 r = r0 + lane;
        const bool in = r < nrec;
        u32 bin = 0xFFFFFFFFu;
        if (in) {
            const u64 l0 = line_off[4 * r], l1 = line_off[4 * r + 1], l2 = line_off[4 * r + 2], l3 = line_off[4 * r + 3], l4 = line_off[4 * r + 4];
            const u64 hl = l1 - l0 - 1, sl = l2 - l1 - 1, pl = l3 - l2 - 1, ql = l4 - l3 - 1;
            cnt++; hb += hl; sb += sl; pb += pl; qb += ql;
            const u32 s32 = sl > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)sl;
            if (~s32 > mn) mn = ~s32;
            if (s32 > mx) mx = s32;
            if (ql > CYC) tail += ql - CYC;
            bin = ql < CYC ? (u32)ql : CYC;
        }
        // reads of one length are the rule: the lanes that agree with the first are counted with one add
        const u32 first = (u32)__builtin_amdgcn_readfirstlane((int)bin);
        const u64 same = __ballot(in && bin == first);
        if (lane == 0) atomicAdd(&s_len[first], (u32)__popcll(same));
        if (in && bin != first) atomicAdd(&s_len[bin], 1u);
    }
    cnt = wave_sum64(cnt); hb = wave_sum64(hb); sb = wave_sum64(sb); pb = wave_sum64(pb); qb = wave_sum64(qb); tail = wave_sum64(tail);
    if (lane == 0) {
        atomicAdd(&s_sum[0], (unsigned long long)cnt); atomicAdd(&s_sum[1], (unsigned long long)hb); atomicAdd(&s_sum[2], (unsigned long long)sb);
        atomicAdd(&s_sum[3], (unsigned long long)pb); atomicAdd(&s_sum[4], (unsigned long long)qb); atomicAdd(&s_sum[5], (unsigned long long)tail);
    }
    atomicMax(&s_min, mn); atomicMax(&s_max, mx);
    __syncthreads();
    for (u32 i = threadIdx.x; i <= CYC; i += 256) if (s_len[i]) add64(&acc->qlen[i], s_len[i]);
    if (threadIdx.x == 0 && s_sum[0]) {
        add64(&acc->s.n_records, s_sum[0]); add64(&acc->s.hdr_bytes, s_sum[1]); add64(&acc->s.seq_bytes, s_sum[2]);
        add64(&acc->s.plus_bytes, s_sum[3]); add64(&acc->s.qlt_bytes, s_sum[4]);
        if (s_sum[5]) add64(&acc->s.cyc_n[CYC], s_sum[5]);
        atomicMax(&acc->s.seq_len_min, s_min); atomicMax(&acc->s.seq_len_max, s_max);
    }
}

// ---- 2. the text -----------------------------------------------------------------------------------------------------------
// a run of equal bytes of one line kind, kept in registers: idx = (kind == 3) * 256 + byte, 0xFFFFFFFF = none
struct Run { u32 idx, n; };
__device__ __forceinline__ void run_flush(Run& run, u32* s_hist, u32 lane) {
    if (run.n) atomicAdd(&s_hist[run.idx * HIST_COPIES + (lane & (HIST_COPIES - 1))], run.n);
    run.n = 0;
}

// the span of the text that starts at byte s0 (16-byte aligned in memory; negative where the text starts inside its first unit)
__device__ __forceinline__ void stats_span(const u8* __restrict__ fq, i64 n, const u64* __restrict__ line_off, u64 nlines, i64 s0,
                                           u32* s_hist, u32* s_cyc, u32& tail, u32 lane) {
    if (s0 >= n) return;
    // the line that holds the span's first byte: the last entry <= sv of the index (line_off[0] = 0, line_off[nlines] = n > sv)
    const u64 sv = s0 < 0 ? 0 : (u64)s0;
    u64 lo = 0, hi = nlines;
    while (hi - lo > 1) {
        const u64 step = (hi - lo + 63) / 64;
        const u64 k = lo + lane * step;
        const bool le = k < hi && line_off[k] <= sv;
        u32 c = (u32)__popcll(__ballot(le));                   // lanes 0 .. c - 1 (the index ascends; lane 0 always)
        if (!c) c = 1;                                         // (an index that does not start at 0: stay inside it)
        const u64 nhi = lo + c * step;
        lo += (c - 1) * step;
        if (nhi < hi) hi = nhi;
    }
    u64 line = lo;
    i64 start = (i64)line_off[lo];                             // where that line starts
    Run run = { 0xFFFFFFFFu, 0 };
    for (u32 row = 0; row < SPAN_ROWS; row++) {
        const i64 rb = s0 + (i64)row * ROW;
        if (rb >= n) break;
        const i64 ub = rb + 16 * (i64)lane;                    // the lane's unit: bytes jlo <= j < jhi of it are text
        const bool live = ub < n && ub + 16 > 0;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (live) v = *reinterpret_cast<const uint4*>(fq + ub);
        const u32 jlo = ub < 0 ? (u32)(-ub) : 0u;
        const u32 jhi = !live ? 0u : (n - ub < 16 ? (u32)(n - ub) : 16u);
        const u32 w[4] = { v.x, v.y, v.z, v.w };
        u32 nl = 0;                                            // its line ends
#pragma unroll
        for (u32 j = 0; j < 16; j++) if (((w[j >> 2] >> (8 * (j & 3))) & 0xFFu) == 10u && j >= jlo && j < jhi) nl |= 1u << j;
        const u32 cnt = (u32)__popc(nl);
        const u32 key = nl ? lane * 16 + (31u - (u32)__clz(nl)) + 1 : 0u;       // behind its last line end, from the row's start
        const u32 icnt = wave_incl_add(cnt, lane), ikey = wave_incl_max(key, lane);
        u32 ekey = (u32)__shfl_up((int)ikey, 1, 64);
        if (lane == 0) ekey = 0;
        u32 ln = (u32)line + (icnt - cnt);                     // the line of the unit's first byte (its low bits: the kind) ...
        u32 pos = (u32)(ub + (i64)jlo - (ekey ? rb + (i64)ekey : start));       // ... and that byte's position in it
#pragma unroll
        for (u32 j = 0; j < 16; j++) {
            if (j < jlo || j >= jhi) continue;
            const u32 b = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            if (b == 10u) { ln++; pos = 0; continue; }
            const u32 kind = ln & 3u;
            if (kind & 1u) {                                   // a base line (1) or a quality line (3)
                const u32 idx = ((kind >> 1) << 8) | b;
                if (idx != run.idx) { run_flush(run, s_hist, lane); run.idx = idx; }
                run.n++;
                if (kind == 3u) {
                    if (pos < CYC) atomicAdd(&s_cyc[pos], b);
                    else tail += b;
                }
            }
            pos++;
        }
        line += (u32)__shfl((int)icnt, 63, 64);
        const u32 last = (u32)__shfl((int)ikey, 63, 64);
        if (last) start = rb + (i64)last;
    }
    run_flush(run, s_hist, lane);
}

__global__ __launch_bounds__(256) void k_stats_text(const u8* __restrict__ base /* 16-byte aligned */, u32 mis /* the text starts at base + mis */,
                                                    u64 n, const u64* __restrict__ line_off, u64 nlines, u64 ntiles, StatsAcc* __restrict__ acc) {
    __shared__ u32 s_hist[512 * HIST_COPIES];
    __shared__ u32 s_cyc[CYC + 1];
    for (u32 i = threadIdx.x; i < 512 * HIST_COPIES; i += 256) s_hist[i] = 0;
    for (u32 i = threadIdx.x; i <= CYC; i += 256) s_cyc[i] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u8* fq = base + mis;
    u32 tail = 0;
    for (u64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x)               // (at most FLUSH_TILES of them)
        stats_span(fq, (i64)n, line_off, nlines, (i64)(tile * WG_TILE + wave * SPAN) - (i64)mis, s_hist, s_cyc, tail, lane);
    const u32 t = (u32)wave_sum64(tail);
    if (lane == 0 && t) atomicAdd(&s_cyc[CYC], t);
    __syncthreads();
    for (u32 i = threadIdx.x; i < 512; i += 256) {
        u32 c = 0;
#pragma unroll
        for (u32 k = 0; k < HIST_COPIES; k++) c += s_hist[i * HIST_COPIES + k];
        if (c) add64(i < 256 ? &acc->s.seq_hist[i] : &acc->s.qlt_hist[i - 256], c);
    }
    for (u32 i = threadIdx.x; i <= CYC; i += 256) if (s_cyc[i]) add64(&acc->s.cyc_qsum[i], s_cyc[i]);
}

// ---- 3. cyc_n[c] = the quality lines longer than c; the shortest base line ---------------------------------------------------
__global__ __launch_bounds__(CYC) void k_stats_finish(StatsAcc* __restrict__ acc) {
    const u32 c = threadIdx.x;
    u64 longer = 0;
    for (u32 l = c + 1; l <= CYC; l++) longer += acc->qlen[l];
    acc->s.cyc_n[c] = longer;
    if (c == 0) acc->s.seq_len_min = acc->s.n_records ? ~acc->s.seq_len_min : 0u;
}

}  // namespace

u64 text_stats_acc_bytes() { return sizeof(StatsAcc); }

void launch_text_stats(const u8* fq, u64 n, const u64* line_off, u64 nrec, void* acc, hipStream_t st) {
    StatsAcc* a = reinterpret_cast<StatsAcc*>(acc);
    const u64 rwg = (nrec + 255) / 256;
    hipLaunchKernelGGL(k_stats_records, dim3((u32)(rwg < 1024 ? rwg : 1024)), dim3(256), 0, st, line_off, nrec, a);
    const u32 mis = (u32)((uintptr_t)fq & 15);
    const u64 ntiles = (mis + n + WG_TILE - 1) / WG_TILE;
    const u64 least = (ntiles + FLUSH_TILES - 1) / FLUSH_TILES;                  // workgroups, so that none gets more than FLUSH_TILES tiles
    const u64 twg = ntiles < 2048 ? ntiles : (least > 2048 ? least : 2048);
    hipLaunchKernelGGL(k_stats_text, dim3((u32)twg), dim3(256), 0, st, fq - mis, mis, n, line_off, 4 * nrec, ntiles, a);
    hipLaunchKernelGGL(k_stats_finish, dim3(1), dim3(CYC), 0, st, a);
}

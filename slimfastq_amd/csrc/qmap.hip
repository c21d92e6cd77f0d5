// qmap.hip -- quality binning: every byte of every 4th line of a FASTQ text (line number & 3 == 3, counted from the start of the
// buffer, the '\n' excluded) through a 256-byte table, in place (sfq_map_qualities, sfq_ctx_set_quality_map).  The pass runs BEFORE
// an encode frames the text and on buffers no encode ever sees, so it has no line index: it counts the line ends itself.
//   1. k_qmap_count: the '\n' bytes of every SPAN of the text, a wavefront per span: one aligned 16-byte unit per lane, a load
//      instruction covers a ROW of 1 KiB of contiguous text.  One u32 per span.
//   2. launch_scan_u32 (frame.hip) over the span counts: the line ends in front of every span.
//   3. k_qmap_apply: a wavefront per span again.  Per row one wave scan of the units' '\n' counts gives the line number of every
//      unit's first byte; the kinds of its 16 bytes follow from the unit's own '\n' mask by two prefix parities (the count of line
//      ends mod 4, bit-sliced over the 16 positions -- no loop over the bytes).  Bytes of kind 3 that are not '\n' go through the
//      table, which every workgroup keeps in LDS (256 bytes; a ds_read_u8 per byte, only in units that hold a quality byte).
//      A unit is stored only where a byte of it changed, a row without a quality byte is left after the scan, without a lookup
//      or a store.  A workgroup adds its changed bytes to the call's 64-bit counter once, at its end: an integer sum, the same in
//      any order.
// Spans are laid from the aligned 16-byte unit that holds the text's first byte.  Like crc.hip and stats.hip the pass READS whole
// aligned units: up to 15 bytes in front of the text and behind it, inside the units of its first and last byte.  It WRITES
// nothing outside [text, text + n): interior units are stored whole, the (at most two) ragged units byte by byte.
// The table never moves a '\n' and never makes one (sfq_quality_map_check), so the counts of step 1 hold while step 3 writes.
#include "kernels.h"
#include "dev_lines.h"

namespace {

using namespace textspan;          // dev_lines.h: ROW, SPAN, the unit loads, newline_mask, the wave sums

// bit j: the parity of the bits below j of a 16-bit mask
__device__ __forceinline__ u32 parity_below(u32 m) {
    u32 x = m << 1;
    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8;
    return x & 0xFFFFu;
}
// ---- 1. line ends per span ---------------------------------------------------------------------------------------------------
template <bool EDGE>
__device__ __forceinline__ u32 count_span(const u8* fq, i64 n, i64 s0, u32 lane) {
    u32 c = 0;
    for (u32 r0 = 0; r0 < SPAN_ROWS; r0 += BATCH) {
        uint4 v[BATCH]; u32 vm[BATCH];
        load_batch<EDGE>(fq, n, s0 + (i64)r0 * ROW, lane, v, vm);
#pragma unroll
        for (u32 k = 0; k < BATCH; k++) c += (u32)__popc(newline_mask(v[k]) & vm[k]);
    }
    return wave_sum(c);
}
__global__ __launch_bounds__(256) void k_qmap_count(const u8* __restrict__ base /* 16-byte aligned */, u32 mis /* the text starts at base + mis */,
                                                    u64 n, u64 nspans, u32* __restrict__ cnt) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u8* fq = base + mis;
    for (u64 s = (u64)blockIdx.x * 4 + wave; s < nspans; s += (u64)gridDim.x * 4) {
        const i64 s0 = (i64)(s * SPAN) - (i64)mis;
        const u32 c = (s0 >= 0 && s0 + (i64)SPAN <= (i64)n) ? count_span<false>(fq, (i64)n, s0, lane) : count_span<true>(fq, (i64)n, s0, lane);
        if (lane == 0) cnt[s] = c;
    }
}

// ---- 3. the table over the quality lines -------------------------------------------------------------------------------------
// line: the line ends in front of the span (its low two bits are all that is used); returns the lane's changed bytes
template <bool EDGE>
__device__ __forceinline__ u32 apply_span(u8* fq, i64 n, i64 s0, u32 line, const u8* s_lut, u32 lane) {
    u32 changed = 0;
    for (u32 r0 = 0; r0 < SPAN_ROWS; r0 += BATCH) {
        uint4 v[BATCH]; u32 vm[BATCH];
        load_batch<EDGE>(fq, n, s0 + (i64)r0 * ROW, lane, v, vm);
#pragma unroll
        for (u32 k = 0; k < BATCH; k++) {
            const u32 nl = newline_mask(v[k]) & vm[k];
            const u32 cnt = (u32)__popc(nl);
            const u32 icnt = wave_incl_add(cnt, lane);
            const u32 ln = line + (icnt - cnt);                // the line of the unit's first byte
            line += (u32)__shfl((int)icnt, 63, 64);
            // kind of byte j = (ln + line ends below j) & 3, as two bit planes over j
            const u32 p0 = parity_below(nl);                   // bit 0 of the count below j
            const u32 p1 = parity_below(nl & p0);              // bit 1: the line ends that carry
            const u32 l0 = (ln & 1u) ? 0xFFFFu : 0u, l1 = (ln & 2u) ? 0xFFFFu : 0u;
            const u32 qm = (p0 ^ l0) & (p1 ^ l1 ^ (p0 & l0)) & ~nl & vm[k];      // kind 3, not '\n', text
            if (!__ballot(qm != 0)) continue;                  // no quality byte in the row
            if (!qm) continue;
            const u32 w[4] = { v[k].x, v[k].y, v[k].z, v[k].w };
            u32 o[4], dm = 0;
#pragma unroll
            for (u32 i = 0; i < 4; i++) {
                u32 m = 0;
#pragma unroll
                for (u32 b = 0; b < 4; b++) m |= (u32)s_lut[(w[i] >> (8 * b)) & 0xFFu] << (8 * b);
                u32 keep = ((qm >> (4 * i)) & 0xFu) * 0x00204081u;           // bit b -> bits 0 / 8 / 16 / 24 of a byte mask ...
                keep = (keep & 0x01010101u) * 0xFFu;                         // ... -> whole bytes
                o[i] = (m & keep) | (w[i] & ~keep);
                dm |= gather_bit7(nonzero_bytes(o[i] ^ w[i])) << (4 * i);
            }
            if (!dm) continue;
            changed += (u32)__popc(dm);
            i64 ub;
            (void)unit_mask<EDGE>(s0 + (i64)(r0 + k) * ROW, n, lane, &ub);
            if (!EDGE || vm[k] == 0xFFFFu) *reinterpret_cast<uint4*>(fq + ub) = make_uint4(o[0], o[1], o[2], o[3]);
            else {                                             // a ragged unit: the changed bytes alone (all of them text: dm is a part of vm)
#pragma unroll
                for (u32 j = 0; j < 16; j++) if ((dm >> j) & 1u) fq[ub + j] = (u8)(o[j >> 2] >> (8 * (j & 3)));
            }
        }
    }
    return changed;
}
__global__ __launch_bounds__(256) void k_qmap_apply(u8* base /* 16-byte aligned */, u32 mis, u64 n, u64 nspans, const u64* __restrict__ before,
                                                    const u8* __restrict__ lut, u64* __restrict__ changed) {
    __shared__ u8 s_lut[256];
    __shared__ unsigned long long s_changed;
    s_lut[threadIdx.x] = lut[threadIdx.x];
    if (threadIdx.x == 0) s_changed = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u8* fq = base + mis;
    u64 ch = 0;
    for (u64 s = (u64)blockIdx.x * 4 + wave; s < nspans; s += (u64)gridDim.x * 4) {
        const i64 s0 = (i64)(s * SPAN) - (i64)mis;
        const u32 line = (u32)before[s];
        ch += (s0 >= 0 && s0 + (i64)SPAN <= (i64)n) ? apply_span<false>(fq, (i64)n, s0, line, s_lut, lane) : apply_span<true>(fq, (i64)n, s0, line, s_lut, lane);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) ch += (u64)__shfl_xor((unsigned long long)ch, o, 64);
    if (lane == 0 && ch) atomicAdd(&s_changed, (unsigned long long)ch);
    __syncthreads();
    if (threadIdx.x == 0 && s_changed) atomicAdd(reinterpret_cast<unsigned long long*>(changed), s_changed);
}

}  // namespace

QmapScratch qmap_scratch(const u8* d, u64 n) {
    QmapScratch q;
    const u64 mis = (u64)((uintptr_t)d & 15);
    q.nspans = (mis + n + SPAN - 1) / SPAN;
    q.cnt_off = 0;
    q.before_off = (q.nspans * 4 + 15) & ~15ull;
    q.tmp_off = q.before_off + (q.nspans + 1) * 8;
    q.bytes = q.tmp_off + (q.nspans / 1024 + 2) * 8;
    return q;
}

void launch_newline_counts(const u8* d, u64 n, u32* cnt, hipStream_t st) {
    if (!n) return;
    const u32 mis = (u32)((uintptr_t)d & 15);
    const u64 nspans = (mis + n + SPAN - 1) / SPAN, tiles = (nspans + 3) / 4;
    hipLaunchKernelGGL(k_qmap_count, dim3((u32)(tiles < MAX_WG ? tiles : MAX_WG)), dim3(256), 0, st, d - mis, mis, n, nspans, cnt);
}

void launch_quality_map(u8* d, u64 n, const u8* d_lut, u8* scratch, u64* d_changed, hipStream_t st) {
    if (!n) return;
    const QmapScratch q = qmap_scratch(d, n);
    const u32 mis = (u32)((uintptr_t)d & 15);
    u32* cnt = reinterpret_cast<u32*>(scratch + q.cnt_off);
    u64* before = reinterpret_cast<u64*>(scratch + q.before_off);
    u64* tmp = reinterpret_cast<u64*>(scratch + q.tmp_off);
    const u64 tiles = (q.nspans + 3) / 4;
    const u32 wg = (u32)(tiles < MAX_WG ? tiles : MAX_WG);
    launch_newline_counts(d, n, cnt, st);
    launch_scan_u32(cnt, before, q.nspans, tmp, st);
    hipLaunchKernelGGL(k_qmap_apply, dim3(wg), dim3(256), 0, st, d - mis, mis, n, q.nspans, (const u64*)before, d_lut, d_changed);
}

// mrg.hip -- merged mates: every pair (X, Y) of a range of records that has an accepted offset d becomes ONE record -- line 1 of X, the
// I = d + Lb consensus bases of a and b', line 3 of X, the I combined qualities -- and the range's other pairs follow whole
// (slimfastq_amd.h "merged mates"; sfq_merge_pairs, sfq_ctx_set_merge).  The first pass behind a decode that COMPUTES bytes; the others
// move them.  Text to text:
//   1. launch_overlap_search (ovl.hip): the line starts, the rules, ins[k] and mm[k] of every pair of the range.
//   2. k_mrg_plan: a lane a pair: ins[k] decides.  mlen[k] = the merged record's bytes, ulen[k] = the unmerged pair's, flag[k]; the
//      report's counts in registers over many pairs, one wave sum and atomic per wavefront and counter, the histogram in LDS.
//   3. launch_scan_u32 three times: mdst (its last entry is merged_bytes), udst (counted from merged_bytes), mpos (the merged pairs in
//      front of a pair: list[mpos[k]] = k compacts them, k - mpos[k] numbers the others).  k_mrg_room (one lane) checks the output's
//      room: nothing is written before it.
//   4. k_mrg_list: the compacted list, and the unmerged pairs as pieces (a pair is one piece: both records whole).
//   5. k_mrg_write, the hot kernel: ONE WAVEFRONT A MERGED RECORD, grid-stride over the list.
//      Bases and qualities: lane l takes positions 8 l .. 8 l + 7 of a round of 512 (I <= 994: two rounds at most).  a and line 4 of X
//      come through load8, the aligned 8-byte words that hold them; b and line 4 of Y counted from the line's END and byte-swapped, so
//      that byte i of the word is position j + i of b'.  Which bytes are bases is one SWAR mask a word; the rule itself is byte
//      arithmetic in registers.  The eight result bytes of either line go to the wavefront's LDS as one aligned u64, the '\n' behind
//      position I - 1 with them.  No lane walks a line byte by byte through memory.
//      Stores: the record is four segments -- line 1, the merged bases, line 3, the merged qualities.  Lines 1 and 3 stream from the
//      text (any length), the other two from LDS.  Neighbouring records are written by other wavefronts at the same time, so every
//      segment goes out as the aligned 16-byte units that lie WHOLLY inside it, a lane a unit, and single bytes in front of and behind
//      them: no word that another record shares is read, modified and written.
//   6. launch_pick_copy_at: the unmerged pairs, to out + merged_bytes.
// Every index into ls[] and the per-pair arrays is checked against the arrays' room, as in ovl.hip.
#include "kernels.h"
#include "dev_lines.h"
#include "dev_wave.h"
#include "dev_pieces.h"

namespace {
using namespace textspan;

constexpr u32 NHIST = 2 * OVL_MAX_LEN + 1;
constexpr u32 STAGE = (2 * OVL_MAX_LEN + 16) / 8;              // u64 words of a staged line: 995 bytes and what a unit's shift reads behind them

// ---- 2. the plan -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mrg_plan(MrgInfo* info, MrgArrays A, u64 n) {
    if (info->o.stop) return;
    __shared__ u32 hist[NHIST];
    for (u32 i = threadIdx.x; i < NHIST; i += 256) hist[i] = 0;
    __syncthreads();
    const u32 lane = threadIdx.x & 63;
    const u64 r0 = info->o.r0, npairs = info->o.nr >> 1, P = A.cap / 2 + 1;
    u32 pairs = 0, skipped = 0, merged = 0;
    u64 bases_in = 0, bases_m = 0, mism = 0;
    bool big = false;
    for (u64 k = (u64)blockIdx.x * 256 + threadIdx.x; k < P; k += (u64)gridDim.x * 256) {
        u32 ml = 0, ul = 0, fl = 0;
        const u64 l = 4 * (r0 + 2 * k);
        if (k < npairs && l + 8 <= 4 * A.cap) {
            const u64 x0 = A.ls[l], a1 = A.ls[l + 1], x2 = A.ls[l + 2], x3 = A.ls[l + 3], b1 = A.ls[l + 5], y2 = A.ls[l + 6], e = A.ls[l + 8];
            const u32 ins = A.ins[k];
            pairs++;
            bases_in += (x2 - a1 - 1) + (y2 - b1 - 1);
            if (ins == OVL_SKIPPED) skipped++;
            else atomicAdd(&hist[ins < NHIST ? ins : 0], 1u);
            u64 len;
            if (ins != 0 && ins != OVL_SKIPPED) {
                fl = 1; merged++; mism += A.mm[k]; bases_m += ins;
                len = (a1 - x0) + (x3 - x2) + 2 * ((u64)ins + 1);
                ml = (u32)len;
            } else {
                len = (e < n ? e : n) - x0;
                ul = (u32)len;
            }
            big |= len >> 32 != 0;
        }
        A.mlen[k] = ml; A.ulen[k] = ul; A.flag[k] = fl;
    }
    if (__any(big) && !lane) { info->o.toolong = 1; info->o.stop = 1; }
    add_to(&info->o.n_pairs, wave_sum(pairs), lane);
    add_to(&info->o.n_skipped, wave_sum(skipped), lane);
    add_to(&info->n_merged, wave_sum(merged), lane);
    add_to(&info->o.bases_in, wave_sum64(bases_in), lane);
    add_to(&info->bases_merged, wave_sum64(bases_m), lane);
    add_to(&info->o.mismatches, wave_sum64(mism), lane);
    __syncthreads();
    for (u32 i = threadIdx.x; i < NHIST; i += 256)
        if (hist[i]) atomicAdd(reinterpret_cast<unsigned long long*>(&info->o.hist[i]), (unsigned long long)hist[i]);
}
// behind the scans: the two parts' sizes, and what the piece copy is
__global__ void k_mrg_room(MrgInfo* info, MrgArrays A, u64 out_cap) {
    if (threadIdx.x || blockIdx.x) return;
    const u64 P = A.cap / 2 + 1;
    if (!info->o.stop) {
        const u64 npairs = info->o.nr >> 1;
        info->merged_bytes = A.mdst[P];
        info->out_bytes = A.mdst[P] + A.udst[P];
        info->o.copy.r0 = 0; info->o.copy.pieces = npairs - A.mpos[P]; info->o.copy.nout = A.udst[P];
        if (info->out_bytes > out_cap) { info->o.status = OVL_ROOM; info->o.stop = 1; }
    }
    info->o.copy.status = info->o.stop ? info->o.stop : info->o.copy.pieces ? 0u : MRG_NOTHING;
}
// ---- 4. the list and the pieces ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mrg_list(const MrgInfo* info, MrgArrays A) {
    if (info->o.stop) return;
    const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 npairs = info->o.nr >> 1, P = A.cap / 2 + 1;
    if (k >= P || k > npairs) return;
    const u64 m = A.mpos[k], u = k - m;
    if (k == npairs) { A.dst[u] = A.udst[k]; return; }         // behind the last piece: the part's end
    const u64 l = 4 * (info->o.r0 + 2 * k);
    if (A.flag[k]) A.list[m] = k;
    else if (l <= 4 * A.cap) { A.from[u] = A.ls[l]; A.dst[u] = A.udst[k]; }
}

// ---- 5. the merged records -----------------------------------------------------------------------------------------------------------
// bit 7 of every byte of w that is one of ACGTacgt
__device__ __forceinline__ u64 base_bytes(u64 w) {
    const u32 x[2] = { (u32)w | 0x20202020u, (u32)(w >> 32) | 0x20202020u };
    u32 m[2];
#pragma unroll
    for (u32 i = 0; i < 2; i++)
        m[i] = ~(nonzero_bytes(x[i] ^ 0x61616161u) & nonzero_bytes(x[i] ^ 0x63636363u) & nonzero_bytes(x[i] ^ 0x67676767u) & nonzero_bytes(x[i] ^ 0x74747474u)) & 0x80808080u;
    return ((u64)m[1] << 32) | m[0];
}
// len bytes to out: the aligned 16-byte units wholly inside [out, out + len) a lane each, single bytes in front of and behind them.
// get16(o): the source's bytes o .. o + 15, asked for only where o + 16 <= len; get1(o): its byte o < len
template <class Get16, class Get1>
__device__ __forceinline__ void wave_put(u8* out, u64 len, u32 lane, Get16 get16, Get1 get1) {
    const u64 mis = (16 - ((uintptr_t)out & 15)) & 15;
    const u64 head = mis < len ? mis : len;
    const u64 body = (len - head) & ~15ull, tail = len - head - body;
    if (lane < head) out[lane] = get1((u64)lane);
    for (u64 o = head + 16 * (u64)lane; o < head + body; o += 16 * 64) *reinterpret_cast<uint4*>(out + o) = get16(o);
    if (lane < tail) out[head + body + lane] = get1(head + body + lane);
}
__device__ __forceinline__ uint4 two_words(u64 lo, u64 hi) { return make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32)); }
// text[at, at + len) to out
__device__ __forceinline__ void put_text(u8* out, const u8* text, u64 n, u64 at, u64 len, u32 lane) {
    wave_put(out, len, lane,
             [&](u64 o) { return two_words(load8(text, (i64)(at + o), n), load8(text, (i64)(at + o + 8), n)); },
             [&](u64 o) { return text[at + o]; });
}
// a staged line's first len bytes to out
__device__ __forceinline__ void put_staged(u8* out, const u64* stage, u64 len, u32 lane) {
    wave_put(out, len, lane,
             [&](u64 o) {
                 const u32 q = (u32)(o >> 3), sh = 8 * ((u32)o & 7u);
                 const u64 w0 = stage[q], w1 = stage[q + 1], w2 = stage[q + 2];
                 return sh ? two_words((w0 >> sh) | (w1 << (64 - sh)), (w1 >> sh) | (w2 << (64 - sh))) : two_words(w0, w1);
             },
             [&](u64 o) { return reinterpret_cast<const u8*>(stage)[o]; });
}
__device__ __forceinline__ void wave_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

__global__ __launch_bounds__(256) void k_mrg_write(MrgInfo* info, const u8* __restrict__ text, u64 n, MrgJob J, MrgArrays A, u8* __restrict__ out) {
    if (info->o.stop) return;
    __shared__ u64 stage[4][2][STAGE];
    const u32 lane = threadIdx.x & 63, wave = rfl(threadIdx.x >> 6);
    u64* sb = stage[wave][0];
    u64* sq = stage[wave][1];
    const u64 r0 = info->o.r0, M = info->n_merged, P = A.cap / 2 + 1;
    const u32 qb = J.qual_base, top = 126 - qb;
    u32 xw = 0, yw = 0;
    for (u64 i = (u64)blockIdx.x * 4 + wave; i < M && i < P; i += (u64)gridDim.x * 4) {
        const u64 k = A.list[i], l = 4 * (r0 + 2 * k);
        if (k >= P || l + 8 > 4 * A.cap) continue;
        const u64 x0 = A.ls[l], a1 = A.ls[l + 1], x2 = A.ls[l + 2], x3 = A.ls[l + 3], b1 = A.ls[l + 5], y2 = A.ls[l + 6], y3 = A.ls[l + 7];
        const u32 La = (u32)(x2 - a1 - 1), Lb = (u32)(y2 - b1 - 1), I = A.ins[k];
        if (La > OVL_MAX_LEN || Lb > OVL_MAX_LEN || I > La + Lb || I < 1) continue;      // (cannot be: the search's own bounds)
        const int d = (int)I - (int)Lb;
        for (u32 base = 0; base <= I; base += 512) {
            const u32 p0 = base + 8 * lane;
            if (p0 > I) continue;
            const int j0 = (int)p0 - d;                        // position p0 of the merged read is position j0 of b'
            u64 wx = 0, wqx = 0, wy = 0, wqy = 0;
            if (p0 < La) { wx = load8(text, (i64)(a1 + p0), n); wqx = load8(text, (i64)(x3 + p0), n); }
            if (j0 + 7 >= 0 && j0 < (int)Lb) {                 // b[Lb - 8 - j0 .. Lb - 1 - j0], the last byte first
                wy = __builtin_bswap64(load8(text, (i64)b1 + (i64)Lb - 8 - (i64)j0, n));
                wqy = __builtin_bswap64(load8(text, (i64)y3 + (i64)Lb - 8 - (i64)j0, n));
            }
            const u64 bx = base_bytes(wx), by = base_bytes(wy);
            u64 ob = 0, oq = 0;
#pragma unroll
            for (u32 t = 0; t < 8; t++) {
                const u32 p = p0 + t, s = 8 * t;
                const u32 x = (u32)(wx >> s) & 255u, qx = (u32)(wqx >> s) & 255u, yb = (u32)(wy >> s) & 255u, qy = (u32)(wqy >> s) & 255u;
                const bool in_a = p < La, in_b = (u32)(j0 + (int)t) < Lb;
                const bool vx = (bx >> s) & 0x80u, vy = (by >> s) & 0x80u;
                const u32 y = vy ? (0x43414754u >> (8 * ((yb >> 1) & 3u))) & 255u : yb;        // A 0, C 1, T 2, G 3 -> T G A C
                u32 b = x, q = qx;
                if (in_a && in_b) {
                    if (vx && vy) {
                        if ((x & ~0x20u) == y) q = qx > qy ? qx : qy;
                        else {
                            const u32 df = qx > qy ? qx - qy : qy - qx, fl = df > 2 ? df : 2u;
                            q = qb + (fl < top ? fl : top);
                            if (qx >= qy) xw++; else { b = y; yw++; }
                        }
                    } else if (vy) { b = y; q = qy; }
                } else if (in_b) { b = y; q = qy; }
                if (p == I) b = q = '\n';
                ob |= (u64)b << s; oq |= (u64)q << s;
            }
            sb[p0 >> 3] = ob; sq[p0 >> 3] = oq;
        }
        wave_lds_fence();
        u8* o = out + A.mdst[k];
        put_text(o, text, n, x0, a1 - x0, lane); o += a1 - x0;
        put_staged(o, sb, (u64)I + 1, lane); o += I + 1;
        put_text(o, text, n, x2, x3 - x2, lane); o += x3 - x2;
        put_staged(o, sq, (u64)I + 1, lane);
        wave_lds_fence();
    }
    add_to(&info->n_x_wins, wave_sum(xw), lane);
    add_to(&info->n_y_wins, wave_sum(yw), lane);
}

}  // namespace

void launch_merge(const PairText& t, const MrgArrays& A, const MrgJob& job, u8* out, MrgInfo* info, hipStream_t st) {
    const u64 P = A.cap / 2 + 1;
    const dim3 per_pair((u32)((P + 255) / 256)), per_wave((u32)((P + 3) / 4));
    const OvlArrays S{ A.ls, A.ins, A.mm, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, A.cap };
    const OvlJob search{ job.r0, job.nr, job.out_cap, job.min_ov, job.max_mm, job.max_pct, 0 };
    launch_overlap_search(t, S, search, &info->o, st);
    hipLaunchKernelGGL(k_mrg_plan, dim3(per_pair.x < MAX_WG ? per_pair.x : MAX_WG), dim3(256), 0, st, info, A, t.n);
    launch_scan_u32(A.mlen, A.mdst, P, A.tmp, st);
    launch_scan_u32(A.ulen, A.udst, P, A.tmp, st);
    launch_scan_u32(A.flag, A.mpos, P, A.tmp, st);
    hipLaunchKernelGGL(k_mrg_room, dim3(1), dim3(64), 0, st, info, A, job.out_cap);
    hipLaunchKernelGGL(k_mrg_list, per_pair, dim3(256), 0, st, (const MrgInfo*)info, A);
    hipLaunchKernelGGL(k_mrg_write, dim3(per_wave.x < 16 * MAX_WG ? per_wave.x : 16 * MAX_WG), dim3(256), 0, st, info, t.d, t.n, job, A, out);
    launch_pick_copy_at(A.dst, A.from, t.d, job.out_cap < t.n ? job.out_cap : t.n, out, &info->merged_bytes, &info->o.copy, st);
}

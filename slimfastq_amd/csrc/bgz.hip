// bgz.hip -- BGZF members (the SAM specification's blocked gzip) of pieces of a device text: sfq_bgzf_deflate and the decode
// entries' last pass.  Member m holds the piece text[mb[m], mb[m + 1]) of at most 65280 bytes:
//     18 header bytes | one raw deflate stream (one dynamic block, or one stored block where that is smaller) | CRC-32 | ISIZE
//   1. crc.hip's range pass over the pieces (launched by the host in front of this file's kernels).
//   2. k_bgz_deflate: a wavefront per member, persistent over the members.  The piece is staged in LDS with the misalignment it has
//      in memory (whole 16-byte units are loaded).  The parse takes 64 positions at a time, a lane each: the lane looks its four
//      bytes up in a table of last positions (4096 u16 entries in LDS) that holds only positions from BEFORE the chunk, extends the
//      match by comparing LDS dwords (up to 258 bytes, a match may run into itself), and a wave-uniform loop over the ballot of
//      the lanes that found a match resolves the greedy parse, carrying "covered until" into the next chunk.  Then all positions
//      of the chunk are entered into the table: lanes with the same slot write until the slot holds the largest of them, so the
//      table is a function of the text.  Tokens go to the workgroup's slot in device memory, their symbols are counted with LDS
//      atomics.  Lanes rank the used symbols (a rank sort on count | symbol); lane 0 builds the two codes and the code-length
//      header (bgz_code.h).  If the dynamic block is larger than the piece + 5 bytes the member is stored.  Otherwise the piece's
//      LDS is zeroed, lane 0 writes the header bits, a wave scan of the tokens' bit lengths places them and the lanes OR their
//      bits into the words (disjoint bits: the order does not matter).  The member goes to its 64 KiB slot of the scratch buffer.
//   3. launch_scan_u32 / k_bgz_room: the members' sizes are scanned; the room check sets the copy's status.
//   4. pick.hip's piece copy compacts the members into the output.
// Nothing in a member depends on another member, on the piece's address or on the order in which lanes or workgroups run.
#include "kernels.h"
#include "bgz_code.h"

namespace {
using namespace bgz;

constexpr u32 TEXT_WORDS = (PIECE + 16 + 16) / 4;      // the piece behind up to 15 bytes of its first unit, and a dword of slack for the compares
constexpr u32 HASH_N = 1u << HASH_BITS;
constexpr u32 NONE = 0xFFFFu;

struct Lds {
    u32 f_ll[288], f_d[32];         // histograms
    u32 c_ll[288], c_d[32];         // codes
    u8  l_ll[288], l_d[32];         // code lengths
    u32 f_cl[20], c_cl[20]; u8 l_cl[20];
    u32 blc[16], nxt[16];
    u32 info[8];                    // lane 0 to all: 0 stored, 1 header bits, 2 deflate bytes
    u16 hash[HASH_N];               // last positions; later the code construction's arrays (Work below)
    u32 text[TEXT_WORDS];           // the staged piece; later the deflate stream.  (The small arrays lie in front: below 64 KiB a
                                    // ds instruction's own offset reaches them, behind it every address wants a register.)
};
// the arrays of the code construction, laid over the hash table (8192 bytes)
struct Work { u32 key[288]; u32 iw[288]; u16 pl[288]; u16 pi[288]; u16 dep[288]; u16 seq[320]; };
static_assert(sizeof(Work) <= HASH_N * 2, "the code construction works in the hash table's LDS");
static_assert(sizeof(Lds) <= 80 * 1024, "two workgroups a CU");

__device__ __forceinline__ u32 ld32(const u32* t, u32 pos) {              // four bytes at any byte position
    const u32 i = pos >> 2, lo = t[i], hi = t[i + 1];
    return (u32)((((u64)hi << 32) | lo) >> (8 * (pos & 3u)));
}
__device__ __forceinline__ u32 wave_incl_add32(u32 v, u32 lane) {
#pragma unroll
    for (u32 o = 1; o < 64; o <<= 1) { const u32 t = (u32)__shfl_up((int)v, o, 64); if (lane >= o) v += t; }
    return v;
}

// the used symbols of f[0, nsym) into key[], ascending: every lane ranks its symbols against all
__device__ u32 rank_sort(const u32* f, u32 nsym, u32* key, u32 lane) {
    u32 n = 0;
    for (u32 s0 = 0; s0 < nsym; s0 += 64) {
        const u32 s = s0 + lane;
        const u32 fs = s < nsym ? f[s] : 0u;
        if (fs) {
            const u32 k = (fs << 9) | s;
            u32 r = 0;
            for (u32 j = 0; j < nsym; j++) { const u32 fj = f[j]; r += (fj && ((fj << 9) | j) < k) ? 1u : 0u; }
            key[r] = k;
        }
        n += (u32)__popcll(__ballot(fs != 0));
    }
    return n;
}

__global__ __launch_bounds__(64) void k_bgz_deflate(const u8* __restrict__ text, const u64* __restrict__ mb, u32 n_members, const u32* __restrict__ crc,
                                                    u32* __restrict__ toks /* [gridDim.x][PIECE] */, u8* __restrict__ slots, u32* __restrict__ msize,
                                                    u32* __restrict__ n_stored) {
    __shared__ Lds L;
    const u32 lane = threadIdx.x;
    u32* tok = toks + (u64)blockIdx.x * PIECE;
    Work& W = *reinterpret_cast<Work*>(L.hash);
    volatile u16* hv = L.hash;                                 // (a lane reads back what the lanes wrote: no value is kept in a register)
    for (u32 m = blockIdx.x; m < n_members; m += gridDim.x) {
        const u64 S = mb[m];
        const u32 n = (u32)(mb[m + 1] - S);                    // 1 .. PIECE
        const u8* a = text + S;
        const u32 mis = (u32)((uintptr_t)a & 15u);
        const u32 end = mis + n;                               // positions count from the first unit's first byte
        __syncthreads();                                       // (the member before is out of LDS)
        {
            const uint4* src = reinterpret_cast<const uint4*>(a - mis);
            const u32 nun = (end + 15) >> 4;
            for (u32 u = lane; u < nun; u += 64) {
                const uint4 v = src[u];
                L.text[4 * u] = v.x; L.text[4 * u + 1] = v.y; L.text[4 * u + 2] = v.z; L.text[4 * u + 3] = v.w;
            }
            for (u32 i = 4 * nun + lane; i < 4 * nun + 8 && i < TEXT_WORDS; i += 64) L.text[i] = 0;
            for (u32 i = lane; i < HASH_N / 2; i += 64) reinterpret_cast<u32*>(L.hash)[i] = 0xFFFFFFFFu;
            for (u32 i = lane; i < 288; i += 64) { L.f_ll[i] = 0; L.l_ll[i] = 0; }
            if (lane < 32) { L.f_d[lane] = 0; L.l_d[lane] = 0; }
            if (lane < 20) { L.f_cl[lane] = 0; L.l_cl[lane] = 0; }
        }
        __syncthreads();
        // ---- the parse
        u32 covered = mis, ntok = 0;
        for (u32 p0 = mis; p0 < end; p0 += CHUNK) {
            const u32 p = p0 + lane;
            const bool can = p + MIN_MATCH <= end;
            const u32 h = can ? hash4(ld32(L.text, p)) : 0u;
            u32 len = 0, dist = 0;
            if (covered < p0 + CHUNK && can && p >= covered) {
                const u32 c = hv[h];
                if (c != NONE && p - c <= MAX_DIST) {
                    const u32 maxlen = end - p < MAX_MATCH ? end - p : MAX_MATCH;
                    while (len < maxlen) {
                        const u32 x = ld32(L.text, c + len) ^ ld32(L.text, p + len);
                        if (x) { len += (u32)(__ffs((int)x) - 1) >> 3; break; }
                        len += 4;
                    }
                    if (len > maxlen) len = maxlen;
                    if (len < MIN_MATCH) len = 0;
                    dist = p - c;
                }
            }
            const u64 mm = __ballot(len != 0);
            u32 cur = covered > p0 ? covered - p0 : 0u;            // the chunk's first position that no token covers yet
            u64 cov = cur >= 64 ? ~0ull : (1ull << cur) - 1ull, starts = 0;
            while (cur < 64) {
                const u64 rest = mm & (~0ull << cur);
                if (!rest) break;
                const u32 j = (u32)__ffsll((long long)rest) - 1u;
                const u32 e = j + (u32)__shfl((int)len, (int)j, 64);       // the match covers lanes j + 1 .. e - 1
                starts |= 1ull << j;
                if (j + 1 < 64) cov |= (e >= 64 ? ~0ull : (1ull << e) - 1ull) & (~0ull << (j + 1));
                cur = e;
            }
            if (p0 + cur > covered) covered = p0 + cur;
            if (covered < p0 + CHUNK) covered = p0 + CHUNK;
            const bool is_tok = p < end && !((cov >> lane) & 1ull);
            const bool is_match = (starts >> lane) & 1ull;
            const u64 tm = __ballot(is_tok);
            if (is_tok) {
                u32 t;
                if (is_match) {
                    t = TOK_MATCH | ((dist - 1) << 8) | (len - 3);
                    u32 s, nx, xv;
                    len_sym(len - 3, &s, &nx, &xv); atomicAdd(&L.f_ll[s], 1u);
                    dist_sym(dist - 1, &s, &nx, &xv); atomicAdd(&L.f_d[s], 1u);
                } else {
                    t = (L.text[p >> 2] >> (8 * (p & 3u))) & 255u;
                    atomicAdd(&L.f_ll[t], 1u);
                }
                tok[ntok + (u32)__popcll(tm & ((1ull << lane) - 1ull))] = t;
            }
            ntok += (u32)__popcll(tm);
            // the chunk's positions into the table: the slot ends up with the largest of the lanes that share it
            bool go = can;
            while (__any(go)) {
                if (go) hv[h] = (u16)p;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                if (go) go = hv[h] < p;
            }
        }
        if (lane == 0) L.f_ll[EOB] = 1;
        __syncthreads();
        // ---- the codes
        const u32 n_ll = rank_sort(L.f_ll, N_LL, W.key, lane);
        __syncthreads();
        const HuffWork HW{ W.key, W.iw, W.pl, W.pi, W.dep, L.blc, L.nxt };
        if (lane == 0) { huff_lengths(HW, n_ll, 15, L.l_ll); huff_codes(L.l_ll, N_LL, 15, HW, L.c_ll); }
        __syncthreads();
        const u32 n_d = rank_sort(L.f_d, N_D, W.key, lane);
        __syncthreads();
        if (lane == 0) {
            if (n_d) huff_lengths(HW, n_d, 15, L.l_d);
            huff_codes(L.l_d, N_D, 15, HW, L.c_d);
            u32 hlit = N_LL, hdist = N_D;
            while (hlit > 257 && !L.l_ll[hlit - 1]) hlit--;
            while (hdist > 1 && !L.l_d[hdist - 1]) hdist--;
            const u32 nseq = cl_sequence(L.l_ll, hlit, L.l_d, hdist, W.seq, L.f_cl);
            u32 ncl = huff_sort_serial(L.f_cl, N_CL, HW);
            if (ncl == 1) {                                        // a complete code needs two symbols: a second one of one bit that is never sent
                const u32 s = W.key[0] & 511u;
                L.l_cl[s] = 1; L.l_cl[s ? 0 : 1] = 1;
            } else huff_lengths(HW, ncl, 7, L.l_cl);
            huff_codes(L.l_cl, N_CL, 7, HW, L.c_cl);
            const u32 hclen = cl_count(L.l_cl);
            const u32 hbits = header_bits(W.seq, nseq, L.l_cl, hclen);
            u64 bits = hbits;
            for (u32 s = 0; s < N_LL; s++) {
                u32 nx = 0;
                if (s >= 265 && s < 285) nx = (s - 261) >> 2;
                bits += (u64)L.f_ll[s] * (L.l_ll[s] + nx);
            }
            for (u32 s = 0; s < N_D; s++) bits += (u64)L.f_d[s] * (L.l_d[s] + (s >= 4 ? (s >> 1) - 1 : 0u));
            const u32 bytes = (u32)((bits + 7) >> 3);
            L.info[0] = bytes > n + 5 ? 1u : 0u;
            L.info[1] = hbits; L.info[2] = bytes;
            L.info[3] = hlit; L.info[4] = hdist; L.info[5] = nseq; L.info[6] = hclen;
        }
        __syncthreads();
        const bool stored = L.info[0] != 0;
        const u32 dbytes = stored ? n + 5 : L.info[2];
        u8* out = slots + (u64)m * SLOT + SLOT_LEAD;
        u32* dw = reinterpret_cast<u32*>(out + 18);               // dword aligned: SLOT_LEAD + 18 = 20
        const u32 nw = (dbytes + 3) >> 2;
        if (stored) {
            // 01 | LEN | ~LEN | the piece, as dwords: word j holds stream bytes 4 j .. 4 j + 3, the text begins at stream byte 5
            for (u32 j = lane; j < nw; j += 64) {
                u32 w;
                if (j >= 2) w = ld32(L.text, mis + 4 * j - 5);
                else {
                    const u32 t0 = ld32(L.text, mis);              // text bytes 0 .. 3
                    w = j == 0 ? (1u | (n << 8) | ((~n & 0xFFu) << 24)) : (((~n >> 8) & 0xFFu) | (t0 << 8));
                }
                dw[j] = w;
            }
        } else {
            const u32 hbits = L.info[1];
            __syncthreads();
            for (u32 i = lane; i < TEXT_WORDS; i += 64) L.text[i] = 0;
            __syncthreads();
            if (lane == 0) {
                BitW bw{ L.text, 0, 0, 0 };
                header_write(bw, L.info[3], L.info[4], W.seq, L.info[5], L.l_cl, L.c_cl, L.info[6]);
                bw.flush();
            }
            __syncthreads();
            u32 at = hbits;                                        // the next token's first bit
            for (u32 t0 = 0; t0 <= ntok; t0 += 64) {               // (token ntok is the end of the block)
                const u32 i = t0 + lane;
                u64 v = 0; u32 nb = 0;
                if (i < ntok) token_bits(tok[i], L.c_ll, L.c_d, &v, &nb);
                else if (i == ntok) { const u32 c = L.c_ll[EOB]; v = c & 0xFFFFu; nb = c >> 16; }
                const u32 incl = wave_incl_add32(nb, lane);
                const u32 b = at + incl - nb;
                at += (u32)__shfl((int)incl, 63, 64);
                if (nb) {
                    const u32 sh = b & 31u, wi = b >> 5;
                    const u64 lo = v << sh;
                    const u32 hi = sh ? (u32)(v >> (64 - sh)) : 0u;
                    atomicOr(&L.text[wi], (u32)lo);
                    if ((u32)(lo >> 32)) atomicOr(&L.text[wi + 1], (u32)(lo >> 32));
                    if (hi) atomicOr(&L.text[wi + 2], hi);
                }
            }
            __syncthreads();
            for (u32 j = lane; j < nw; j += 64) dw[j] = L.text[j];
        }
        // header and trailer, bytes: the trailer lies wherever the stream ends
        const u32 total = 18 + dbytes + 8;
        if (lane < 18) {
            const u32 bs = total - 1;
            const u32 hw[5] = { 0x04088B1Fu, 0x00000000u, 0x0006FF00u, 0x00024342u, bs & 0xFFFFu };
            u32 w = 0;
#pragma unroll
            for (u32 q = 0; q < 5; q++) if ((lane >> 2) == q) w = hw[q];
            out[lane] = (u8)(w >> (8 * (lane & 3u)));
        }
        __syncthreads();                                           // (the stream's last dword may reach into the trailer's bytes: it goes first)
        if (lane < 8) {
            const u32 w = lane < 4 ? crc[m] : n;
            out[18 + dbytes + lane] = (u8)(w >> (8 * (lane & 3u)));
        }
        if (lane == 0) { msize[m] = total; if (stored) atomicAdd(n_stored, 1u); }
    }
}

// behind the scan of the sizes: what the copy is
__global__ void k_bgz_room(PickInfo* info, const u64* __restrict__ dst, u32 n_members, u64 out_cap) {
    if (threadIdx.x || blockIdx.x) return;
    info->r0 = 0; info->pieces = n_members; info->nout = dst[n_members];
    info->status = info->nout > out_cap ? (u32)PICK_ROOM : (u32)PICK_OK;
}
// from[m] = where member m lies in the scratch buffer
__global__ __launch_bounds__(256) void k_bgz_from(u64* __restrict__ from, u32 n_members) {
    const u32 m = blockIdx.x * 256 + threadIdx.x;
    if (m < n_members) from[m] = (u64)m * SLOT + SLOT_LEAD;
}

}  // namespace

u32 bgz_workgroups(u32 n_members, u32 cus) { const u32 g = 2 * cus; return n_members < g ? n_members : g; }
u64 bgz_token_bytes(u32 workgroups) { return (u64)workgroups * PIECE * 4; }
u64 bgz_slot_bytes(u32 n_members) { return (u64)n_members * SLOT + 32; }

void launch_bgz_deflate(const u8* text, const u64* mb, u32 n_members, const u32* crc, u32 workgroups, u32* toks, u8* slots, u32* msize, u64* from,
                        u64* dst, u64* scan_tmp, u32* n_stored, u64 out_cap, u8* out, PickInfo* info, hipStream_t st) {
    hipLaunchKernelGGL(k_bgz_deflate, dim3(workgroups), dim3(64), 0, st, text, mb, n_members, crc, toks, slots, msize, n_stored);
    hipLaunchKernelGGL(k_bgz_from, dim3((n_members + 255) / 256), dim3(256), 0, st, from, n_members);
    launch_scan_u32(msize, dst, n_members, scan_tmp, st);
    hipLaunchKernelGGL(k_bgz_room, dim3(1), dim3(64), 0, st, info, (const u64*)dst, n_members, out_cap);
    const u64 most = (u64)n_members * (PIECE + 31);
    launch_pick_copy(dst, from, slots, out_cap < most ? out_cap : most, out, info, st);
}

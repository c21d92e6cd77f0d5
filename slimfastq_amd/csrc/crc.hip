// crc.hip -- CRC-32 (IEEE 802.3: reflected, polynomial 0xEDB88320, init and final XOR 0xFFFFFFFF; Python's zlib.crc32) of
// contiguous ranges [bounds[i], bounds[i+1]) of one device buffer.  The checksums of the block format (INTEGRATION.md 4,
// "blk.crc") and the sfq_crc32 entry point.
//
// The pass works on the RAW CRC (zero init, no final XOR), which is linear over GF(2):
//     raw(A || B) = raw(A) * x^(8|B|) mod P  ^  raw(B),      zlib(M) = raw(M) ^ (0xFFFFFFFF * x^(8|M|) mod P) ^ 0xFFFFFFFF.
// Values are zlib's bit order: bit 31 is the coefficient of x^0.  Zero bytes in front of a message add nothing to its raw CRC,
// which lets a pass read whole aligned 16-byte units and clear the bytes outside its range.
//   1. k_crc_tiles: the raw CRC of every whole 4 KiB tile of the span (tiles laid from the first 16-byte boundary of the
//      span), a wavefront per tile: a lane reads one 16-byte unit per 1 KiB row (each load instruction covers 1 KiB of
//      contiguous text), folds it in with slicing-by-16 (sixteen 256-entry tables in LDS, picked by the ds_read offset) and
//      shifts its running value by 1 KiB per row (four byte tables); the 64 lanes' values are brought to the tile's end by a
//      constant per lane and XORed together across the wavefront.
//   2. k_crc_groups: the raw CRC of every 64 whole tiles (256 KiB), a wavefront per group.
//   3. k_crc_ranges: a wavefront per range: its ragged ends (pieces under two tiles, read as masked units), the tiles up to
//      the first group border, the groups, the tiles after the last -- each run folded like the rows of step 1 -- joined
//      with shifts by x^(8n).  Only step 3 knows the ranges: the work of steps 1-2 does not depend on their number, and
//      step 3 reads a 3.7 GB range as 14 000 group values.
#include "kernels.h"

namespace {

constexpr u32 CRC_POLY = 0xEDB88320u;
constexpr u32 TILE = 4096;                 // bytes per tile (step 1)
constexpr u32 GROUP = 64;                  // tiles per group (step 2)
// table layout (words), built once per context on the host (crc_build_tables)
constexpr u32 T_SLICE = 0;                 // [16][256]: raw CRC of byte b followed by m zero bytes
constexpr u32 T_SH_ROW = 4096;             // [4][256]: multiply by x^(8*1024)       (a row of 64 units)
constexpr u32 T_SH_TILES = 5120;           // [4][256]: multiply by x^(8*64*TILE)    (64 tiles)
constexpr u32 T_SH_GROUPS = 6144;          // [4][256]: multiply by x^(8*64*64*TILE) (64 groups)
constexpr u32 T_LANE_UNIT = 7168;          // [64]: x^(8*16*(63-i))
constexpr u32 T_LANE_TILE = 7232;          // [64]: x^(8*TILE*(63-i))
constexpr u32 T_LANE_GROUP = 7296;         // [64]: x^(8*GROUP*TILE*(63-i))
constexpr u32 T_POW = 7360;                // [64]: x^(8*2^k)
constexpr u32 T_INV = 7424;                // [16]: x^(-8*p)
constexpr u32 T_WORDS = 7440;
constexpr u32 LDS_TILES = T_SH_TILES;      // what step 1 keeps in LDS (20 KiB)
constexpr u32 LDS_RANGES = T_LANE_UNIT;    // what step 3 keeps in LDS (28 KiB)

// a * b mod P (zlib's multmodp)
__host__ __device__ inline u32 mulp(u32 a, u32 b) {
    u32 p = 0;
#pragma unroll 8
    for (int i = 0; i < 32; i++) {
        p ^= (0u - (a >> 31)) & b;
        a <<= 1;
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
// x^(8n) mod P from the powers x^(8*2^k)
__host__ __device__ inline u32 x8n(const u32* pw, u64 n) {
    u32 p = 0x80000000u;
    for (int k = 0; n; n >>= 1, k++)
        if (n & 1) p = mulp(pw[k], p);
    return p;
}

// ---- device ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ u32 wave_xor(u32 v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v ^= __shfl_xor(v, o);
    return v;
}
// c * K through the four byte tables of K
__device__ __forceinline__ u32 shift_tab(const u32* t, u32 c) {
    return t[c & 0xFFu] ^ t[256 + ((c >> 8) & 0xFFu)] ^ t[512 + ((c >> 16) & 0xFFu)] ^ t[768 + (c >> 24)];
}
// raw CRC of the 16 bytes of v (byte j of the unit is followed by 15 - j bytes)
__device__ __forceinline__ u32 slice16(const u32* s, uint4 v) {
    const u32 w[4] = { v.x, v.y, v.z, v.w };
    u32 c = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) c ^= s[(15 - j) * 256 + ((w[j >> 2] >> (8 * (j & 3))) & 0xFFu)];
    return c;
}
__device__ __forceinline__ void load_tables(u32* lds, const u32* tab, u32 words) {
    for (u32 i = threadIdx.x; i < words; i += blockDim.x) lds[i] = tab[i];
    __syncthreads();
}

// step 1: raw CRC of whole tiles [o + t*TILE, o + (t+1)*TILE), o 16-byte aligned
__global__ __launch_bounds__(256) void k_crc_tiles(const u8* __restrict__ o, u64 ntiles, u32* __restrict__ tile_crc, const u32* __restrict__ tab) {
    __shared__ u32 s[LDS_TILES];
    load_tables(s, tab, LDS_TILES);
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 lk = tab[T_LANE_UNIT + lane];
    for (u64 t = (u64)blockIdx.x * 4 + wave; t < ntiles; t += (u64)gridDim.x * 4) {
        const uint4* p = reinterpret_cast<const uint4*>(o + t * TILE) + lane;
        uint4 v[TILE / 1024];
#pragma unroll
        for (u32 j = 0; j < TILE / 1024; j++) v[j] = p[64 * j];
        u32 acc = 0;
#pragma unroll
        for (u32 j = 0; j < TILE / 1024; j++) acc = shift_tab(s + T_SH_ROW, acc) ^ slice16(s, v[j]);
        const u32 c = wave_xor(mulp(lk, acc));
        if (lane == 0) tile_crc[t] = c;
    }
}

// step 2: raw CRC of GROUP consecutive tiles
__global__ __launch_bounds__(256) void k_crc_groups(const u32* __restrict__ tile_crc, u64 ngroups, u32* __restrict__ grp_crc, const u32* __restrict__ tab) {
    const u32 lane = threadIdx.x & 63;
    const u64 g = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= ngroups) return;
    const u32 c = wave_xor(mulp(tab[T_LANE_TILE + lane], tile_crc[g * GROUP + lane]));
    if (lane == 0) grp_crc[g] = c;
}

// The raw CRC of m consecutive items of one size whose raw CRCs are c[0..m): lane i folds the items m - 64 (K - k) + i, k < K
// (the last 64 end on lanes 0..63), stepping by 64 items (step table), then its value is brought to the run's end (lane table).
__device__ u32 run_crc(const u32* __restrict__ c, u64 m, const u32* step, const u32* __restrict__ lane_tab, u32 lane) {
    if (!m) return 0;
    const u64 K = (m + 63) / 64;
    const i64 first = (i64)m - (i64)(64 * K) + (i64)lane;
    u32 acc = 0;
    for (u64 k = 0; k < K; k += 8) {
        u32 v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const i64 idx = first + (i64)(64 * (k + j));
            v[j] = (k + j < K && idx >= 0) ? c[idx] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) if (k + j < K) acc = shift_tab(step, acc) ^ v[j];
    }
    return wave_xor(mulp(lane_tab[lane], acc));
}

// raw CRC of the bytes [a, e) (e - a < 2 * TILE + 16): the 16-byte units that cover them, the bytes outside cleared (the
// leading ones add nothing; the trailing pad is divided out)
__device__ u32 piece_crc(const u8* a, const u8* e, const u32* s, const u32* __restrict__ tab, u32 lane) {
    if (e <= a) return 0;
    const uintptr_t ua = (uintptr_t)a & ~(uintptr_t)15, ue = ((uintptr_t)e + 15) & ~(uintptr_t)15;
    const i64 nunits = (i64)((ue - ua) / 16);
    const i64 K = (nunits + 63) / 64;
    u32 acc = 0;
    for (i64 k = 0; k < K; k++) {
        const i64 u = nunits - 64 * (K - k) + (i64)lane;
        u32 c = 0;
        if (u >= 0) {
            const uintptr_t ub = ua + 16 * (uintptr_t)u;
            uint4 v = *reinterpret_cast<const uint4*>(ub);
            const i64 lo = (i64)((uintptr_t)a - ub), hi = (i64)((uintptr_t)e - ub);       // keep bytes lo <= q < hi
            if (lo > 0 || hi < 16) {
                u32 w[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                for (int q = 0; q < 16; q++)
                    if (q < lo || q >= hi) w[q >> 2] &= ~(0xFFu << (8 * (q & 3)));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            c = slice16(s, v);
        }
        acc = shift_tab(s + T_SH_ROW, acc) ^ c;
    }
    const u32 r = wave_xor(mulp(tab[T_LANE_UNIT + lane], acc));
    return mulp(tab[T_INV + (u32)(ue - (uintptr_t)e)], r);
}

// step 3: a wavefront per range; range n_ranges (whole != 0) is the span [bounds[0], bounds[n_ranges])
__global__ __launch_bounds__(256) void k_crc_ranges(const u8* __restrict__ d, const u64* __restrict__ bounds, u32 n_ranges, u32 whole,
                                                    const u8* o, u64 ntiles, const u32* __restrict__ tile_crc, const u32* __restrict__ grp_crc,
                                                    u32* __restrict__ out, const u32* __restrict__ tab) {
    __shared__ u32 s[LDS_RANGES];
    load_tables(s, tab, LDS_RANGES);
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32* pw = tab + T_POW;
    for (u64 r = (u64)blockIdx.x * 4 + wave; r < (u64)n_ranges + whole; r += (u64)gridDim.x * 4) {
        const u64 S = bounds[r < n_ranges ? r : 0], E = bounds[r < n_ranges ? r + 1 : n_ranges];
        if (E <= S) { if (lane == 0) out[r] = 0; continue; }
        const u8* a = d + S;
        const u8* e = d + E;
        // whole tiles inside the range: [ta, tb)
        const u64 ta = a <= o ? 0 : ((u64)(a - o) + TILE - 1) / TILE;
        u64 tb = e <= o ? 0 : (u64)(e - o) / TILE;
        if (tb > ntiles) tb = ntiles;
        u32 R;
        if (tb <= ta) R = piece_crc(a, e, s, tab, lane);
        else {
            const u8* ea = o + ta * TILE;
            const u8* eb = o + tb * TILE;
            R = piece_crc(a, ea, s, tab, lane);
            const u64 ga = (ta + GROUP - 1) / GROUP, gb = tb / GROUP;
            if (ga < gb) {
                const u64 m1 = ga * GROUP - ta, mg = gb - ga, m2 = tb - gb * GROUP;
                R = mulp(x8n(pw, m1 * TILE), R) ^ run_crc(tile_crc + ta, m1, s + T_SH_TILES, tab + T_LANE_TILE, lane);
                R = mulp(x8n(pw, mg * GROUP * TILE), R) ^ run_crc(grp_crc + ga, mg, s + T_SH_GROUPS, tab + T_LANE_GROUP, lane);
                R = mulp(x8n(pw, m2 * TILE), R) ^ run_crc(tile_crc + gb * GROUP, m2, s + T_SH_TILES, tab + T_LANE_TILE, lane);
            } else {
                R = mulp(x8n(pw, (tb - ta) * TILE), R) ^ run_crc(tile_crc + ta, tb - ta, s + T_SH_TILES, tab + T_LANE_TILE, lane);
            }
            R = mulp(x8n(pw, (u64)(e - eb)), R) ^ piece_crc(eb, e, s, tab, lane);
        }
        R ^= mulp(x8n(pw, E - S), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;       // zlib's pre- and post-conditioning
        if (lane == 0) out[r] = R;
    }
}

// bounds of the blocks of a call from a record offset table: block b starts at offs[b * stride] (b > 0)
__global__ __launch_bounds__(256) void k_crc_block_bounds(const u64* __restrict__ offs, u64 stride, u32 nblocks, u64 total, u64* __restrict__ bounds) {
    const u32 b = blockIdx.x * 256 + threadIdx.x;
    if (b > nblocks) return;
    bounds[b] = b == 0 ? 0 : b == nblocks ? total : offs[(u64)b * stride];
}

// ---- host -----------------------------------------------------------------------------------------------------------------

u32 x_inv(u32 p) {                          // p / x mod P: the step b -> (b >> 1) ^ (POLY if b & 1) run backwards
    return (p & 0x80000000u) ? (((p ^ CRC_POLY) << 1) | 1u) : (p << 1);
}
void byte_tables(u32 k, u32* t) {           // t[j * 256 + b] = (b << 8j) * k
    for (u32 j = 0; j < 4; j++)
        for (u32 b = 0; b < 256; b++) t[j * 256 + b] = mulp(k, b << (8 * j));
}

}  // namespace

void crc_build_tables(u32* t) {
    for (u32 b = 0; b < 256; b++) {
        u32 c = b;
        for (int i = 0; i < 8; i++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
        t[T_SLICE + b] = c;
    }
    for (u32 m = 1; m < 16; m++)
        for (u32 b = 0; b < 256; b++) {
            const u32 c = t[T_SLICE + (m - 1) * 256 + b];
            t[T_SLICE + m * 256 + b] = (c >> 8) ^ t[T_SLICE + (c & 0xFFu)];
        }
    u32* pw = t + T_POW;
    pw[0] = 0x00800000u;                                                         // x^8
    for (int k = 1; k < 64; k++) pw[k] = mulp(pw[k - 1], pw[k - 1]);
    byte_tables(x8n(pw, 1024), t + T_SH_ROW);
    byte_tables(x8n(pw, 64ull * TILE), t + T_SH_TILES);
    byte_tables(x8n(pw, 64ull * GROUP * TILE), t + T_SH_GROUPS);
    for (u32 i = 0; i < 64; i++) {
        t[T_LANE_UNIT + i] = x8n(pw, 16ull * (63 - i));
        t[T_LANE_TILE + i] = x8n(pw, (u64)TILE * (63 - i));
        t[T_LANE_GROUP + i] = x8n(pw, (u64)GROUP * TILE * (63 - i));
    }
    u32 inv = 0x80000000u;
    for (u32 p = 0; p < 16; p++) {
        t[T_INV + p] = inv;
        for (int i = 0; i < 8; i++) inv = x_inv(inv);
    }
}
u32 crc_table_words() { return T_WORDS; }

u32 crc32_combine_host(u32 crc_a, u32 crc_b, u64 len_b) {
    struct Powers { u32 w[64]; };
    static const Powers pw = [] {                // (a function-local static: its first initialisation is thread-safe)
        Powers p;
        p.w[0] = 0x00800000u;                    // x^8
        for (int k = 1; k < 64; k++) p.w[k] = mulp(p.w[k - 1], p.w[k - 1]);
        return p;
    }();
    return mulp(x8n(pw.w, len_b), crc_a) ^ crc_b;
}

CrcScratch crc_scratch_words(u64 lo, u64 hi, const u8* d) {
    CrcScratch w;
    const uintptr_t o = ((uintptr_t)(d + lo) + 15) & ~(uintptr_t)15;
    const uintptr_t e = (uintptr_t)(d + hi);
    w.ntiles = e > o ? (u64)(e - o) / TILE : 0;
    w.ngroups = w.ntiles / GROUP;
    return w;
}

void launch_crc32(const u8* d, const u64* d_bounds, u32 n_ranges, u32 whole, u64 lo, u64 hi, u32* tile_crc, u32* grp_crc, u32* out,
                  const u32* tab, hipStream_t st) {
    const CrcScratch w = crc_scratch_words(lo, hi, d);
    const u8* o = reinterpret_cast<const u8*>(((uintptr_t)(d + lo) + 15) & ~(uintptr_t)15);
    if (w.ntiles) {
        const u64 wg = (w.ntiles + 3) / 4 < 2048 ? (w.ntiles + 3) / 4 : 2048;
        hipLaunchKernelGGL(k_crc_tiles, dim3((u32)wg), dim3(256), 0, st, o, w.ntiles, tile_crc, tab);
    }
    if (w.ngroups) hipLaunchKernelGGL(k_crc_groups, dim3((u32)((w.ngroups + 3) / 4)), dim3(256), 0, st, (const u32*)tile_crc, w.ngroups, grp_crc, tab);
    const u64 nr = (u64)n_ranges + whole;
    if (nr) {
        const u64 wg = (nr + 3) / 4 < 1024 ? (nr + 3) / 4 : 1024;
        hipLaunchKernelGGL(k_crc_ranges, dim3((u32)wg), dim3(256), 0, st, d, d_bounds, n_ranges, whole, o, w.ntiles,
                           (const u32*)tile_crc, (const u32*)grp_crc, out, tab);
    }
}

void launch_crc_block_bounds(const u64* offs, u64 stride, u32 nblocks, u64 total, u64* bounds, hipStream_t st) {
    hipLaunchKernelGGL(k_crc_block_bounds, dim3((nblocks + 1 + 255) / 256), dim3(256), 0, st, offs, stride, nblocks, total, bounds);
}

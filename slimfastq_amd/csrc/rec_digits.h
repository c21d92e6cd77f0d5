// rec_digits.h -- the token step's short decimal fields (chains.hip nw_tok), four digits a step, and a number's symbols in closed form.
// Plain C++, so that a host program can run them over every short field (scratch/host_rec_digits_test.cpp).
//
// A field of at most nine bytes lies in at most three dwords of its header's staged column.  The three dwords that END with the field's
// last byte are read -- never one before the column's first, never one behind the dword of the field's last byte --, shifted so that the
// last byte becomes the window's last, and the bytes in front of the field are masked to zero by its length: nine digit places, the
// field right-aligned in them, zeros in front.  Per dword then
//   * c ^ '0' is 0 .. 9 for a digit and 10 or more for every other byte: "all digits" is one carry test on four bytes at once;
//   * d0 d1 d2 d3 (d0 in the low byte, the most significant) fold by multiply-and-mask: y * 10 + (y >> 8) has d0 d1 and d2 d3 as two
//     numbers below 100 in bytes 0 and 2, and t * 100 + (t >> 16) their number below 10000 in its low sixteen bits.
// No step depends on the field's length but through a mask: there is no loop whose trip count differs from lane to lane.
#pragma once
#include "dev_common.h"

struct RdField {
    u32 value;               // the digits' number (below 10^9); whatever where !plain
    u32 plain;               // 1: every byte of the field is a decimal digit (an empty field: yes)
    u32 lead;                // 0: the first byte is no '0'; 1: "0", "0d..."; 3: "00..." (where !plain: whatever)
};
// 0x80 in every byte of y that is 10 or more (no carry leaves a byte: 0x7f + 0x76 < 0x100)
__device__ __forceinline__ u32 rd_not_digit(u32 y) { return (((y & 0x7f7f7f7fu) + 0x76767676u) | y) & 0x80808080u; }
// four digit values, the most significant in the low byte, as their number
__device__ __forceinline__ u32 rd_fold4(u32 y) {
    const u32 t = (y * 10u + (y >> 8)) & 0x00ff00ffu;
    return (t * 100u + (t >> 16)) & 0xffffu;
}
// the low 32 bits of hi:lo shifted right by sh bits, sh = 8 .. 32
__device__ __forceinline__ u32 rd_funnel(u32 hi, u32 lo, u32 sh) { return (u32)(((((u64)hi) << 32) | lo) >> sh); }
// The field of len <= 9 bytes at byte off of the column tw (dwords, little endian; dword (off + len - 1) / 4 and those before it are the column's).
__device__ __forceinline__ RdField rd_parse9(const u32* tw, u32 off, u32 len) {
    const u32 last = off + len - 1u;                                         // (an empty field at offset 0: every byte below is masked)
    const u32 q = len && last >= 4u ? last >> 2 : 0u;                        // the dword of the last byte, but never before the column
    const u32 sh = 8u * ((last & 3u) + 1u);
    const u32 x2 = tw[q], x1 = tw[q >= 1u ? q - 1u : 0u], x0 = tw[q >= 2u ? q - 2u : 0u];
    // digit places 0 .. 8, the field's last byte in place 8: place 0 alone, places 1 .. 4 (a dword), places 5 .. 8 (a dword)
    const u32 m2 = len >= 4u ? ~0u : len ? ~0u << (8u * (4u - len)) : 0u;
    const u32 m1 = len >= 8u ? ~0u : len > 4u ? ~0u << (8u * (8u - len)) : 0u;
    const u32 y2 = (rd_funnel(x2, x1, sh) ^ 0x30303030u) & m2;
    const u32 y1 = (rd_funnel(x1, x0, sh) ^ 0x30303030u) & m1;
    const u32 y0 = len == 9u ? ((x0 >> (sh - 8u)) & 0xffu) ^ 0x30u : 0u;
    RdField r;
    r.plain = (rd_not_digit(y2) | rd_not_digit(y1)) == 0u && y0 <= 9u ? 1u : 0u;
    r.value = y0 * 100000000u + rd_fold4(y1) * 10000u + rd_fold4(y2);
    // zero places in front: 9 - len of them are not the field's
    const u64 y21 = ((u64)y2 << 32) | y1;
    const u32 nz = y0 ? 0u : y21 ? 1u + ((u32)__builtin_ctzll(y21) >> 3) : 9u;
    r.lead = (nz + len >= 10u ? 1u : 0u) | (nz + len >= 11u ? 2u : 0u);      // (one byte: nz <= 9, so bit 1 stays clear)
    return r;
}

// PowerRangerU::put_u's symbols (dev_rec_lane.h put_u_rows) in closed form: n of them on rows row0 + row[j]
//   n = 1: num;  2: 0x80 | num >> 8, num & 0xff;  6: 0xff 0xfe + 4 LE bytes on rows 2 .. 5;  10: 0xff 0xff + 8 LE bytes on rows 6 .. 13
__device__ __forceinline__ u32 rd_u_count(u64 num) { return num <= 0x7fu ? 1u : num < 0x7ffeu ? 2u : num < (1ull << 32) ? 6u : 10u; }
__device__ __forceinline__ u32 rd_u_sym0(u32 n, u64 num) { return n == 1u ? (u32)num : n == 2u ? (0x80u | (u32)(num >> 8)) & 0xffu : 0xffu; }
__device__ __forceinline__ u32 rd_u_sym1(u32 n, u64 num) { return n == 2u ? (u32)num & 0xffu : n == 6u ? 0xfeu : 0xffu; }

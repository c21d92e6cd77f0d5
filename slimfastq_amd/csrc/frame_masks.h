// frame_masks.h -- k_frame's byte tests, a dword at a time, and the gather of their flags into one 16-bit mask per 16-byte piece.
// Plain C++ but for one builtin, so that a host program can run them over every dword (scratch/host_frame_masks_test.cpp).
//
// These run for every dword of the text, and their masks are what a workgroup of k_frame keeps in LDS:
//   * a test flags a byte with ONE bit, 0x80 (0x40: odd_flags), and leaves every other bit of the dword 0;
//   * the tests for a given byte flag the bytes that DIFFER (ne_flags, nbang_flags): an exact "differs" is the carry of one add
//     joined with the byte's own top bit -- two instructions a dword (v_xad_u32, v_and_or_b32) once the dword's low seven bits
//     and top bits are split, which every test of the dword shares --, an exact "equals" needs a complement on top.  The
//     masks of those tests are kept complemented, and complemented back where they are read: once per 64 bytes;
//   * the flags of four dwords become sixteen mask bits by dot products with the weights 1, 2, 4 .. 128 (gather16): four
//     v_dot4_u32_u8, a shift and a shift-or, no multiply.
#pragma once
#include "dev_common.h"

// a's four bytes times b's four bytes, summed, plus c (v_dot4_u32_u8)
__device__ __forceinline__ u32 dot4_u8(u32 a, u32 b, u32 c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, c, false);
#else
    return c + (a & 0xffu) * (b & 0xffu) + ((a >> 8) & 0xffu) * ((b >> 8) & 0xffu) + ((a >> 16) & 0xffu) * ((b >> 16) & 0xffu) + (a >> 24) * (b >> 24);
#endif
}
// Bit 4 d + i of the result = flag bit BIT of byte i of dword d (fx, fy, fz, fw = d 0 .. 3); every other bit of the dwords must be 0.
// (A half's sum is at most 255 << BIT: no carry leaves its sixteen bits, none enters the other half's.)
template <u32 BIT>
__device__ __forceinline__ u32 gather16(u32 fx, u32 fy, u32 fz, u32 fw) {
    const u32 lo = dot4_u8(fy, 0x80402010u, dot4_u8(fx, 0x08040201u, 0u));
    const u32 hi = dot4_u8(fw, 0x80402010u, dot4_u8(fz, 0x08040201u, 0u));
    return (lo >> BIT) | (hi << (8u - BIT));
}
// a dword of text split once for all its tests
struct TextDword {
    u32 w;                                                 // the four bytes
    u32 lo7;                                               // ... their low seven bits
    u32 top;                                               // ... their top bits
    __device__ __forceinline__ explicit TextDword(u32 x) : w(x), lo7(x & 0x7f7f7f7fu), top(x & 0x80808080u) {}
};
// 0x80 where the byte DIFFERS from the one c4 repeats four times (c4's bytes below 0x80).  Per byte: (lo7 ^ c) + 0x7f is at most
// 0xfe -- no carry into the next byte -- and has bit 7 set unless lo7 == c; a byte of 0x80 and more differs by its top bit.
__device__ __forceinline__ u32 ne_flags(const TextDword& d, u32 c4) { return (((d.lo7 ^ c4) + 0x7f7f7f7fu) & 0x80808080u) | d.top; }
// 0x80 where the byte is NO '!' candidate.  A candidate is a byte b with (b & 0x5e) == 0: in a quality line (0x21 .. 0x7e) that
// is '!' alone.  (No carry between bytes: 0x5e + 0x7f < 0x100.)
__device__ __forceinline__ u32 nbang_flags(const TextDword& d) { return ((d.w & 0x5e5e5e5eu) + 0x7f7f7f7fu) & 0x80808080u; }
// 0x40 where the byte is an odd-base candidate: bit 3 (N, '.') or bits 5 and 6 (lowercase) -- every N-like or lowercase base, and
// no A C G T 0 1 2 3.  (Bit 6 of w & (w << 1) is the byte's own bits 6 and 5; bit 6 of w << 3 its own bit 3.)
__device__ __forceinline__ u32 odd_flags(const TextDword& d) { return ((d.w << 3) | (d.w & (d.w << 1))) & 0x40404040u; }

// The masks of one 16-byte piece.  nl, at, pl, bang are COMPLEMENTS: a 0 bit is a newline, an '@', a '+', a '!' candidate.
struct PieceMasks { u32 nnl, nat, npl, nbang, odd; };
template <bool MARKS>
__device__ __forceinline__ PieceMasks piece_masks(u32 x, u32 y, u32 z, u32 w) {
    const TextDword a(x), b(y), c(z), d(w);
    PieceMasks m;
    m.nnl = gather16<7>(ne_flags(a, 0x0a0a0a0au), ne_flags(b, 0x0a0a0a0au), ne_flags(c, 0x0a0a0a0au), ne_flags(d, 0x0a0a0a0au));
    m.nat = gather16<7>(ne_flags(a, 0x40404040u), ne_flags(b, 0x40404040u), ne_flags(c, 0x40404040u), ne_flags(d, 0x40404040u));
    m.npl = gather16<7>(ne_flags(a, 0x2b2b2b2bu), ne_flags(b, 0x2b2b2b2bu), ne_flags(c, 0x2b2b2b2bu), ne_flags(d, 0x2b2b2b2bu));
    m.nbang = 0; m.odd = 0;
    if (MARKS) {
        m.nbang = gather16<7>(nbang_flags(a), nbang_flags(b), nbang_flags(c), nbang_flags(d));
        m.odd = gather16<6>(odd_flags(a), odd_flags(b), odd_flags(c), odd_flags(d));
    }
    return m;
}

// ---- the '@' and '+' masks as ONE ------------------------------------------------------------------------------------------
// Only a byte behind a line end is ever asked whether it is '@' or '+', so the two masks fold into one without loss: a line
// end's own bit says whether the byte BEHIND it is a '+' (a line end is neither prefix: its own bit is free), every other bit
// whether its own byte is an '@'.  Complemented like the masks it is made of:
//     nfold bit p = byte p is a line end ? (byte p + 1 is no '+') : (byte p is no '@')
// npl_next: the '+' mask of the sixteen bytes behind this piece (bit 0 alone is used).  What the fold confuses is a line start
// that is itself a line end -- an empty line: its bit answers for the byte behind it.  The readers below do not ask it:
//   * "is the line start at p no '@'?" looks at the line-end mask first (prefix_no_at: an empty line has no '@');
//   * "is the line start behind the line end at i no '+'?" reads bit i, which a line end always owns (prefix_no_plus): an empty
//     '+' line is a byte '\n' that is no '+', as before.
// So every text gets the verdict the two plain masks gave (scratch/host_frame_masks_test.cpp runs both over hostile windows).
__device__ __forceinline__ u32 fold_prefix16(u32 nnl, u32 nat, u32 npl, u32 npl_next) {
    const u32 npl_behind = (npl | (npl_next << 16)) >> 1;  // bit p: byte p + 1 is no '+'
    return nat & (nnl | npl_behind);                       // (nat has sixteen bits: so has the result)
}
// nl: the window's line ends (not complemented), nfold: its folded mask
__device__ __forceinline__ u32 prefix_no_at(u64 nl, u64 nfold, u32 p) { return (u32)(((nl | nfold) >> p) & 1ull); }
__device__ __forceinline__ u32 prefix_no_plus(u64 nfold, u32 i) { return (u32)((nfold >> i) & 1ull); }       // i: the line end before the line start

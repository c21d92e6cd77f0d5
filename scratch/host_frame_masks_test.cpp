// g++ -O2 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iscratch/hoststub -Islimfastq_amd/csrc scratch/host_frame_masks_test.cpp && ./a.out
// k_frame's byte tests and mask gather (frame_masks.h) against a byte-by-byte loop, on the CPU: a portable statement of the
// dot product stands in for v_dot4_u32_u8.
//   1. every per-dword test (differs from '\n', '@', '+'; no '!' candidate; odd-base candidate) over ALL 2^32 dwords: the flag
//      of each byte as the loop says, every other bit of the dword 0 (what gather16 needs);
//   2. gather16 over every one of the 2^16 flag patterns of a piece, for both flag bits in use, and that stray carries cannot
//      happen: the sums stay within their sixteen bits;
//   3. piece_masks on pieces of random and hostile bytes (line ends, prefixes, their neighbours in value, 0x00, 0x8a, 0xab, 0xc0,
//      0xff) against five byte loops, with and without the marks;
//   4. the fold of the '@' and '+' masks into one (fold_prefix16, prefix_no_at, prefix_no_plus) against the two plain masks: windows
//      of 64 bytes and the 16 behind them, random and hostile -- a third to a half of the bytes line ends, so that empty lines,
//      line ends at a piece's and the window's last byte, and both prefixes behind each other are common --, every line start
//      asked both questions.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include "frame_masks.h"

static bool bang_cand(u32 b) { return (b & 0x5eu) == 0; }
static bool odd_cand(u32 b) { return (b & 0x08u) || ((b & 0x60u) == 0x60u); }

static int fail(const char* what, u64 at, u32 got, u32 want) {
    printf("FAIL %s at %llx: got %08x want %08x\n", what, (unsigned long long)at, got, want);
    return 1;
}

int main() {
    // 1. per byte value, what each test must flag; a dword's expected flags are its bytes' side by side
    static u32 t_nl[256], t_at[256], t_pl[256], t_bang[256], t_odd[256];
    for (u32 b = 0; b < 256; b++) {
        t_nl[b] = b != '\n' ? 0x80u : 0u; t_at[b] = b != '@' ? 0x80u : 0u; t_pl[b] = b != '+' ? 0x80u : 0u;
        t_bang[b] = bang_cand(b) ? 0u : 0x80u; t_odd[b] = odd_cand(b) ? 0x40u : 0u;
    }
    for (u64 v = 0; v < (1ull << 32); v++) {
        const u32 x = (u32)v, b0 = x & 0xff, b1 = (x >> 8) & 0xff, b2 = (x >> 16) & 0xff, b3 = x >> 24;
        const TextDword d(x);
#define WANT(t) (t[b0] | t[b1] << 8 | t[b2] << 16 | t[b3] << 24)
        if (ne_flags(d, 0x0a0a0a0au) != WANT(t_nl)) return fail("ne_flags newline", v, ne_flags(d, 0x0a0a0a0au), WANT(t_nl));
        if (ne_flags(d, 0x40404040u) != WANT(t_at)) return fail("ne_flags @", v, ne_flags(d, 0x40404040u), WANT(t_at));
        if (ne_flags(d, 0x2b2b2b2bu) != WANT(t_pl)) return fail("ne_flags +", v, ne_flags(d, 0x2b2b2b2bu), WANT(t_pl));
        if (nbang_flags(d) != WANT(t_bang)) return fail("nbang_flags", v, nbang_flags(d), WANT(t_bang));
        if (odd_flags(d) != WANT(t_odd)) return fail("odd_flags", v, odd_flags(d), WANT(t_odd));
#undef WANT
    }
    printf("per-dword tests: all 2^32 dwords agree with the byte loop\n");

    // 2. the gather: bit 4 d + i of the mask = the flag of byte i of dword d
    for (u32 bit = 6; bit <= 7; bit++)
        for (u32 m = 0; m < 65536; m++) {
            u32 f[4] = {0, 0, 0, 0};
            for (u32 k = 0; k < 16; k++) if ((m >> k) & 1u) f[k >> 2] |= (1u << bit) << (8 * (k & 3));
            const u32 got = bit == 7 ? gather16<7>(f[0], f[1], f[2], f[3]) : gather16<6>(f[0], f[1], f[2], f[3]);
            if (got != m) return fail("gather16", m, got, m);
        }
    printf("gather16: all 2^16 patterns, flag bits 6 and 7\n");

    // 3. whole pieces
    static const u8 hostile[] = {'\n', '@', '+', '!', 'N', 'n', '.', 'a', 'A', 0x00, 0x0b, 0x09, 0x8a, 0xab, 0xc0, 0xff, 0x2a, 0x2c, 0x3f, 0x41, 0x80, 0x20, 0x7e, 0x7f};
    srand(7);
    for (u32 trial = 0; trial < 4000000; trial++) {
        u8 p[16];
        const int mode = rand() % 3;                       // 0: any bytes, 1: hostile bytes alone, 2: a mix
        for (int i = 0; i < 16; i++) p[i] = (mode == 0 || (mode == 2 && rand() % 2)) ? (u8)(rand() & 0xff) : hostile[rand() % sizeof(hostile)];
        u32 w[4];
        memcpy(w, p, 16);                                  // (little endian, as the device)
        u32 nl = 0, at = 0, pl = 0, bang = 0, odd = 0;
        for (int i = 0; i < 16; i++) {
            nl |= (u32)(p[i] == '\n') << i; at |= (u32)(p[i] == '@') << i; pl |= (u32)(p[i] == '+') << i;
            bang |= (u32)bang_cand(p[i]) << i; odd |= (u32)odd_cand(p[i]) << i;
        }
        const PieceMasks a = piece_masks<true>(w[0], w[1], w[2], w[3]), b = piece_masks<false>(w[0], w[1], w[2], w[3]);
        if (a.nnl != (~nl & 0xffffu) || b.nnl != a.nnl) return fail("piece newline", trial, a.nnl, ~nl & 0xffffu);
        if (a.nat != (~at & 0xffffu) || b.nat != a.nat) return fail("piece @", trial, a.nat, ~at & 0xffffu);
        if (a.npl != (~pl & 0xffffu) || b.npl != a.npl) return fail("piece +", trial, a.npl, ~pl & 0xffffu);
        if (a.nbang != (~bang & 0xffffu)) return fail("piece !", trial, a.nbang, ~bang & 0xffffu);
        if (a.odd != odd) return fail("piece odd", trial, a.odd, odd);
    }
    printf("piece_masks: 4000000 pieces agree with the byte loops\n");

    // 4. the fold
    static const u8 few[] = {'\n', '\n', '\n', '@', '+', '@', '+', 'A', 0x0b, 0xab, 0xc0, '!'};
    long asked = 0, empty_lines = 0;
    for (u32 trial = 0; trial < 1000000; trial++) {
        u8 t[80];
        const int mode = rand() % 3;
        for (int i = 0; i < 80; i++) t[i] = mode == 0 ? (u8)(rand() & 0xff) : mode == 1 ? few[rand() % sizeof(few)] : hostile[rand() % 6];
        u64 nl = 0, nfold = 0;
        for (int q = 0; q < 4; q++) {
            u32 w[4], w2[4];
            memcpy(w, t + 16 * q, 16); memcpy(w2, t + 16 * q + 16, 16);
            const PieceMasks m = piece_masks<false>(w[0], w[1], w[2], w[3]), m2 = piece_masks<false>(w2[0], w2[1], w2[2], w2[3]);
            const u32 f = fold_prefix16(m.nnl, m.nat, m.npl, m2.npl);
            if (f >> 16) return fail("fold: more than sixteen bits", trial, f, f & 0xffffu);
            nl |= (u64)(~m.nnl & 0xffffu) << (16 * q); nfold |= (u64)f << (16 * q);
        }
        if (prefix_no_at(nl, nfold, 0) != (u32)(t[0] != '@')) return fail("fold: '@' at the window's first byte", trial, prefix_no_at(nl, nfold, 0), t[0] != '@');
        for (u32 i = 0; i < 64; i++) {
            if (t[i] != '\n') continue;
            asked++; empty_lines += t[i + 1] == '\n';
            if (prefix_no_plus(nfold, i) != (u32)(t[i + 1] != '+')) return fail("fold: '+' behind a line end", trial * 64ull + i, prefix_no_plus(nfold, i), t[i + 1] != '+');
            if (i < 63 && prefix_no_at(nl, nfold, i + 1) != (u32)(t[i + 1] != '@')) return fail("fold: '@' behind a line end", trial * 64ull + i, prefix_no_at(nl, nfold, i + 1), t[i + 1] != '@');
        }
    }
    printf("fold: %ld line starts asked both questions, %ld of them empty lines\nok\n", asked, empty_lines);
    return 0;
}

// bgz_code.h -- the serial steps of bgz.hip's deflater, written once for the device and the host: the symbols of a token, the
// Huffman code lengths of a histogram under a length limit, the canonical codes, the code-length header of a dynamic block
// (RFC 1951 3.2.7) and the bit writer the header goes through.  On the device one lane runs them over arrays in LDS -- nothing here
// indexes an array of its own, so nothing goes to scratch; tests/bgzf_model.cpp runs the same functions on the CPU.
#pragma once
#include <stdint.h>
typedef uint8_t  u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;
typedef int32_t  i32;

#if defined(__HIPCC__)
#define BGZ_HD __host__ __device__ __forceinline__
#else
#define BGZ_HD inline
#endif

namespace bgz {

constexpr u32 PIECE = 65280;              // SFQ_BGZF_PIECE: text bytes of a member at most
constexpr u32 SLOT = 65536;               // a member's slot in the scratch buffer
constexpr u32 SLOT_LEAD = 2;              // the member begins here in its slot: its deflate stream, 18 bytes on, is dword aligned
constexpr u32 MIN_MATCH = 4, MAX_MATCH = 258, MAX_DIST = 32768;
constexpr u32 HASH_BITS = 12;             // 4096 u16 entries: the last position of a 4-byte string, 8 KiB of LDS
constexpr u32 CHUNK = 64;                 // positions the parse takes at a time: a lane each
constexpr u32 N_LL = 286, N_D = 30, N_CL = 19, EOB = 256;
constexpr u32 TOK_MATCH = 1u << 31;       // a token: a literal's byte, or TOK_MATCH | (distance - 1) << 8 | (length - 3)

BGZ_HD u32 hash4(u32 w) { return (w * 2654435761u) >> (32 - HASH_BITS); }
BGZ_HD u32 log2u(u32 v) { u32 r = 0; while (v >>= 1) r++; return r; }          // v > 0

// length - 3 (0 .. 255) -> literal/length symbol, extra bits and their value
BGZ_HD void len_sym(u32 l, u32* sym, u32* nx, u32* xv) {
    if (l < 8) { *sym = 257 + l; *nx = 0; *xv = 0; return; }
    if (l == 255) { *sym = 285; *nx = 0; *xv = 0; return; }
    const u32 e = log2u(l) - 2;
    *sym = 261 + 4 * e + ((l >> e) & 3u); *nx = e; *xv = l & ((1u << e) - 1u);
}
// distance - 1 (0 .. 32767) -> distance symbol, extra bits and their value
BGZ_HD void dist_sym(u32 d, u32* sym, u32* nx, u32* xv) {
    if (d < 4) { *sym = d; *nx = 0; *xv = 0; return; }
    const u32 nb = log2u(d);
    *sym = 2 * nb + ((d >> (nb - 1)) & 1u); *nx = nb - 1; *xv = d & ((1u << (nb - 1)) - 1u);
}
BGZ_HD u32 rev_bits(u32 v, u32 len) {     // the low len (1 .. 16) bits of v, first bit last
    v = ((v >> 1) & 0x5555u) | ((v & 0x5555u) << 1);
    v = ((v >> 2) & 0x3333u) | ((v & 0x3333u) << 2);
    v = ((v >> 4) & 0x0F0Fu) | ((v & 0x0F0Fu) << 4);
    v = ((v >> 8) & 0x00FFu) | ((v & 0x00FFu) << 8);
    return v >> (16 - len);
}

// What the code construction works in (LDS on the device).  key[n]: the used symbols as freq << 9 | sym; iw, pl, pi, dep: n entries
// each; blc, nxt: 16 entries each.
struct HuffWork { u32* key; u32* iw; u16* pl; u16* pi; u16* dep; u32* blc; u32* nxt; };

// The used symbols of freq[0, nsym) into W.key, ascending (by count, then by symbol: every key is different, so the order -- and with
// it every code length -- is a function of the histogram alone).  A rank sort; the device ranks with all lanes (bgz.hip).
BGZ_HD u32 huff_sort_serial(const u32* freq, u32 nsym, const HuffWork& W) {
    u32 n = 0;
    for (u32 s = 0; s < nsym; s++) {
        if (!freq[s]) continue;
        const u32 k = (freq[s] << 9) | s;
        u32 i = n++;
        while (i && W.key[i - 1] > k) { W.key[i] = W.key[i - 1]; i--; }
        W.key[i] = k;
    }
    return n;
}

// Code lengths of the n >= 1 sorted symbols of W.key, none above maxbits, into len[] (zeroed by the caller).  The tree is Huffman's,
// built with two queues (the sorted leaves; the inner nodes, which come out in ascending order), a leaf before an inner node of the
// same weight.  Only the COUNT of leaves at every depth is kept; depths above maxbits are folded back as zlib's gen_bitlen does it (a
// leaf one level above the deepest legal one moves down and takes a too-deep leaf as its brother, until none is left), which keeps the
// Kraft sum at one; then the longest lengths go to the rarest symbols in sorted order.  One symbol alone gets one bit.
// Returns the depth of Huffman's own tree, before the limit (the tests ask it whether the limit acted).
BGZ_HD u32 huff_lengths(const HuffWork& W, u32 n, u32 maxbits, u8* len) {
    if (n == 1) { len[W.key[0] & 511u] = 1; return 1; }
    u32 li = 0, ii = 0, ni = 0;
    for (u32 k = 0; k + 1 < n; k++) {
        u32 w = 0;
        for (u32 t = 0; t < 2; t++) {
            if (li < n && (ii >= ni || (W.key[li] >> 9) <= W.iw[ii])) { w += W.key[li] >> 9; W.pl[li++] = (u16)ni; }
            else { w += W.iw[ii]; W.pi[ii++] = (u16)ni; }
        }
        W.iw[ni++] = w;
    }
    for (u32 b = 0; b < 16; b++) W.blc[b] = 0;
    W.dep[ni - 1] = 0;
    for (u32 i = ni - 1; i-- > 0;) W.dep[i] = (u16)(W.dep[W.pi[i]] + 1);
    u32 deepest = 0;
    for (u32 k = 0; k < n; k++) {
        const u32 d = W.dep[W.pl[k]] + 1u;
        if (d > deepest) deepest = d;
        W.blc[d > maxbits ? maxbits : d]++;
    }
    u32 kraft = 0;                                             // in units of 2^-maxbits; the clamped leaves make it too large
    for (u32 b = 1; b <= maxbits; b++) kraft += W.blc[b] << (maxbits - b);
    for (u32 over = kraft - (1u << maxbits); over; over--) {   // a step takes exactly one unit off
        u32 b = maxbits - 1;
        while (!W.blc[b]) b--;
        W.blc[b]--; W.blc[b + 1] += 2; W.blc[maxbits]--;
    }
    u32 i = 0;
    for (u32 b = maxbits; b; b--)
        for (u32 c = W.blc[b]; c; c--) len[W.key[i++] & 511u] = (u8)b;
    return deepest;
}

// canonical codes (RFC 1951 3.2.2) of len[0, nsym), bit-reversed as the stream wants them: code[s] = bits | len << 16
BGZ_HD void huff_codes(const u8* len, u32 nsym, u32 maxbits, const HuffWork& W, u32* code) {
    for (u32 b = 0; b < 16; b++) W.blc[b] = 0;
    for (u32 s = 0; s < nsym; s++) W.blc[len[s]]++;
    u32 c = 0;
    W.blc[0] = 0; W.nxt[0] = 0;
    for (u32 b = 1; b <= maxbits; b++) { c = (c + W.blc[b - 1]) << 1; W.nxt[b] = c; }
    for (u32 s = 0; s < nsym; s++) {
        const u32 l = len[s];
        code[s] = l ? rev_bits(W.nxt[l]++, l) | (l << 16) : 0u;
    }
}

// bits into zeroed words, first bit lowest
struct BitW {
    u32* w; u64 acc; u32 nb, pos;
    BGZ_HD void put(u32 v, u32 n) {
        acc |= (u64)v << nb; nb += n;
        if (nb >= 32) { w[pos++] = (u32)acc; acc >>= 32; nb -= 32; }
    }
    BGZ_HD void flush() { if (nb) w[pos] = (u32)acc; }
    BGZ_HD u32 bits() const { return 32 * pos + nb; }
};

// the order in which the code-length code's lengths are sent
BGZ_HD u32 cl_order(u32 i) {
    // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    if (i < 3) return 16 + i;
    if (i == 3) return 0;
    const u32 k = (i - 4) >> 1;                              // 8 7 | 9 6 | 10 5 | ...
    return (i & 1u) ? 7 - k : 8 + k;
}

// The lengths ll[0, hlit) then dl[0, hdist) as code-length symbols, runs folded (16: the length before 3 .. 6 times; 17, 18: 3 .. 10,
// 11 .. 138 zeros): seq[k] = symbol | extra value << 8, their counts into clf[19] (zeroed by the caller).  Returns the entries.
BGZ_HD u32 cl_sequence(const u8* ll, u32 hlit, const u8* dl, u32 hdist, u16* seq, u32* clf) {
    const u32 total = hlit + hdist;
    u32 i = 0, k = 0;
    while (i < total) {
        const u32 v = i < hlit ? ll[i] : dl[i - hlit];
        u32 run = 1;
        while (i + run < total && (i + run < hlit ? ll[i + run] : dl[i + run - hlit]) == v) run++;
        i += run;
        if (!v) {
            while (run >= 11) { const u32 r = run < 138 ? run : 138; seq[k++] = (u16)(18 | (r - 11) << 8); clf[18]++; run -= r; }
            if (run >= 3) { seq[k++] = (u16)(17 | (run - 3) << 8); clf[17]++; run = 0; }
        } else {
            seq[k++] = (u16)v; clf[v]++; run--;
            while (run >= 3) { const u32 r = run < 6 ? run : 6; seq[k++] = (u16)(16 | (r - 3) << 8); clf[16]++; run -= r; }
        }
        for (; run; run--) { seq[k++] = (u16)v; clf[v]++; }
    }
    return k;
}
BGZ_HD u32 cl_extra_bits(u32 sym) { return sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u; }

// the last used code-length symbol in sending order, as HCLEN counts it (4 at least)
BGZ_HD u32 cl_count(const u8* cll) {
    u32 h = 19;
    while (h > 4 && !cll[cl_order(h - 1)]) h--;
    return h;
}
// bits of a dynamic block's header: BFINAL, BTYPE, HLIT, HDIST, HCLEN, the code-length code, the sequence
BGZ_HD u32 header_bits(const u16* seq, u32 nseq, const u8* cll, u32 hclen) {
    u32 b = 3 + 5 + 5 + 4 + 3 * hclen;
    for (u32 k = 0; k < nseq; k++) { const u32 s = seq[k] & 255u; b += cll[s] + cl_extra_bits(s); }
    return b;
}
BGZ_HD void header_write(BitW& bw, u32 hlit, u32 hdist, const u16* seq, u32 nseq, const u8* cll, const u32* clc, u32 hclen) {
    bw.put(1, 1); bw.put(2, 2);
    bw.put(hlit - 257, 5); bw.put(hdist - 1, 5); bw.put(hclen - 4, 4);
    for (u32 i = 0; i < hclen; i++) bw.put(cll[cl_order(i)], 3);
    for (u32 k = 0; k < nseq; k++) {
        const u32 s = seq[k] & 255u, c = clc[s];
        bw.put(c & 0xFFFFu, c >> 16);
        if (s >= 16) bw.put(seq[k] >> 8, cl_extra_bits(s));
    }
}

// a token's bits under the two codes (at most 15 + 5 + 15 + 13 = 48)
BGZ_HD void token_bits(u32 t, const u32* llc, const u32* dc, u64* bits, u32* nbits) {
    if (!(t & TOK_MATCH)) { const u32 c = llc[t & 255u]; *bits = c & 0xFFFFu; *nbits = c >> 16; return; }
    u32 s, nx, xv;
    len_sym(t & 255u, &s, &nx, &xv);
    u32 c = llc[s];
    u64 v = c & 0xFFFFu; u32 n = c >> 16;
    v |= (u64)xv << n; n += nx;
    dist_sym((t >> 8) & 0x7FFFu, &s, &nx, &xv);
    c = dc[s];
    v |= (u64)(c & 0xFFFFu) << n; n += c >> 16;
    v |= (u64)xv << n; n += nx;
    *bits = v; *nbits = n;
}

}  // namespace bgz

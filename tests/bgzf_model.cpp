// bgzf_model.cpp -- bgz.hip's deflater on the CPU: the parse restated serially (the same chunks, table and tie rules), everything
// behind it -- code lengths, their limit, the canonical codes, the code-length header, the tokens' bits -- through the very functions
// the kernel calls (slimfastq_amd/csrc/bgz_code.h).  tests/test_bgzf_host.py compiles it, runs it over texts and inflates what it
// writes with zlib; the GPU tests compare the kernel's members with its members byte for byte.
//     bgzf_model IN OUT [maxbits]      IN as ONE part: BGZF members to OUT (no end-of-file block); maxbits: the literal/length and
//                                      distance codes' limit (15; a test lowers it to make the limit act on small texts).  Per
//                                      member a line on stdout: the depths of Huffman's own trees before the limits (literal/length,
//                                      distance, code lengths) and the tokens
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../slimfastq_amd/csrc/bgz_code.h"

using namespace bgz;

static u32 crc_tab[256];
static u32 crc32(const u8* p, size_t n) {
    if (!crc_tab[1]) for (u32 b = 0; b < 256; b++) { u32 c = b; for (int i = 0; i < 8; i++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); crc_tab[b] = c; }
    u32 c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = (c >> 8) ^ crc_tab[(c ^ p[i]) & 255u];
    return ~c;
}
static u32 ld32(const u8* t, u32 pos) { u32 w; memcpy(&w, t + pos, 4); return w; }

static void member(const u8* a, u32 n, u32 maxbits, std::vector<u8>& out) {
    std::vector<u8> text(n + 8, 0);
    memcpy(text.data(), a, n);
    std::vector<u16> hash(1u << HASH_BITS, 0xFFFF);
    std::vector<u32> tok;
    u32 f_ll[288] = {0}, f_d[32] = {0};
    u32 covered = 0;
    for (u32 p0 = 0; p0 < n; p0 += CHUNK) {
        u32 len[CHUNK], dist[CHUNK], h[CHUNK]; bool can[CHUNK];
        for (u32 lane = 0; lane < CHUNK; lane++) {
            const u32 p = p0 + lane;
            can[lane] = p + MIN_MATCH <= n;
            h[lane] = can[lane] ? hash4(ld32(text.data(), p)) : 0;
            len[lane] = dist[lane] = 0;
            if (covered < p0 + CHUNK && can[lane] && p >= covered) {
                const u32 c = hash[h[lane]];
                if (c != 0xFFFF && p - c <= MAX_DIST) {
                    const u32 maxlen = n - p < MAX_MATCH ? n - p : MAX_MATCH;
                    u32 l = 0;
                    while (l < maxlen && text[c + l] == text[p + l]) l++;
                    len[lane] = l < MIN_MATCH ? 0 : l; dist[lane] = p - c;
                }
            }
        }
        u32 pos = covered > p0 ? covered : p0;
        const u32 lim = p0 + CHUNK < n ? p0 + CHUNK : n;
        while (pos < lim) {
            const u32 lane = pos - p0;
            u32 s, nx, xv;
            if (len[lane]) {
                tok.push_back(TOK_MATCH | ((dist[lane] - 1) << 8) | (len[lane] - 3));
                len_sym(len[lane] - 3, &s, &nx, &xv); f_ll[s]++;
                dist_sym(dist[lane] - 1, &s, &nx, &xv); f_d[s]++;
                pos += len[lane];
            } else { tok.push_back(text[pos]); f_ll[text[pos]]++; pos++; }
        }
        if (pos > covered) covered = pos;
        if (covered < p0 + CHUNK) covered = p0 + CHUNK;
        for (u32 lane = 0; lane < CHUNK; lane++) if (can[lane]) hash[h[lane]] = (u16)(p0 + lane);
    }
    f_ll[EOB] = 1;
    u32 key[288], iw[288], blc[16], nxt[16], c_ll[288], c_d[32], f_cl[20] = {0}, c_cl[20];
    u16 pl[288], pi[288], dep[288], seq[320];
    u8 l_ll[288] = {0}, l_d[32] = {0}, l_cl[20] = {0};
    const HuffWork HW{ key, iw, pl, pi, dep, blc, nxt };
    u32 depth[3] = {0, 0, 0};                                  // Huffman's own trees, before the limits: literal/length, distance, code lengths
    depth[0] = huff_lengths(HW, huff_sort_serial(f_ll, N_LL, HW), maxbits, l_ll);
    huff_codes(l_ll, N_LL, 15, HW, c_ll);
    const u32 n_d = huff_sort_serial(f_d, N_D, HW);
    if (n_d) depth[1] = huff_lengths(HW, n_d, maxbits, l_d);
    huff_codes(l_d, N_D, 15, HW, c_d);
    u32 hlit = N_LL, hdist = N_D;
    while (hlit > 257 && !l_ll[hlit - 1]) hlit--;
    while (hdist > 1 && !l_d[hdist - 1]) hdist--;
    const u32 nseq = cl_sequence(l_ll, hlit, l_d, hdist, seq, f_cl);
    const u32 ncl = huff_sort_serial(f_cl, N_CL, HW);
    if (ncl == 1) { const u32 s = key[0] & 511u; l_cl[s] = 1; l_cl[s ? 0 : 1] = 1; }
    else depth[2] = huff_lengths(HW, ncl, 7, l_cl);
    printf("%u %u %u %zu\n", depth[0], depth[1], depth[2], tok.size());
    huff_codes(l_cl, N_CL, 7, HW, c_cl);
    const u32 hclen = cl_count(l_cl);
    const u32 hbits = header_bits(seq, nseq, l_cl, hclen);
    u64 bits = hbits;
    for (u32 t : tok) { u64 v; u32 nb; token_bits(t, c_ll, c_d, &v, &nb); bits += nb; }
    bits += c_ll[EOB] >> 16;
    const u32 bytes = (u32)((bits + 7) >> 3);
    const bool stored = bytes > n + 5;
    const u32 dbytes = stored ? n + 5 : bytes;
    std::vector<u8> d(dbytes + 16, 0);
    if (stored) {
        d[0] = 1; d[1] = (u8)n; d[2] = (u8)(n >> 8); d[3] = (u8)~n; d[4] = (u8)(~n >> 8);
        memcpy(d.data() + 5, a, n);
    } else {
        std::vector<u32> w(dbytes / 4 + 4, 0);
        BitW bw{ w.data(), 0, 0, 0 };
        header_write(bw, hlit, hdist, seq, nseq, l_cl, c_cl, hclen);
        tok.push_back(~0u);
        for (u32 t : tok) {
            u64 v; u32 nb;
            if (t == ~0u) { v = c_ll[EOB] & 0xFFFFu; nb = c_ll[EOB] >> 16; } else token_bits(t, c_ll, c_d, &v, &nb);
            bw.put((u32)v & 0xFFFFu, nb < 16 ? nb : 16);
            if (nb > 16) { bw.put((u32)(v >> 16) & 0xFFFFu, nb - 16 < 16 ? nb - 16 : 16); }
            if (nb > 32) bw.put((u32)(v >> 32) & 0xFFFFu, nb - 32);
        }
        bw.flush();
        memcpy(d.data(), w.data(), dbytes);
    }
    const u32 total = 18 + dbytes + 8, bs = total - 1, crc = crc32(a, n);
    const u8 hdr[18] = { 0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (u8)bs, (u8)(bs >> 8) };
    out.insert(out.end(), hdr, hdr + 18);
    out.insert(out.end(), d.begin(), d.begin() + dbytes);
    for (int i = 0; i < 4; i++) out.push_back((u8)(crc >> (8 * i)));
    for (int i = 0; i < 4; i++) out.push_back((u8)(n >> (8 * i)));
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: bgzf_model IN OUT [maxbits]\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    std::vector<u8> in;
    u8 buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + k);
    fclose(f);
    const u32 maxbits = argc > 3 ? (u32)atoi(argv[3]) : 15;
    std::vector<u8> out;
    for (size_t at = 0; at < in.size(); at += PIECE) member(in.data() + at, (u32)(in.size() - at < PIECE ? in.size() - at : PIECE), maxbits, out);
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    return 0;
}

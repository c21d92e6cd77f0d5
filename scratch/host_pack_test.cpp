// g++ -O2 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Iscratch/hoststub -Islimfastq_amd/csrc scratch/host_pack_test.cpp && ./a.out
// k_gen_pack_raw's arithmetic (gen_pack_place.h) on the CPU: a chain of lines is packed the way the kernel does it -- chunks of 64
// records, a group of lanes per record whose width the chunk's longest line sets, a lane per sixteen bases, the validity mask, the place of a piece's thirty-two bits, the ring
// of GP_RING dwords and its rows -- and compared with a pack written byte by byte.  The text lies in a buffer of exactly its
// size and the ring in one of exactly GP_RING dwords: a step outside either is the sanitizer's.  Checked on the way: a deposit
// never lands outside the ring's window [row, row + GP_RING), a dword is stored once, and a row only when nothing is deposited
// into it afterwards.
//   1. the validity mask for every length 0 .. 40 against a byte loop;
//   2. gp_place for every position mod 16 and hostile codes against a 64-bit shift;
//   3. chains: every group width 1 .. 64 (gp_div_lanes against the integer division on the way); random lengths of each width class; runs of 1-, 2-, 3-base lines between normal ones; every residue mod 16; the
//      widths' edges 64 / 128 / 256 / 1024 +- 1; empty lines; chains of 1, 7, 64, 65, 130, 200 records; chains that go round
//      the ring many times (200 x 257, 200 x 150, lines of 6000).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "gen_pack_place.h"

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u32 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (u32)(rng_state >> 32); }

static int fail(const char* what, u64 at, u64 got, u64 want) {
    printf("FAIL %s at %llu: got %llx want %llx\n", what, (unsigned long long)at, (unsigned long long)got, (unsigned long long)want);
    return 1;
}

// the kernel's loop over one chain: lines[i] = {offset in text, bases}; returns the dwords stored
static int pack_chain(const std::vector<u8>& text, const std::vector<std::pair<u64, u32>>& lines, std::vector<u32>& out, u32& bases) {
    std::vector<u32> ring(GP_RING, 0u);
    const u32 nrec = (u32)lines.size();
    u32 done = 0, row = 0;
    for (u32 k0 = 0; k0 < nrec; k0 += 64u) {
        const u32 n = nrec - k0 < 64u ? nrec - k0 : 64u;
        u64 b0[64]; u32 len[64], inc[64], first[64];
        u32 sum = 0, mx = 0;
        for (u32 l = 0; l < 64; l++) {
            b0[l] = l < n ? lines[k0 + l].first : 0; len[l] = l < n ? lines[k0 + l].second : 0u;
            first[l] = done + sum; sum += len[l]; inc[l] = sum; if (len[l] > mx) mx = len[l];
        }
        const u32 lanes = gp_group_lanes(mx), per = gp_div_lanes(64u, lanes);
        if (per != 64u / lanes || 16u * lanes < (mx < 1024u ? mx : 1024u)) return fail("group", mx, lanes, per);
        for (u32 s0 = 0; s0 < n; s0 += per) {
            const u32 last = gp_step_last(s0, n, per);
            const u32 rec_end = done + inc[last], last_len = len[last];
            u32 q0 = 0;
            do {
                for (u32 lane = 0; lane < 64; lane++) {
                    const u32 sub = gp_div_lanes(lane, lanes);
                    if (sub != lane / lanes) return fail("gp_div_lanes", lane, sub, lane / lanes);
                    const u32 rec = s0 + sub;
                    const u32 off = q0 + gp_lane_piece(lane, sub, lanes, per);
                    if (rec >= n || off >= len[rec]) continue;
                    const uint4 vm = gp_valid4(len[rec] - off);
                    const u32 m[4] = {vm.x, vm.y, vm.z, vm.w};
                    u32 code = 0;
                    for (u32 j = 0; j < 16; j++) {
                        if (!((m[j >> 2] >> (8u * (j & 3u))) & 0xffu)) continue;
                        code |= (gen_code_of(text.at(b0[rec] + off + j)) & 3u) << (2u * j);        // (at(): a valid byte lies inside the text)
                    }
                    const GpPlace g = gp_place(first[rec] + off, code);
                    if (g.d < row || g.d - row >= GP_RING) return fail("deposit outside the ring's window", g.d, g.d, row);
                    ring[gp_ring_slot(g.d)] |= g.lo;
                    if (g.hi) {
                        if (g.d + 1u - row >= GP_RING) return fail("spill outside the ring's window", g.d + 1u, g.d + 1u, row);
                        ring[gp_ring_slot(g.d + 1u)] |= g.hi;
                    }
                }
                const u32 next = gp_turn_end(rec_end, last_len, q0);
                if (gp_row_ready(row, next)) {
                    for (u32 lane = 0; lane < 64; lane++) { const u32 t = row + lane; out.push_back(ring[gp_ring_slot(t)]); ring[gp_ring_slot(t)] = 0; }
                    row += GP_ROW;
                }
                if (gp_row_ready(row, next)) return fail("two rows complete in one turn", row, next, 0);
                q0 += 1024u;
            } while (q0 < last_len);
        }
        done += inc[63];
    }
    const u32 tail = gp_tail_dwords(row, done);
    if (tail > GP_ROW) return fail("tail longer than a row", row, tail, GP_ROW);
    for (u32 lane = 0; lane < tail; lane++) { out.push_back(ring[gp_ring_slot(row + lane)]); ring[gp_ring_slot(row + lane)] = 0; }
    for (u32 i = 0; i < GP_RING; i++) if (ring[i]) return fail("bits left in the ring", i, ring[i], 0);
    bases = done;
    return 0;
}

// lens -> a text (a FASTQ-like neighbourhood: the line, '\n', '+', so that the bytes behind a line differ from bases), packed both ways
static int run_case(const char* what, const std::vector<u32>& lens) {
    std::vector<u8> text;
    std::vector<std::pair<u64, u32>> lines;
    for (u32 ln : lens) {
        text.push_back('@');
        lines.push_back({(u64)text.size(), ln});
        for (u32 i = 0; i < ln; i++) { const u32 r = rnd(); text.push_back((r & 0xff) < 3 ? "Nn.acgt"[(r >> 8) % 7] : "ACGT"[(r >> 8) & 3]); }
        if (rnd() & 1) { text.push_back('\n'); text.push_back('+'); }
    }
    std::vector<u8> want;
    u32 nb = 0, cur = 0;
    for (auto& l : lines) for (u32 i = 0; i < l.second; i++) {
        cur |= (gen_code_of(text[l.first + i]) & 3u) << (2u * (nb & 3u));
        if ((++nb & 3u) == 0) { want.push_back((u8)cur); cur = 0; }
    }
    if (nb & 3u) want.push_back((u8)cur);
    std::vector<u32> out; u32 bases = 0;
    if (pack_chain(text, lines, out, bases)) { printf("  in case %s\n", what); return 1; }
    if (bases != nb) { printf("  in case %s\n", what); return fail("bases", 0, bases, nb); }
    if (out.size() != (nb + 15u) / 16u) { printf("  in case %s\n", what); return fail("dwords stored", 0, out.size(), (nb + 15u) / 16u); }
    for (size_t i = 0; i < out.size() * 4; i++) {
        const u8 got = (u8)(out[i >> 2] >> (8 * (i & 3))), w = i < want.size() ? want[i] : 0;
        if (got != w) { printf("  in case %s\n", what); return fail("packed byte", i, got, w); }
    }
    return 0;
}

int main() {
    // 1. the validity mask
    for (u32 rem = 0; rem <= 40; rem++) {
        const uint4 v = gp_valid4(rem);
        const u32 m[4] = {v.x, v.y, v.z, v.w};
        for (u32 j = 0; j < 16; j++) {
            const u32 got = (m[j >> 2] >> (8u * (j & 3u))) & 0xffu, want = j < rem ? 0xffu : 0u;
            if (got != want) return fail("gp_valid4", rem * 16 + j, got, want);
        }
    }
    // 2. the place of thirty-two bits
    const u32 codes[] = {0u, 1u, 0x80000000u, 0xffffffffu, 0xaaaaaaaau, 0x55555555u, 0xc0000003u, 0x12345678u};
    for (u32 pos = 0; pos < 4096; pos += (pos < 64 ? 1 : 61)) for (u32 cd : codes) {
        const GpPlace g = gp_place(pos, cd);
        const u64 w = (u64)cd << (2u * (pos & 15u));
        if (g.d != pos / 16 || g.lo != (u32)w || g.hi != (u32)(w >> 32)) return fail("gp_place", pos, ((u64)g.hi << 32) | g.lo, w);
    }
    // 3. chains
    int bad = 0, cases = 0;
    const u32 cls[4][2] = {{1, 64}, {65, 128}, {129, 256}, {257, 1100}};
    const u32 counts[] = {1, 7, 64, 65, 130, 200};
    for (auto& c : cls) for (u32 n : counts) for (u32 rep = 0; rep < 4; rep++) {
        std::vector<u32> lens;
        for (u32 i = 0; i < n; i++) lens.push_back(rep == 0 ? c[0] : rep == 1 ? c[1] : c[0] + rnd() % (c[1] - c[0] + 1));
        if (rep == 3 && n > 2) { lens[0] = c[1]; lens[n - 1] = c[0]; lens[n / 2] = 1; }
        bad |= run_case("one width class", lens); cases++;
    }
    for (u32 p = 1; p <= 66; p++) for (u32 n : {5u, 64u, 131u}) {                                // every group width, full and short lines
        std::vector<u32> lens;
        for (u32 i = 0; i < n; i++) lens.push_back(i % 4 == 1 ? 16u * p : i % 4 == 2 ? 16u * p - 15u : 1 + rnd() % (16u * p));
        bad |= run_case("every group width", lens); cases++;
    }
    for (u32 tiny = 1; tiny <= 3; tiny++) for (u32 normal : {5u, 100u, 150u, 300u}) {           // many records in one dword
        std::vector<u32> lens;
        for (u32 g = 0; g < 4; g++) { lens.push_back(normal + g); for (u32 i = 0; i < 40 + 7 * g; i++) lens.push_back(tiny); }
        lens.push_back(normal);
        bad |= run_case("runs of tiny lines", lens); cases++;
    }
    for (u32 base : {0u, 16u, 48u, 112u, 240u, 1008u}) for (u32 r = 0; r < 16; r++) {             // every residue mod 16, in every class
        std::vector<u32> lens;
        for (u32 i = 0; i < 70; i++) lens.push_back(base + r + (base + r == 0 ? 1 : 0));
        bad |= run_case("residues mod 16", lens); cases++;
    }
    for (u32 edge : {64u, 128u, 256u, 1024u}) for (int d = -1; d <= 1; d++) for (u32 n : {3u, 64u, 67u}) {
        std::vector<u32> lens;
        for (u32 i = 0; i < n; i++) lens.push_back(i % 5 == 2 ? edge + d : 1 + rnd() % (edge + d));
        bad |= run_case("width edges", lens); cases++;
    }
    {   std::vector<u32> lens;                                                                     // empty lines among the others
        for (u32 i = 0; i < 150; i++) lens.push_back(i % 3 == 1 ? 0u : rnd() % 40);
        bad |= run_case("empty lines", lens); cases++;
        bad |= run_case("one empty line", std::vector<u32>{0u}); cases++;
        bad |= run_case("no line", std::vector<u32>{}); cases++;
    }
    bad |= run_case("ring wrap 200 x 257", std::vector<u32>(200, 257u)); cases++;
    bad |= run_case("ring wrap 200 x 150", std::vector<u32>(200, 150u)); cases++;
    bad |= run_case("ring wrap 130 x 1024", std::vector<u32>(130, 1024u)); cases++;
    for (u32 ln : {700u, 1000u, 2500u, 6000u, 5999u, 65535u}) { bad |= run_case("one long line", std::vector<u32>{ln}); cases++; }
    for (u32 rep = 0; rep < 300; rep++) {                                                          // anything
        std::vector<u32> lens;
        const u32 n = 1 + rnd() % 200, top = 1u << (1 + rnd() % 11);
        for (u32 i = 0; i < n; i++) lens.push_back(rnd() % 7 == 0 ? 1 + rnd() % 3 : 1 + rnd() % top);
        bad |= run_case("random", lens); cases++;
    }
    if (bad) return 1;
    printf("host_pack_test: ok (%d chains)\n", cases);
    return 0;
}

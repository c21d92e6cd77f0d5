// g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iscratch/hoststub -Islimfastq_amd/csrc scratch/host_renorm_test.cpp && ./a.out
// LaneEncB::renorm() -- one branch-free round, the later rounds a block of their own with a scalar guard -- against the form it had before
// (a `while` with the guard counter in front of it), one "lane": random symbol streams, and hostile ones -- symbols of probability 2^-16
// (a second round each, a third behind a clamp), escapes' flat rows, low forced to where the interval crosses a carry (coder.hpp:76-77), and low forced to where the
// clamp leaves a range of 0, which only the guard ends (err = 1, the range opened again).  Bytes, sizes, err and the coder's state
// must be the same after every symbol.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "dev_chain.h"

struct OldEncB : LaneEncB<1, 8> {
    void renorm_old() {
        step();
        int guard = 0;
        while (__any(range < RC_TOP)) {
            step();
            if (++guard > RC_GUARD) { err = 1; range = 0xFFFFFFFFu; break; }
        }
    }
    void encode_if_old(u32 vm, u32 cum, u32 freq, u32 tot, u32 recip) {
        const u32 r = rc_div(range, tot, recip);
        low += (u64)(cum & vm) * r;
        range ^= (range ^ (r * freq)) & vm;
        renorm_old();
    }
    void encode16_if_old(u32 vm, u32 cum, u32 freq) {
        const u32 r = range >> 16;
        low += (u64)(cum & vm) * r;
        range ^= (range ^ (r * freq)) & vm;
        renorm_old();
    }
};

int main() {
    srand(11);
    long guarded = 0, rounds2 = 0, rounds3 = 0;
    for (int trial = 0; trial < 6000; trial++) {
        const int nsym = rand() % 2000;
        const int mode = rand() % 4;                  // 0: 2^16 rows, 1: a small flat row, 2: any total, 3: hostile
        std::vector<uint8_t> o1(nsym * 8 + 64, 0xAA), o2(nsym * 8 + 64, 0xBB);
        const u32 cap = (u32)((nsym * 8 + 32) & ~15);
        static u32 ring1[LaneEncB<1, 8>::LDS_DWORDS], ring2[LaneEncB<1, 8>::LDS_DWORDS];
        OldEncB a; a.init(ring1, 0, o1.data(), cap);
        LaneEncB<1, 8> b; b.init(ring2, 0, o2.data(), cap);
        for (int i = 0; i < nsym; i++) {
            const int f = rand() % (mode == 3 ? 23 : 97);
            if (f == 0) {                             // the carry-less corner: bits 24..55 of low all ones
                const u64 forced = ((u64)(rand() & 0xff) << 56) | 0x00FFFFFFFF000000ull | (u64)(rand() & 0xFFFFFF);
                a.low = b.low = forced;
            } else if (f == 1 && mode == 3) {         // ... and its low 24 bits too: the clamp leaves range 0, round after round
                a.low = b.low = ((u64)(rand() & 0xff) << 56) | 0x00FFFFFFFFFFFFFFull;
            } else if (f == 2 && mode == 3) {         // ... and all but its last byte: a range below 2^8, three rounds and more
                a.low = b.low = ((u64)(rand() & 0xff) << 56) | 0x00FFFFFFFFFFFF00ull | (u64)(rand() & 0xff);
            }
            const bool valid = rand() % 8 != 0;
            const u32 vm = valid ? ~0u : 0u;
            u32 cum, freq, tot;
            if (mode == 0) { tot = 65536; freq = 1 + rand() % (rand() % 4 ? 60000 : 3); cum = rand() % (tot - freq + 1); }
            else if (mode == 1) { tot = 12; freq = 3; cum = 3 * (rand() % 4); }
            else if (mode == 2) { tot = 4 + rand() % 1017; freq = 1 + rand() % (tot < 256 ? tot : 255); if (freq > tot) freq = tot; cum = rand() % (tot - freq + 1); }
            else { tot = 65536; if (rand() % 3) { freq = 1; cum = rand() % tot; } else { freq = 256; cum = (rand() & 0xff) << 8; } }
            if (mode == 3 && f <= 2 && rand() % 2) cum = 0;         // (low stays where it was forced to)
            const u32 q0 = b.q;
            if (tot == 65536) { a.encode16_if_old(vm, cum, freq); b.encode16_if(vm, cum, freq); }
            else { const u32 rc = rc_recip(tot); a.encode_if_old(vm, cum, freq, tot, rc); b.encode_if(vm, cum, freq, tot, rc); }
            if (b.q - q0 == 2) rounds2++;
            if (b.q - q0 >= 3) rounds3++;
            if (a.low != b.low || a.range != b.range || a.q != b.q || a.err != b.err) { printf("STATE MISMATCH trial %d symbol %d mode %d\n", trial, i, mode); return 1; }
            if (b.err & 1) { guarded++; a.err = b.err = 0; }
            a.drain(); b.drain();                     // (15 bytes may wait, a symbol the guard ends adds 14: the ring's 32 hold that)
        }
        const u32 s1 = a.finish(), s2 = b.finish();
        if (s1 != s2 || a.err != b.err || memcmp(o1.data(), o2.data(), s1 < cap ? s1 : cap)) { printf("MISMATCH trial %d nsym %d mode %d sizes %u %u err %u %u\n", trial, nsym, mode, s1, s2, a.err, b.err); return 1; }
        for (size_t k = cap; k < o2.size(); k++) if (o2[k] != 0xBB || o1[k] != 0xAA) { printf("write past cap trial %d\n", trial); return 1; }
    }
    if (!guarded || !rounds2 || rounds3 <= guarded) { printf("the streams did not reach the guard (%ld), a second round (%ld) or a third (%ld)\n", guarded, rounds2, rounds3); return 1; }
    printf("ok: %ld symbols of two rounds, %ld of three or more, the guard fired %ld times\n", rounds2, rounds3, guarded);
    return 0;
}

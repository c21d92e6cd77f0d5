// g++ -O2 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -Iscratch/hoststub -Islimfastq_amd/csrc scratch/host_rec_digits_test.cpp -o /tmp/host_rec_digits_test && /tmp/host_rec_digits_test
// The token step's short decimal fields (rec_digits.h: rd_parse9, four digits a step from the staged dwords) against a byte-wise statement of
// nw_tok's short path (chains.hip), on the CPU.  Every column is a heap block of exactly the dwords the header promises -- up to the dword of the
// field's last byte and no further --, so the address sanitizer sees a load that leaves it on either side.
//   1. every length 0 .. 10 at every byte offset 0 .. 11 (every offset within a dword, fields that begin in the column's first, second and
//      third dword); per length every all-digit field up to five digits, 10^6 random ones above; the bytes before and behind the field filled
//      with digits, letters and 0xFF in turn.  (Ten bytes: the caller does not use the result; the loads must still stay in the column.)
//   2. one byte that is no digit at every position of every length, for bytes on both sides of the digits and with the top bit set.
//   3. a number's symbols in closed form (rd_u_count, rd_u_sym0, rd_u_sym1) against put_u_rows' loop (dev_rec_lane.h) around every threshold.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include "rec_digits.h"

struct Ref { u32 value, plain, lead; };
static Ref ref_short(const u8* p, u32 len) {                       // nw_tok's loop, as it was written a byte a step
    Ref r = {0, 1, 0};
    for (u32 j = 0; j < len; j++) {
        const u32 d = (u32)p[j] - '0';
        r.plain = r.plain && d <= 9u;
        r.lead |= (j < 2u && d == 0u) ? 1u << j : 0u;
        r.value = r.value * 10u + d;
    }
    return r;
}
static const u8 fills[3][4] = {{'0', '9', '5', '1'}, {'a', 'Z', 'f', 'x'}, {0xff, 0xff, 0xff, 0xff}};
static long cases = 0;
// the field `text` (len bytes) at byte `off` of a column that ends with the dword of its last byte
static int check(const u8* text, u32 len, u32 off, u32 fill) {
    const u32 nd = len ? (off + len - 1u) / 4u + 1u : 1u;
    u32* col = (u32*)malloc(4u * nd);
    u8* b = (u8*)col;
    for (u32 i = 0; i < 4u * nd; i++) b[i] = fills[fill][i & 3u];
    if (len) memcpy(b + off, text, len);
    const RdField got = rd_parse9(col, off, len);
    free(col);
    cases++;
    if (len > 9u) return 0;
    Ref want = ref_short(text, len);
    want.lead = (want.lead & 1u) ? want.lead : 0u;                 // nw_tok asks "00..." first, then "0...": a zero behind another digit is none of its classes
    if (got.plain != want.plain || (want.plain && (got.value != want.value || got.lead != want.lead))) {
        printf("FAIL len %u off %u fill %u text '%.*s': got plain %u value %u lead %u, want %u %u %u\n", len, off, fill, (int)len, (const char*)text,
               got.plain, got.value, got.lead, want.plain, want.value, want.lead);
        return 1;
    }
    return 0;
}
static int check_all_places(const u8* text, u32 len) {
    for (u32 off = 0; off < 12; off++)
        for (u32 fill = 0; fill < 3; fill++)
            if (check(text, len, off, fill)) return 1;
    return 0;
}
static void digits_of(u8* t, u32 len, u64 v) { for (u32 j = len; j-- > 0;) { t[j] = (u8)('0' + v % 10); v /= 10; } }

// put_u_rows' loop, its symbols written down: (row - row0) << 8 | sym
static u32 ref_put_u(u64 num, u32* out) {
    const u32 n = num <= 0x7f ? 1u : num < 0x7ffe ? 2u : num < (1ULL << 32) ? 6u : 10u;
    for (u32 j = 0; j < n; j++) {
        u32 row, sym;
        if (j == 0)      { row = 0; sym = n == 1 ? (u32)num : n == 2 ? (0xff & (0x80 | (u32)(num >> 8))) : 0xffu; }
        else if (j == 1) { row = 1; sym = n == 2 ? (0xff & (u32)num) : n == 6 ? 0xfeu : 0xffu; }
        else             { row = (n == 6 ? 2 : 6) + (j - 2); sym = 0xff & (u32)(num >> (8 * (j - 2))); }
        out[j] = row << 8 | sym;
    }
    return n;
}
static u32 closed_put_u(u64 num, u32* out) {                       // chains.hip tok_put_u
    const u32 n = rd_u_count(num);
    u32 k = 0;
    out[k++] = rd_u_sym0(n, num);
    if (n >= 2u) out[k++] = 1u << 8 | rd_u_sym1(n, num);
    if (n >= 6u) {
        const u32 r = n == 6u ? 2u : 6u, lo = (u32)num;
        out[k++] = r << 8 | (lo & 0xffu); out[k++] = (r + 1) << 8 | ((lo >> 8) & 0xffu); out[k++] = (r + 2) << 8 | ((lo >> 16) & 0xffu); out[k++] = (r + 3) << 8 | (lo >> 24);
    }
    if (n == 10u) { const u32 hi = (u32)(num >> 32); for (u32 j = 0; j < 4; j++) out[k++] = (10 + j) << 8 | ((hi >> (8 * j)) & 0xffu); }
    return k;
}

int main() {
    u8 t[16];
    // 1. all-digit fields
    if (check_all_places(t, 0)) return 1;
    for (u32 len = 1; len <= 5; len++) {
        u64 top = 1; for (u32 j = 0; j < len; j++) top *= 10;
        for (u64 v = 0; v < top; v++) { digits_of(t, len, v); if (check_all_places(t, len)) return 1; }
    }
    srand(11);
    for (u32 len = 6; len <= 10; len++)
        for (u32 trial = 0; trial < 1000000; trial++) {
            const int lead = rand() % 8;                           // leading zeros often: "0...", "00...", and all zeros now and then
            for (u32 j = 0; j < len; j++) t[j] = (u8)('0' + rand() % 10);
            if (lead == 0) t[0] = '0';
            if (lead == 1) t[0] = t[1] = '0';
            if (lead == 2) for (u32 j = 0; j + 1 < len; j++) t[j] = '0';
            if (lead == 3) for (u32 j = 0; j < len; j++) t[j] = '9';
            if (check(t, len, (u32)rand() % 12u, (u32)rand() % 3u)) return 1;
        }
    printf("all-digit fields: lengths 0 .. 10, %ld columns agree with the byte loop\n", cases);
    // 2. one non-digit
    static const u8 odd[] = {'/', ':', ' ', '.', 'a', 'f', 'A', 'F', 'x', '_', 0x00, 0x01, 0x0a, 0x7f, 0x80, 0xb0, 0xb5, 0xb9, 0xff, '0' - 16, '9' + 16, '0' ^ 0x40};
    const long before = cases;
    for (u32 len = 1; len <= 10; len++)
        for (u32 pos = 0; pos < len; pos++)
            for (u32 k = 0; k < sizeof(odd); k++)
                for (u32 trial = 0; trial < 50; trial++) {
                    for (u32 j = 0; j < len; j++) t[j] = (u8)('0' + (trial ? rand() % 10 : 0));
                    t[pos] = odd[k];
                    if (check_all_places(t, len)) return 1;
                }
    printf("one non-digit: every position of lengths 1 .. 10, %ld columns\n", cases - before);
    // 3. a number's symbols
    static const u64 edge[] = {0, 1, 0x7f, 0x80, 0xff, 0x100, 0x7ffd, 0x7ffe, 0x7fff, 0x8000, 0xffff, 0xffffffffull, 0x100000000ull, 0x123456789abcdef0ull, ~0ull};
    long nums = 0;
    for (u32 e = 0; e < sizeof(edge) / sizeof(edge[0]); e++)
        for (int d = -3; d <= 3; d++) {
            const u64 num = edge[e] + (u64)(i64)d;
            u32 a[10], c[10];
            const u32 na = ref_put_u(num, a), nc = closed_put_u(num, c);
            if (na != nc || memcmp(a, c, 4u * na)) { printf("FAIL put_u %llx: %u symbols against %u\n", (unsigned long long)num, nc, na); return 1; }
            nums++;
        }
    for (u32 trial = 0; trial < 1000000; trial++) {
        const u64 num = (((u64)rand() << 40) ^ ((u64)rand() << 20) ^ (u64)rand()) >> (rand() % 64);
        u32 a[10], c[10];
        const u32 na = ref_put_u(num, a), nc = closed_put_u(num, c);
        if (na != nc || memcmp(a, c, 4u * na)) { printf("FAIL put_u %llx: %u symbols against %u\n", (unsigned long long)num, nc, na); return 1; }
        nums++;
    }
    printf("put_u in closed form: %ld numbers agree with the loop\nok\n", nums);
    return 0;
}

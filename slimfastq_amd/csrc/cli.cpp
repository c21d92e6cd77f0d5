// cli.cpp -- `slimfastq-amd`: the reference's command line (config.cpp:161-277) over the C ABI.
//
//   -u fastq  -f file.sfq  -d  -O  -l N | -1..-4  -q  -s  -v  -h        (same meaning as the reference)
//   -B reads  : records per independent block (default 1024; 0 = one block = a format-6 file the
//               reference itself can decode)
//   -A        : adaptive tables (every block runs the reference's per-symbol table updates) instead of the default
//               frozen tables (rows built by counting passes, one chain per GPU lane)
//   -g dev    : HIP device
//   -K        : store the CRC-32 of every block's text ("blk.crc") and of the file (info key "crc32"); a decode checks them
//   -Y        : count the statistics of the text on the GPU while it is coded and store them ("txt.stat"); -s prints them
//   -Q name   : LOSSY, encode only: bin the qualities on the GPU before they are coded (illumina8: 8 levels, novaseq4: 4 levels);
//               info keys "qlt.map" / "qlt.map.changed"
//   -R F:N    : with -d: records F .. F + N - 1 only (numbered from 0 over the archive) -- the blocks that hold them are decoded, no others
//   -p fastq  : paired files: the mates of -u's records; both are interleaved on the GPU and coded as one text (info key "usr.pair");
//               with -d: the second mates go here, the first to -u
//   -W F:N    : with -d and -p: pairs F .. F + N - 1 only (numbered from 0 over the archive), cut and split on the GPU
//   -M        : with -p on encode: the mates' names are compared on the GPU before a slab is coded; a mismatch ends the run
//   -k terms  : with -d: the records that pass a filter only (length, N count, mean quality, a motif, a sample), chosen on the GPU
//   -c terms  : with -d: every record trimmed on the GPU (crops, quality cuts from either end, a quality window, a 3' adapter), in front of -k
//   -o terms  : with -d: the mates of every pair overlapped on the GPU, the read-through behind the insert cut, the insert sizes counted;
//               behind -c, in front of -k; with the term merge=PATH instead: every pair whose mates overlap merged into ONE record on the
//               GPU (consensus bases, combined qualities) and written to PATH, behind -k; the other pairs go where they go without it
//   -D        : with -d: duplicates dropped on the GPU -- the first record (pair) of every base line (pair of base lines) only, over the
//               whole archive: one set of keys in device memory lasts the run; behind -k, in front of merge=, -p and -x
//   -G terms  : with -d: the reads screened against reference sequences on the GPU -- those that share k-mers with the FASTA files
//               named by ref=PATH dropped (phiX, adapters, rRNA, a host genome), or with the term keep only those kept (baits); one
//               set of k-mers in device memory lasts the run; behind -k, in front of -D, merge=, -p and -x
//   -X terms  : with -d: the reads demultiplexed on the GPU -- sorted by the sample of a sheet whose barcode they carry in the header's
//               index field or inline, within mm= mismatches, a file a sample (out=PREFIX), the rest to -u (and -p); behind -D, last
// All model / coder work happens in libslimfastq_amd.so on the GPU; this file parses arguments, reads and
// writes files and fills the info page.
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "container.h"

static const int   kInternalVersion = 6;      // config.cpp:41
using sfqc::kBlockVersion;                       // the block format's "version" (container.h)
using sfqc::kBlockVersionMin;
static const char* kUserVersion = "2.04-amd";

static bool g_encode = true;
static bool g_batch = false;                  // -b: jobs from stdin, one context for all of them; errors end the job, not the process
static std::string g_usr;

struct JobError { std::string msg; };

// SFQ_TIMING=1: where a run spends its wall time (stderr)
#include <chrono>
#include <thread>
#include <atomic>
static bool g_timing = false;                 // -z: phase timings on stderr
static void tick(const char* what) {
    static auto t0 = std::chrono::steady_clock::now(), last = t0;
    if (!g_timing) return;
    const auto now = std::chrono::steady_clock::now();
    fprintf(stderr, "[timing] %-28s +%7.3f s  (%7.3f s)\n", what, std::chrono::duration<double>(now - last).count(), std::chrono::duration<double>(now - t0).count());
    last = now;
}

static std::string g_partial;                // an archive being written as the slabs come back: a failed job removes it
[[noreturn]] static void croak(const char* fmt, ...) {                 // config.cpp:54-68
    char msg[1024];
    va_list ap; va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    if (!g_partial.empty()) { unlink(g_partial.c_str()); g_partial.clear(); }
    // (thrown in one-shot mode too: the stack unwinds through the guards below, which join the reader / writer threads
    //  before main() prints the message and exits -- exit() from here would race a thread still inside pwrite / fwrite)
    throw JobError{msg};
}
// a thread that is joined wherever its scope ends, croak()'s unwinding included (a joinable std::thread that goes out of
// scope calls std::terminate)
struct Joiner {
    std::thread t;
    ~Joiner() { join(); }
    void join() { if (t.joinable()) t.join(); }
    template <typename F> void start(F&& f) { join(); t = std::thread(std::forward<F>(f)); }
};

static void usage() {
    printf("Usage: \n"
           "-u  usr-filename : (default: stdin)\n"
           "-f comp-filename : required - compressed\n"
           "-d               : decode (instead of encoding) \n"
           "-O               : silently overwrite existing files\n"
           "-l level         : compression level 1 to 4 (default is 3 ) \n"
           "-1, -2, -3, -4   : alias for -l 1, -l 2, etc \n"
           "-B reads         : records per independent GPU block (default: about 376 KiB of text, i.e. 1024 reads of 150 bp;\n"
           "                   0 = single block, reference-compatible file)\n"
           "-A               : adaptive tables: every block updates its rows per symbol, as the reference does (slower)\n"
           "-F               : frozen tables, built by counting passes, one coding chain per GPU lane\n"
           "                   default: -F from 64 MiB of text on, -A in blocks of 65536 reads below that (the priors\n"
           "                   frozen tables transmit weigh too much on a small file)\n"
           "-C reads         : frozen tables: records per chain (default: automatic)\n"
           "-K               : checksums: store the CRC-32 of every block's text and of the whole file (computed on the GPU);\n"
           "                   decoding checks them and fails on a mismatch (needs the block format: not with -B 0)\n"
           "-Y               : text statistics: count bases, GC / N share, Q20 / Q30 share, read lengths and the mean quality per cycle\n"
           "                   on the GPU while the text is coded, and store them in the archive; -s prints them (works with -B 0 too)\n"
           "-Q illumina8|novaseq4 : LOSSY: bin the qualities on the GPU before they are coded -- Illumina's 8 levels or NovaSeq's 4\n"
           "                   (Phred+33; Q0 and Q1 stay) -- the archive holds, checks (-K) and counts (-Y) the binned text; -s names\n"
           "                   the map and the bytes it changed (encode only; works with -B 0)\n"
           "-R first:count   : with -d: write records first .. first+count-1 only (numbered from 0 over the whole archive; count is\n"
           "                   clipped at the end): only the blocks that hold them are decoded (and, under a base model, what the\n"
           "                   format makes them depend on); with -b: of every job\n"
           "-p fastq         : paired files: record i of this file is the mate of record i of -u; the two are interleaved on the GPU\n"
           "                   (R1 R2 R1 R2 ...) and coded as one text, so a mate's header costs the one field that differs; with -d:\n"
           "                   the first mates are written to -u, the second mates here (the archive must have been written with -p;\n"
           "                   without -p it decodes to interleaved FASTQ); needs -u, not with -b or -R\n"
           "-W first:count   : with -d and -p: write pairs first .. first+count-1 only (numbered from 0 over the whole archive; count is\n"
           "                   clipped at the end): first mates to -u, second mates to -p; only the blocks that hold them are decoded,\n"
           "                   and they are cut to the pairs and split on the GPU; needs -d, -u and -p, not with -R or -b\n"
           "-x fasta|names|bases|quals : with -d: write those lines of every record only, picked on the GPU before the text comes back --\n"
           "                   FASTA (lines 1 and 2, '>' for '@'), the names (line 1 without its '@'), the base lines or the quality lines;\n"
           "                   goes with -R, -p, -W, -K and -b (-p and -W write each mate's lines to its file)\n"
           "-k terms         : with -d: write only the records that pass a filter, chosen on the GPU before the text comes back; terms is a\n"
           "                   comma-separated list of minlen=N, maxlen=N (bases), maxn=N (N bases at most), meanq=Q (mean quality at least Q,\n"
           "                   Phred+33, up to two fraction digits), seq=MOTIF (the base line holds it; at most 32 of ACGT, either case), rc\n"
           "                   (or its reverse complement), invert (the records that fail), sample=F[:SEED] (a reproducible share 0 < F < 1)\n"
           "                   and either; an archive written with -p keeps or drops whole pairs: where both mates pass, with either where\n"
           "                   one does; goes with -R, -W, -p, -x, -K and -b; without -q one line on stderr says what was kept\n"
           "-c terms         : with -d: trim every record on the GPU before the text comes back, and before -k judges it; terms is a\n"
           "                   comma-separated list of head=N, tail=N (bases cropped), maxlen=N (bases kept at most), q5=Q, q3=Q (cut the\n"
           "                   bases in front of the first / behind the last quality of at least Q, Phred+33), win=W:Q (cut from the first\n"
           "                   window of W <= 32 bases whose mean quality is below Q), adapter=SEQ (cut from where it begins; at most 32 of\n"
           "                   ACGT), mm=N (mismatches allowed over its length) and overlap=N (bases of it that count at the read's end,\n"
           "                   default 3); no record is dropped (-k minlen= does that); goes with -R, -W, -p, -x, -k, -K and -b, not with\n"
           "                   -s; without -q one line on stderr says what was cut\n"
           "-o terms         : with -d, of an archive of pairs: overlap the mates of every pair on the GPU (read 1 against the reverse complement\n"
           "                   of read 2) and cut what lies behind the insert off both, the adapter read through into, whatever it is;\n"
           "                   behind -c and before -k judges the records; terms is a comma-separated list of min=N (bases that must overlap,\n"
           "                   default 30), mm=N (mismatches at most, default 5), pct=N (and at most that share of the overlap, default 20),\n"
           "                   nocut (count only, the text stays) and hist=PATH (the insert sizes as 'insert<TAB>pairs' lines; insert 0: no\n"
           "                   overlap found), or the word default; no record is dropped; goes with -R, -W, -p, -x, -k, -c and -K, not\n"
           "                   with -s or -b; without -q one line on stderr says what was found\n"
           "                   merge=PATH among the terms: instead of cutting, every pair that has such an overlap is merged into one record\n"
           "                   -- read 1's name, the insert's bases (where the mates differ the base of the higher quality), the combined\n"
           "                   qualities -- and appended to PATH; the pairs that do not merge go to -u (and -p) as without it; behind -c and\n"
           "                   -k, which judges the mates; hist= and the line on stderr then speak of the merged pairs; goes with -W, -p, -x\n"
           "                   (PATH too), -k, -c and -K, with -R where the range is whole pairs (an even first record and count: -W\n"
           "                   says it in pairs), not with nocut\n"
           "-D               : with -d: write only the first record of every base line (letter case aside; names and qualities play no\n"
           "                   part), duplicates dropped on the GPU before the text comes back, over the whole archive: one hash set in\n"
           "                   device memory lasts the run; of an archive written with -p, or with -p / -W: the first pair of every pair\n"
           "                   of base lines; behind -c, -o and -k, in front of merge=, -p and -x; under -R / -W only the window's records\n"
           "                   count; goes with -R, -p, -W, -x, -k, -c, -o and -K, not with -s or -b; without -q the last line on stderr\n"
           "                   says what was kept\n"
           "-G terms         : with -d: screen the reads against reference sequences on the GPU before the text comes back: ref=PATH (a\n"
           "                   FASTA file; the term may be repeated) names the references, whose k-mers of either strand go into one set\n"
           "                   in device memory that lasts the run; k=N (4 .. 31, default 27) their length; a read is MATCHED when at\n"
           "                   least hits=N (default 1) of its k-mers, and at least pct=N percent of them (default 0), are in the set.\n"
           "                   Matched reads are dropped (phiX, adapters, rRNA, a host genome); with the term keep only they are written\n"
           "                   (baits).  Of an archive written with -p, or with -p / -W, a pair is matched when either mate is; with the\n"
           "                   term both, when both mates are.  Behind -c, -o and -k, in front of -D, merge=, -p and -x; under -R / -W only\n"
           "                   the window's records count; goes with -R, -p, -W, -x, -k, -c, -o, -D and -K, not with -s or -b; without\n"
           "                   -q the last line on stderr says what was matched and kept\n"
           "-X sheet[,terms] : with -d: demultiplex the reads on the GPU before the text comes back.  sheet: a file of lines name<TAB>BARCODE or\n"
           "                   name<TAB>BARCODE+BARCODE ('#' lines are comments).  out=PREFIX (required): sample files PREFIX<name>.fastq, with\n"
           "                   -p PREFIX<name>_R1.fastq and _R2.fastq; the units no sample takes go to -u (and -p).  mm=N: mismatches allowed\n"
           "                   (default 1; a unit whose nearest barcode is not unique is unassigned); hdr (the default): the barcode is the\n"
           "                   last ':' field of the header, a second part behind its '+'; inline[=POS]: it is in the read's bases at POS (a\n"
           "                   second part follows it); inline2[=POS]: the second part in the second mate's bases (needs -p); hdr2: the second\n"
           "                   part in the header's field; clip: inline barcodes are cut from the reads of assigned units; counts=FILE:\n"
           "                   name<TAB>barcode<TAB>units per sample.  Behind -c, -o, -k, -G and -D, the last pass; goes with -R, -p, -k, -c,\n"
           "                   -o, -D, -G and -K, not with -x, -W, -o merge=, -s, -b or a -B 0 archive; without -q the last line on stderr\n"
           "                   says how many units were assigned\n"
           "-M               : with -p on a compress run: compare the names of every pair of mates on the GPU before it is coded (the\n"
           "                   header's first word, without a final /1 or /2); a pair that differs ends the run with its index and both\n"
           "                   names, and no archive is written\n"
           "-S mbytes        : input is compressed in slabs of this many MiB, one archive segment each (default 512 for a\n"
           "                   regular file, read ahead while the GPU codes the slab before; 2048 for a pipe)\n"
           "-t threads       : threads reading a slab (default 6)\n"
           "-Z               : with -d: every FASTQ, FASTA or line file the run writes is BGZF (blocked gzip, what bgzip writes; any gzip\n"
           "                   reader reads it), deflated on the GPU as the call's last pass: -u, -p, merge=PATH, the outputs of -x and the\n"
           "                   sample files of -X, whose names gain .gz; the names of -u and -p are taken as given.  Every file ends with\n"
           "                   the end-of-file block, an empty result is that block alone (28 bytes).  hist= and counts= stay text.  Not\n"
           "                   with -R, which cuts the decoded text on the host (-W cuts on the device and works); without -q the last\n"
           "                   line on stderr says text bytes, compressed bytes and members\n"
           "-z               : print the time of every phase on stderr\n"
           "-g device        : HIP device index (default 0)\n"
           "-T percent       : share of the device memory this process may use for model tables (several processes on one GPU)\n"
           "-b               : batch: read '<fastq>\\t<sfq>' jobs (with -d: '<sfq>\\t<fastq>') from stdin, answer 'ok|fail\\t...' per job on stdout\n"
           "-v               : version : internal version \n"
           "-h               : help : this message \n"
           "-s               : stat : information about a compressed file \n"
           "-q               : suppress extra stats info that could have been seen by -s \n"
           "\nslimfastq-amd A B : compress A (a fastq file) to B, or decompress A (a slimfastq file) to B / stdout\n");
    exit(0);
}

static int clamp_level(int l) { return l > 4 ? 4 : l < 1 ? 1 : l; }   // config.cpp:232-237
static int level_gen_bits(int level) { switch (level) { case 1: return 18; case 2: return 22; case 3: return 24; default: return 26; } }

struct Opts {
    int level = 3, device = 0;
    long block_reads = -1;                                             // -1 = automatic (about 376 KiB of text per block)
    bool overwrite = false, quiet = false;
    uint64_t slab_bytes = 0;                      // -S; 0 = 512 MiB for a regular file (read ahead into pinned buffers), 2 GiB otherwise
    int io_threads = 6;                           // -t: threads that read a slab
    int table_pct = 0;                                                 // -T: share of the device memory for model tables (0 = the library's default)
    bool adaptive = false;                                             // -A
    bool force_frozen = false;                                         // -F
    long chain_reads = 0;                                              // -C
    bool checksum = false;                                             // -K
    bool stats = false;                                                // -Y
    bool range = false; uint64_t r_first = 0, r_count = 0;             // -R first:count
    int qmap = 0; std::string qmap_name;                               // -Q: SFQ_QMAP_* (0 = none) and its name
    std::string pair;                                                  // -p: the second file of a pair
    bool window = false; uint64_t w_first = 0, w_count = 0;            // -W first:count (pairs)
    bool mates = false;                                                // -M
    int pick = 0; std::string pick_name;                               // -x: SFQ_PICK_* (0 = none, -1 = no such word) and the word
    bool select = false; std::string select_spec;                      // -k terms
    sfq_select sel; bool sel_either = false;                           // ... parsed: the rule (its range and pairs are the decode's), `either`
    bool trim = false; std::string trim_spec; sfq_trim trim_rule;      // -c terms, and the rule they parse to
    bool ovl = false; std::string ovl_spec, ovl_hist; sfq_overlap ovl_rule;        // -o terms, the hist=PATH among them, and the rule the others parse to
    std::string ovl_merge;                                             // ... and the merge=PATH: the pairs are merged, not cut
    bool dedup = false;                                                // -D
    bool screen = false; std::string screen_spec; sfq_screen screen_rule; uint32_t screen_k = 27;       // -G terms, and the rule and k they parse to
    bool bgzf = false;                                                 // -Z: every text file a decode writes is BGZF
    bool demux = false; std::string demux_spec; sfq_demux demux_rule;  // -X terms, and the rule they and the sheet give
    std::vector<std::string> demux_names; std::vector<uint8_t> demux_codes;       // ... the sheet's samples: names, barcode rows
    std::string demux_out, demux_counts;                               // ... out=PREFIX, counts=FILE
    std::vector<std::vector<uint8_t>> screen_seqs;                     // ... and the sequence text of every ref=PATH, read before anything is decoded
};
// "FIRST:COUNT", both decimal, COUNT > 0
static bool parse_range(const char* t, uint64_t& first, uint64_t& count) {
    if (!t || *t < '0' || *t > '9') return false;
    char* e = nullptr;
    errno = 0;
    const unsigned long long f = strtoull(t, &e, 10);
    if (errno || !e || *e != ':' || e[1] < '0' || e[1] > '9') return false;
    char* e2 = nullptr;
    const unsigned long long c = strtoull(e + 1, &e2, 10);
    if (errno || !e2 || *e2 || !c) return false;
    first = f; count = c;
    return true;
}
// the name of the record whose header line begins at t[off] (slimfastq_amd.h: mates by name), cut at 64 bytes, for a message
static std::string mate_name(const uint8_t* t, size_t n, uint64_t off) {
    if (off >= n || t[off] == '\n') return "";
    size_t b = (size_t)off + 1, e = b;
    while (e < n && t[e] != '\n' && t[e] != ' ' && t[e] != '\t') e++;
    if (e - b >= 2 && t[e - 2] == '/' && (t[e - 1] == '1' || t[e - 1] == '2')) e -= 2;
    std::string s((const char*)t + b, std::min<size_t>(e - b, 64));
    for (char& c : s) if ((unsigned char)c < 32 || (unsigned char)c > 126) c = '?';
    return s;
}
// where the first `skip` records (four lines each; of picked lines, -x: two or one) of a text end, or n where it has fewer
static size_t records_end(const uint8_t* t, size_t n, uint64_t skip, uint64_t lines = 4) {
    size_t at = 0;
    for (uint64_t l = 0; l < lines * skip && at < n; l++) {
        const void* q = memchr(t + at, '\n', n - at);
        at = q ? (size_t)((const uint8_t*)q - t) + 1 : n;
    }
    return at;
}

// Growable byte buffer that never zero-fills (a std::vector would touch gigabytes just to size them).
struct Bytes {
    uint8_t* p = nullptr; size_t n = 0, cap = 0, touched = 0;
    ~Bytes() { free(p); }
    // Fault the first `upto` bytes in now: a device-to-host copy into pages the process has never touched goes
    // through the driver page by page and is ~10x slower than touching them here first (measured).
    void touch(size_t upto) {
        if (upto > cap) upto = cap;
        for (size_t i = touched & ~(size_t)4095; i < upto; i += 4096) p[i] = 0;
        if (upto > touched) touched = upto;
    }
    bool reserve(size_t want) {
        if (want <= cap) return true;
        uint8_t* q = (uint8_t*)realloc(p, want);
        if (!q) return false;
        p = q; cap = want; touched = std::min(touched, n);               // realloc may have moved to fresh pages
        return true;
    }
};
// Fill `buf` (which may hold a carried-over tail) up to `want` bytes; returns false on a read error.
static bool fill(FILE* f, Bytes& buf, size_t want, bool& eof) {
    if (!buf.reserve(want)) return false;
    while (buf.n < want) {
        const size_t got = fread(buf.p + buf.n, 1, want - buf.n, f);
        if (got == 0) { eof = true; break; }
        buf.n += got;
    }
    return !ferror(f);
}
// Bytes of [p, p+n) that hold whole records (a record is four lines), given that p starts at a record and [p, p+n) holds nl
// newlines: the partial last line goes, and nl % 4 lines more.
static size_t whole_records(const uint8_t* p, size_t n, uint64_t nl) {
    size_t drop = (size_t)(nl & 3), end = n;
    while (end > 0 && p[end - 1] != '\n') end--;
    while (drop && end > 0) { end--; while (end > 0 && p[end - 1] != '\n') end--; drop--; }
    return end;
}

// [0, n) ends at a line end or at the end of a file: the same without its last `drop` records (four lines each)
static size_t drop_records(const uint8_t* p, size_t end, uint64_t drop) {
    for (uint64_t l = 0; l < 4 * drop && end > 0; l++) { end--; while (end > 0 && p[end - 1] != '\n') end--; }
    return end;
}
// the lines of [p, p + n): a text without a final '\n' ends in a line all the same
static uint64_t count_lines(const uint8_t* p, size_t n) {
    return (uint64_t)std::count(p, p + n, (uint8_t)'\n') + (n && p[n - 1] != '\n');
}

// One finished library call (a segment of raw bytes of text) into the archive's index.
static void collect(sfq_ctx* ctx, const sfq_result& res, uint64_t raw, sfqc::SegmentedIndex& idx, bool checksum, bool stats) {
    std::vector<sfq_block_info> blocks(res.n_blocks);
    sfq_get_block_index(ctx, blocks.data(), res.n_blocks);
    std::vector<uint8_t> first((size_t)res.first_hdr_bytes + 1);
    sfq_get_first_headers(ctx, first.data(), res.first_hdr_bytes);
    auto blob = [ctx](int64_t (*get)(sfq_ctx*, uint8_t*, uint64_t)) {
        std::vector<uint8_t> v((size_t)std::max<int64_t>(0, get(ctx, nullptr, 0)));
        if (!v.empty()) get(ctx, v.data(), v.size());
        return v;
    };
    const std::vector<uint8_t> pri = blob(sfq_get_qlt_prior), chn = blob(sfq_get_chain_index), rpr = blob(sfq_get_rec_prior);
    sfq_segment g; memset(&g, 0, sizeof g);
    g.blocks = blocks.data(); g.n_blocks = res.n_blocks; g.first_hdrs = first.data(); g.first_hdr_bytes = res.first_hdr_bytes;
    g.qlt_prior = pri.data(); g.qlt_prior_bytes = pri.size(); g.chain_index = chn.data(); g.chain_index_bytes = chn.size();
    g.rec_prior = rpr.data(); g.rec_prior_bytes = rpr.size(); g.raw_bytes = raw;
    std::vector<uint32_t> crc;
    uint32_t text_crc = 0;
    if (checksum) {                                                    // -K: the call's checksums (sfq_ctx_set_checksums in encode_file)
        crc.resize(res.n_blocks + 1);
        if (sfq_get_checksums(ctx, crc.data(), res.n_blocks, &text_crc) != (int)res.n_blocks) croak("checksums: the library returned none for this call");
    }
    sfq_text_stats ts;
    if (stats && sfq_get_text_stats(ctx, &ts) != 1) croak("text statistics: the library returned none for this call");   // -Y (sfq_ctx_set_stats in encode_file)
    idx.add(g, checksum ? crc.data() : nullptr, text_crc, stats ? &ts : nullptr);
}

// -s: the third section, from "txt.stat" (archives written with -Y)
static void print_text_stats(const std::vector<uint8_t>& bytes) {
    sfq_text_stats t;
    fprintf(stderr, "\n:::: Text ::::\n");
    if (!sfqc::unpack_text_stats(bytes, t)) { fprintf(stderr, "txt.stat: damaged (%zu bytes): no text statistics\n", bytes.size()); return; }
    auto row = [](const char* key, const std::string& val) { fprintf(stderr, "%-16s = %s\n", key, val.c_str()); };
    auto fixed = [](double v, int digits) { char b[64]; snprintf(b, sizeof b, "%.*f", digits, v); return std::string(b); };
    auto pct = [&](uint64_t part, uint64_t all) { return fixed(all ? 100.0 * (double)part / (double)all : 0.0, 2); };
    row("records", std::to_string(t.n_records));
    row("bases", std::to_string(t.seq_bytes));
    row("seq_len_min", std::to_string(t.seq_len_min));
    row("seq_len_max", std::to_string(t.seq_len_max));
    row("seq_len_mean", fixed(t.n_records ? (double)t.seq_bytes / (double)t.n_records : 0.0, 2));
    row("gc_pct", pct(t.seq_hist['G'] + t.seq_hist['C'] + t.seq_hist['g'] + t.seq_hist['c'], t.seq_bytes));
    row("n_pct", pct(t.seq_hist['N'] + t.seq_hist['n'] + t.seq_hist['.'], t.seq_bytes));
    uint64_t q20 = 0, q30 = 0;
    int qmin = -1, qmax = -1;
    for (int b = 0; b < 256; b++) {
        if (b >= '5') q20 += t.qlt_hist[b];
        if (b >= '?') q30 += t.qlt_hist[b];
        if (t.qlt_hist[b]) { if (qmin < 0) qmin = b; qmax = b; }
    }
    row("q20_pct", pct(q20, t.qlt_bytes));
    row("q30_pct", pct(q30, t.qlt_bytes));
    row("qlt_min", qmin < 0 ? std::string() : std::string(1, (char)qmin));
    row("qlt_max", qmax < 0 ? std::string() : std::string(1, (char)qmax));
    std::string cyc;
    int last = -1;
    for (int c = 0; c < SFQ_STATS_CYCLES; c++) if (t.cyc_n[c]) last = c;
    auto mean_q = [&](int c) { return fixed(t.cyc_n[c] ? (double)t.cyc_qsum[c] / (double)t.cyc_n[c] - 33.0 : 0.0, 1); };
    for (int c = 0; c <= last; c++) { if (c) cyc += ","; cyc += mean_q(c); }
    if (t.cyc_n[SFQ_STATS_CYCLES]) { if (!cyc.empty()) cyc += ","; cyc += mean_q(SFQ_STATS_CYCLES); }
    row("cycle_mean_q", cyc);
}

static void encode_file(sfq_ctx* ctx, const Opts& o, const std::string& usr, const std::string& fil) {
    if (!o.overwrite && access(fil.c_str(), F_OK) == 0) {
        if (g_batch) croak("Can't write file '%s': File exists", fil.c_str());
        fprintf(stderr, "Can't write file '%s': File exists\n", fil.c_str()); exit(1);
    }
    FILE* in = usr.empty() ? stdin : fopen(usr.c_str(), "rb");
    if (!in) {
        if (g_batch) croak("Can't read file '%s'", usr.c_str());
        fprintf(stderr, "Can't read file '%s'\n", usr.c_str()); exit(1);
    }
    const bool paired = !o.pair.empty();
    FILE* in2 = paired ? fopen(o.pair.c_str(), "rb") : nullptr;
    if (paired && !in2) { fprintf(stderr, "Can't read file '%s'\n", o.pair.c_str()); exit(1); }
    const bool legacy = o.block_reads == 0;
    if (sfq_ctx_set_checksums(ctx, o.checksum ? 1 : 0)) croak("%s", sfq_last_error(ctx));
    if (sfq_ctx_set_stats(ctx, o.stats ? 1 : 0)) croak("%s", sfq_last_error(ctx));
    if (sfq_ctx_set_mate_check(ctx, o.mates ? 1 : 0)) croak("%s", sfq_last_error(ctx));
    uint8_t qlut[256];
    if (o.qmap && sfq_quality_map_preset(o.qmap, qlut)) croak("-Q: no such preset");
    if (sfq_ctx_set_quality_map(ctx, o.qmap ? qlut : nullptr)) croak("%s", sfq_last_error(ctx));      // (a -b worker's context: set for every job)
    uint64_t qmap_changed = 0;                                         // over the slabs
    sfq_params p; memset(&p, 0, sizeof p);
    p.level = o.level; p.block_reads = o.block_reads < 0 ? SFQ_BLOCK_AUTO : (uint32_t)o.block_reads;
    p.prior_step = legacy ? 0 : SFQ_PRIOR_AUTO;                        // warm start needs the block format
    // tables: by the size of the text unless asked for (one decision per file: the first slab's size stands for a pipe's)
    bool frozen = !legacy && !o.adaptive;
    bool tables_decided = legacy || o.adaptive || o.force_frozen;
    p.tables = frozen ? SFQ_TABLES_FROZEN : SFQ_TABLES_ADAPTIVE;
    p.chain_reads = (uint32_t)std::max(0l, o.chain_reads);

    std::vector<uint8_t> streams[SFQ_NSTREAMS];
    sfqc::SegmentedIndex idx;                                          // one segment per library call
    // (Mapping the file and handing the mapping to the library was measured: the copy engine pins page-cache pages one
    //  by one, 4-10x slower than reading into an ordinary buffer first.)
    size_t file_left = SIZE_MAX;                                       // bytes not yet read, when the input is a regular file
    if (in != stdin) { struct stat st; if (fstat(fileno(in), &st) == 0 && S_ISREG(st.st_mode)) file_left = (size_t)st.st_size; }
    if (paired && file_left != SIZE_MAX) {                             // (the text that is coded: both files)
        struct stat st;
        if (fstat(fileno(in2), &st) == 0 && S_ISREG(st.st_mode)) file_left += (size_t)st.st_size; else file_left = SIZE_MAX;
    }
    auto decide_tables = [&](uint64_t text_bytes) {
        if (tables_decided) return;
        tables_decided = true;
        frozen = text_bytes >= (64ull << 20);
        p.tables = frozen ? SFQ_TABLES_FROZEN : SFQ_TABLES_ADAPTIVE;
        if (!frozen) { p.prior_step = 0; if (o.block_reads < 0) p.block_reads = 65536; }      // include/slimfastq_amd.h SFQ_TABLES_AUTO
    };
    if (file_left != SIZE_MAX) decide_tables(file_left);
    // A one-shot process pays for every byte of model tables it allocates (device allocations of tens of GB take
    // seconds), and its time is file I/O anyway: size the tables for a fraction of the block slots the text could use.
    if (!g_batch) {
        const uint64_t slab0 = o.slab_bytes ? o.slab_bytes : (!legacy && in != stdin && file_left != SIZE_MAX) ? (512ull << 20) : (2048ull << 20);
        const uint64_t text = std::min<uint64_t>(file_left == SIZE_MAX ? slab0 : file_left, legacy ? UINT64_MAX : slab0);
        uint64_t budget = std::max<uint64_t>(2ull << 30, 8 * text);
        if (o.table_pct) budget = std::min<uint64_t>(budget, sfq_ctx_device_memory(ctx) / 100 * (uint64_t)o.table_pct);
        sfq_ctx_set_table_budget(ctx, budget);
    }
    // A regular file in the block format: slabs are read AHEAD -- several threads pread the next slab into one of two
    // page-locked buffers while the GPU codes the current one -- and the streams come back into a page-locked buffer too.
    // (File to file the time is the host's: one thread fread()s at ~5 GB/s, pageable H2D/D2H copies crawl.)
    bool ahead = !legacy && in != stdin && file_left != SIZE_MAX && !paired;      // (pairs: the plain loop below)
    size_t slab = (size_t)(o.slab_bytes ? o.slab_bytes : ahead ? (512ull << 20) : (2048ull << 20));
    // (a small file: buffers of its size, not of the slab's -- page-locking 1.5 GiB for a 1 MB file costs hundreds of
    //  milliseconds and may not fit a small memlock limit)
    if (ahead) slab = std::min(slab, std::max<size_t>(file_left, (size_t)1 << 20));
    // kept for the life of the process: a -b worker reuses them, a one-shot run exits without the 0.2 s of unpinning
    static uint8_t* pinned[4] = { nullptr, nullptr, nullptr, nullptr }; static size_t pinned_cap = 0;
    if (ahead) {
        const size_t cap = slab + (64u << 20), out_pin = cap / 3 + (16u << 20);
        if (pinned_cap < cap) {
            for (auto& q : pinned) { if (q) sfq_host_free(ctx, q); q = nullptr; }
            pinned[0] = (uint8_t*)sfq_host_alloc(ctx, cap); pinned[1] = (uint8_t*)sfq_host_alloc(ctx, cap);
            pinned[2] = (uint8_t*)sfq_host_alloc(ctx, out_pin); pinned[3] = (uint8_t*)sfq_host_alloc(ctx, out_pin);
            pinned_cap = (pinned[0] && pinned[1] && pinned[2] && pinned[3]) ? cap : 0;
            if (!pinned_cap) {                                             // no page-locked memory to be had: the plain path below
                for (auto& q : pinned) { if (q) sfq_host_free(ctx, q); q = nullptr; }
                ahead = false;
                slab = (size_t)(o.slab_bytes ? o.slab_bytes : (2048ull << 20));
            }
        }
    }
    Bytes fq, out;
    bool eof = false;
    sfqc::PagedWriter pw; bool streamed = false;                       // the archive written as the slabs come back
    if (ahead) {
        const int fd = fileno(in);
        const size_t fsize = file_left;
        const size_t cap = slab + (64u << 20);                          // room for the carried-over partial record
        const size_t out_cap = (size_t)sfq_encode_bound(cap);
        // the streams of a slab are rarely a third of its text: that much is page-locked, twice (one buffer is written to
        // the archive while the next slab's streams arrive in the other); a slab that needs more goes through a plain buffer
        const size_t out_pin = cap / 3 + (16u << 20);
        uint8_t* buf[2] = { pinned[0], pinned[1] };
        Bytes big_out;                                                  // only for a slab whose streams outgrow the pinned buffer
        std::string werr;
        if (!pw.open(fil, werr)) croak("%s", werr.c_str());
        g_partial = fil;
        int sid[SFQ_NSTREAMS];
        for (int s2 = 0; s2 < SFQ_NSTREAMS; s2++) sid[s2] = -1;           // a stream gets its directory entry with its first bytes
        Joiner writer;                                                  // appends the previous slab's streams to the archive
        int ob = 0;
        tick("pinned buffers");
        // read file bytes [off, off + len) to dst with o.io_threads threads; newlines counted on the way
        struct Read {
            std::vector<std::thread> th; std::atomic<uint64_t> nl{0}; std::atomic<int> bad{0};
            ~Read() { for (auto& t : th) if (t.joinable()) t.join(); }
        };
        auto start_read = [&](Read& r, uint8_t* dst, size_t off, size_t len) {
            r.nl = 0; r.bad = 0;
            const int nt = std::max(1, o.io_threads);
            const size_t per = ((len + nt - 1) / nt + 4095) & ~(size_t)4095;
            for (int t = 0; t < nt; t++) {
                const size_t a0 = std::min(len, per * t), a1 = std::min(len, per * (t + 1));
                if (a0 >= a1) break;
                r.th.emplace_back([&r, fd, dst, off, a0, a1]() {
                    size_t at = a0; uint64_t nl = 0;
                    while (at < a1) {
                        const ssize_t got = pread(fd, dst + at, std::min<size_t>(a1 - at, 8u << 20), (off_t)(off + at));
                        if (got <= 0) { r.bad = 1; return; }
                        for (const uint8_t* q = dst + at, *e = q + got; q < e; q++) nl += *q == '\n';
                        at += (size_t)got;
                    }
                    r.nl += nl;
                });
            }
        };
        auto join_read = [&](Read& r) { for (auto& t : r.th) t.join(); r.th.clear(); if (r.bad) croak("read error"); };
        size_t off = 0;                                                 // file bytes handed to a reader so far
        size_t have[2] = {0, 0}; uint64_t nls[2] = {0, 0};
        int cur = 0;
        {
            Read r; const size_t len = std::min(slab, fsize);
            start_read(r, buf[0], 0, len); join_read(r);
            have[0] = len; nls[0] = r.nl; off = len;
        }
        tick("read slab");
        while (have[cur]) {
            const bool last = off >= fsize;
            uint8_t* text = buf[cur];
            size_t use = have[cur];
            if (!last) {                                                // whole records only
                use = whole_records(text, use, nls[cur]);
                if (use == 0) croak("a record longer than the slab (%zu MiB): raise -S", slab >> 20);
            }
            // the next slab: the carried-over tail, then file bytes read by the threads while this one is coded
            const int nxt = cur ^ 1;
            const size_t carry = have[cur] - use;
            Read r;
            size_t len = 0;
            if (carry > (64u << 20)) croak("a record longer than 64 MiB next to a slab boundary: raise -S");
            memcpy(buf[nxt], text + use, carry);
            const uint64_t carry_nl = (uint64_t)std::count(buf[nxt], buf[nxt] + carry, (uint8_t)'\n');
            if (!last) { len = std::min(slab, fsize - off); start_read(r, buf[nxt] + carry, off, len); }
            sfq_result res;
            uint8_t* outp = pinned[2 + ob];
            int rc = sfq_encode_blocks_host(ctx, text, use, &p, outp, out_pin, &res);
            if (rc == SFQ_E_OVERFLOW) {
                if (!big_out.reserve(out_cap)) croak("out of memory");
                writer.join();
                outp = big_out.p;
                rc = sfq_encode_blocks_host(ctx, text, use, &p, outp, out_cap, &res);
            }
            if (rc) croak("%s", sfq_last_error(ctx));
            tick("sfq_encode_blocks_host");
            qmap_changed += sfq_get_quality_map_changed(ctx);
            collect(ctx, res, use, idx, o.checksum, o.stats);
            tick("collect slab");
            writer.join();
            {
                const sfq_result rr = res; sfqc::PagedWriter* w = &pw; int* ids = sid; const uint8_t* src = outp;
                writer.start([rr, w, ids, src]() {
                    for (int s2 = 0; s2 < SFQ_NSTREAMS; s2++) if (rr.stream_bytes[s2]) {
                        if (ids[s2] < 0) ids[s2] = w->stream(sfq_stream_name(s2));
                        w->append(ids[s2], src + rr.stream_offset[s2], (size_t)rr.stream_bytes[s2]);
                    }
                });
                if (outp == big_out.p) writer.join(); else ob ^= 1;
            }
            join_read(r);
            tick("wait for the next slab");
            have[nxt] = carry + len; nls[nxt] = carry_nl + r.nl; off += len;
            cur = nxt;
        }
        writer.join();
        streamed = true;
        eof = true;                                                     // nothing left for the loop below
    }
    // -p: up to half a slab of each file, both cut to the same number of whole records and interleaved on the GPU; both tails are
    // carried, so every archive segment holds whole pairs
    if (paired) {
        Bytes fb;
        bool eof2 = false;
        uint64_t done = 0;                                              // pairs coded so far
        // the records of a file from its carried tail on, read to its end (only to name both counts where they differ)
        auto count_rest = [&](FILE* f, Bytes& buf, bool& at_end) {
            uint64_t lines = 0;
            for (;;) {
                lines += (uint64_t)std::count(buf.p, buf.p + buf.n, (uint8_t)'\n');
                const bool open_line = buf.n && buf.p[buf.n - 1] != '\n';
                if (at_end) return (lines + open_line + 3) / 4;
                buf.n = 0;
                if (!fill(f, buf, (size_t)64 << 20, at_end)) croak("read error");
            }
        };
        auto unequal = [&](uint64_t na, uint64_t nb) {
            croak("-p: the files do not pair up: '%s' holds %llu records, '%s' holds %llu", usr.c_str(), (unsigned long long)na, o.pair.c_str(), (unsigned long long)nb);
        };
        for (;;) {
            auto want_of = [&](const Bytes& b) {
                size_t want = legacy ? std::max<size_t>(b.n * 2, 64u << 20) : slab / 2;
                return want <= b.n ? b.n * 2 : want;                    // a record longer than half a slab: grow
            };
            if (!eof && !fill(in, fq, want_of(fq), eof)) croak("read error");
            if (!eof2 && !fill(in2, fb, want_of(fb), eof2)) croak("read error");
            tick("read slab");
            if (eof && eof2 && fq.n == 0 && fb.n == 0) break;
            if (legacy && !(eof && eof2)) continue;                     // (one adaptive state cannot be cut: one slab holds both files)
            // whole records of each, then the same number of them
            size_t ua = fq.n, ub = fb.n;
            if (!eof) ua = whole_records(fq.p, fq.n, (uint64_t)std::count(fq.p, fq.p + fq.n, (uint8_t)'\n'));
            if (!eof2) ub = whole_records(fb.p, fb.n, (uint64_t)std::count(fb.p, fb.p + fb.n, (uint8_t)'\n'));
            const uint64_t la = count_lines(fq.p, ua), lb = count_lines(fb.p, ub);
            if (la & 3) croak("'%s': %llu lines at the end of the file, not a multiple of four", usr.c_str(), (unsigned long long)la);
            if (lb & 3) croak("'%s': %llu lines at the end of the file, not a multiple of four", o.pair.c_str(), (unsigned long long)lb);
            const uint64_t ra = la / 4, rb = lb / 4, r = std::min(ra, rb);
            if (eof && eof2 && ra != rb) unequal(done + ra, done + rb);
            if (!r) {
                if ((eof && !ra) || (eof2 && !rb)) unequal(done + count_rest(in, fq, eof), done + count_rest(in2, fb, eof2));
                continue;                                               // not one whole record of a file yet: read on
            }
            ua = drop_records(fq.p, ua, ra - r); ub = drop_records(fb.p, ub, rb - r);
            decide_tables(eof && eof2 ? ua + ub : (64ull << 20));
            const size_t bound = (size_t)sfq_encode_bound(ua + ub);
            if (!out.reserve(bound)) croak("out of memory");
            out.touch((ua + ub) / 3 + (1 << 20));
            sfq_result res;
            if (sfq_encode_pairs_host(ctx, fq.p, ua, fb.p, ub, &p, out.p, bound, &res)) {
                sfq_mate_report mr;                                     // -M: the report counts from the slab's first pair
                if (o.mates && sfq_get_mate_report(ctx, &mr) == 1 && mr.n_mismatch)
                    croak("-M: the files are out of step: pair %llu is \"%s\" in '%s' and \"%s\" in '%s' (%llu of the %llu pairs from pair %llu on differ)",
                          (unsigned long long)(done + mr.first_mismatch), mate_name(fq.p, ua, mr.first_off_a).c_str(), usr.c_str(),
                          mate_name(fb.p, ub, mr.first_off_b).c_str(), o.pair.c_str(), (unsigned long long)mr.n_mismatch,
                          (unsigned long long)mr.n_pairs, (unsigned long long)done);
                croak("%s", sfq_last_error(ctx));
            }
            tick("sfq_encode_pairs_host");
            qmap_changed += sfq_get_quality_map_changed(ctx);
            collect(ctx, res, ua + ub, idx, o.checksum, o.stats);
            for (int s = 0; s < SFQ_NSTREAMS; s++)
                streams[s].insert(streams[s].end(), out.p + res.stream_offset[s], out.p + res.stream_offset[s] + res.stream_bytes[s]);
            memmove(fq.p, fq.p + ua, fq.n - ua); fq.n -= ua;
            memmove(fb.p, fb.p + ub, fb.n - ub); fb.n -= ub;
            done += r;
        }
        fclose(in2);
        eof = true; fq.n = 0;                                           // nothing left for the loop below
    }
    for (;;) {
        if (eof && fq.n == 0) break;
        // the reference's single adaptive state (format 6) cannot be cut: one slab holds the whole file
        size_t want = legacy ? std::max<size_t>(fq.n * 2, 64u << 20) : slab;
        if (want <= fq.n) want = fq.n * 2;                              // a record longer than the slab: grow
        if (file_left != SIZE_MAX) want = legacy ? fq.n + file_left + 1 : std::min(want, fq.n + file_left + 1);   // +1: see the end of the file
        const size_t before = fq.n;
        if (!eof && !fill(in, fq, want, eof)) croak("read error");
        if (file_left != SIZE_MAX) file_left -= std::min(file_left, fq.n - before);
        tick("read slab");
        if (legacy && !eof) continue;
        size_t use = fq.n;
        if (!eof) { use = whole_records(fq.p, fq.n, (uint64_t)std::count(fq.p, fq.p + fq.n, (uint8_t)'\n')); if (use == 0) continue; }
        const uint8_t* text = fq.p;
        if (use == 0) break;
        decide_tables(eof ? use : (64ull << 20));                          // (a pipe: more than one slab of text is a big file)
        const size_t bound = (size_t)sfq_encode_bound(use);
        if (!out.reserve(bound)) croak("out of memory");
        out.touch(use / 3 + (1 << 20));                                    // the streams rarely exceed a third of the text
        sfq_result res;
        const int rc = sfq_encode_blocks_host(ctx, text, use, &p, out.p, bound, &res);
        if (rc) croak("%s", sfq_last_error(ctx));
        tick("sfq_encode_blocks_host");
        qmap_changed += sfq_get_quality_map_changed(ctx);
        collect(ctx, res, use, idx, o.checksum, o.stats);
        for (int s = 0; s < SFQ_NSTREAMS; s++)
            streams[s].insert(streams[s].end(), out.p + res.stream_offset[s], out.p + res.stream_offset[s] + res.stream_bytes[s]);
        memmove(fq.p, fq.p + use, fq.n - use); fq.n -= use;               // keep the partial record for the next slab
    }
    if (in != stdin) fclose(in);
    if (idx.segs.empty()) croak("fastq file: empty input");
    tick("collect streams");

    const std::string orig_name = usr.empty() ? "<< stdin >>" : usr;
    sfqc::Archive a;
    if (legacy) {                                                      // info keys in the reference's order (config.cpp:334-347, usrs.cpp:262-266, recs.cpp:71, gens.cpp:104, usrs.cpp:405)
        const sfq_block_info& b = idx.blocks[0];
        if (idx.first.size() >= 400) croak("first header too long for the reference's info page (recs.cpp:30)");
        a.set("whoami", "slimfastq");
        a.set("version", kInternalVersion);
        a.set("config.level", o.level);
        a.set("orig.filename", orig_name);
        if (!usr.empty()) a.set("orig.size", (long long)idx.raw);
        if (b.solid) a.set("usr.solid", 1);
        a.set("llen", b.llen);
        a.set("usr.2id", b.two_id);
        a.set("rec.first", std::string(idx.first.begin(), idx.first.end()));
        if (b.n_byte && b.n_byte != 'N') a.set("gen.N_byte", b.n_byte);
        a.set("num_records", (long long)idx.records);
        if (!o.quiet && b.extra_hi) a.set("qlt.extra.hi", b.extra_hi);
    } else a.info = idx.info(o.level, orig_name, frozen, false);
    if (paired) a.set("usr.pair", 1);                                  // R1 R2 R1 R2 ...: a decode with -p splits them again
    if (o.qmap) {                                                      // (the reference reads its info page into a map: keys it does not know are no harm)
        a.set("qlt.map", o.qmap_name);
        a.set("qlt.map.changed", (long long)qmap_changed);
    }
    if (streamed) {
        for (auto& s : idx.streams(frozen)) pw.append(pw.stream(s.first), s.second.data(), s.second.size());
        std::string werr;
        if (!pw.finish(a.info, werr)) croak("%s", werr.c_str());
        g_partial.clear();
        tick("finish archive");
        return;
    }
    for (int s = 0; s < SFQ_NSTREAMS; s++) if (!streams[s].empty()) a.add(sfq_stream_name(s), std::move(streams[s]));
    if (!legacy) for (auto& s : idx.streams(frozen)) a.add(s.first, std::move(s.second));
    else if (o.stats) a.add("txt.stat", sfqc::pack_text_stats(idx.stats));      // (a stream of its own: the reference's decoder does not look at it)
    std::string err;
    tick("build archive");
    if (!sfqc::write_file(fil, a, err)) croak("%s", err.c_str());
    tick("write file");
}

static void decode_file(sfq_ctx* ctx, const Opts& o, const std::string& usr, const std::string& fil) {
    std::string err;
    sfqc::Archive a;
    tick("start");
    if (!sfqc::read_file(fil, a, err)) croak("%s", err.c_str());
    tick("read archive");
    const int version = (int)a.get_long("version", 0);
    if (version > kBlockVersion) croak("%s was compressed with slimfastq version %d. My version is %d. Please upgrade me before decoing", fil.c_str(), version, kBlockVersion);
    const int level = clamp_level((int)a.get_long("config.level", 2));       // config.cpp:359
    if (o.demux && version < kBlockVersionMin)
        croak("-X: %s is a format-%d file (-B 0), which decodes on one lane and is not sorted by sample: write the archive in the block format", fil.c_str(), version);
    std::vector<sfq_block_info> blocks;
    std::vector<uint8_t> first;
    std::vector<sfqc::Segment> segs;
    std::vector<uint32_t> crcs;                                        // "blk.crc" (archives written with -K)
    const std::vector<uint8_t>* pri = a.find("qlt.pri");
    const std::vector<uint8_t>* chn = a.find("chn.idx");
    const std::vector<uint8_t>* rpr = a.find("rec.pri");
    const long long blk_tables = a.get_long("blk.tables", 0);
    if (blk_tables != 0 && blk_tables != 1) croak("%s: blk.tables = %lld is not a table mode this version knows. Please upgrade me before decoing", fil.c_str(), blk_tables);
    const bool frozen = blk_tables == 1;
    if (!frozen && chn) croak("archive holds a chain index (chn.idx) but does not say frozen tables (blk.tables)");
    const bool shared_prior = a.get_long("seg.shared_prior", 0) == 1;
    if (frozen && !chn) croak("archive says frozen tables but holds no chain index (chn.idx)");
    if (version >= kBlockVersionMin) {
        const std::vector<uint8_t>* idx = a.find("blk.idx");
        if (!idx || !sfqc::unpack_block_index(*idx, blocks, version >= 8 ? SFQ_NSTREAMS : 10)) croak("bad block index");
        if (const std::vector<uint8_t>* h = a.find("blk.hdr")) first = *h;
        if (const std::vector<uint8_t>* si = a.find("seg.idx")) {
            if (!sfqc::unpack_segment_index(*si, segs, frozen) || segs.size() > blocks.size()) croak("bad segment index");
        } else segs.push_back(sfqc::Segment{blocks.size(), pri ? pri->size() : 0, (uint64_t)a.get_long("orig.size", 0), chn ? chn->size() : 0, rpr ? rpr->size() : 0});
        if (blocks.empty()) croak("bad block index (no blocks)");
        if (const std::vector<uint8_t>* c = a.find("blk.crc")) {
            if (!sfqc::unpack_block_checksums(*c, blocks.size(), crcs)) croak("bad block checksums (blk.crc: %zu bytes for %zu blocks)", c->size(), blocks.size());
        }
    } else {
        sfq_block_info b; memset(&b, 0, sizeof b);
        b.n_records = (uint32_t)a.get_long("num_records");
        if (!b.n_records) croak("Zero records, what's going on?");
        b.llen = (uint32_t)a.get_long("llen");
        b.solid = a.get_long("usr.solid") != 0; b.two_id = a.get_long("usr.2id") != 0;
        b.n_byte = (uint8_t)a.get_long("gen.N_byte", 0);
        b.gen_bits = (uint8_t)level_gen_bits(level);
        std::string f = a.get("rec.first");
        first.assign(f.begin(), f.end());
        b.first_hdr_len = (uint32_t)first.size();
        if (a.get_long("num_records") > 0xFFFFFFFFll) croak("archive too large for the single-block GPU path (more than 2^32 - 1 records)");
        for (int s = 0; s < SFQ_NSTREAMS; s++) if (auto* v = a.find(sfq_stream_name(s))) {
            if (v->size() > 0xFFFFFFFFull) croak("archive too large for the single-block GPU path (stream %s has %zu bytes)", sfq_stream_name(s), v->size());
            b.size[s] = v->size();
        }
        blocks.push_back(b);
        segs.push_back(sfqc::Segment{1, 0, (uint64_t)a.get_long("orig.size", 0), 0, 0});
    }
    // -R: records [r_lo, r_hi) of the archive
    uint64_t r_lo = 0, r_hi = 0;
    if (o.range) {
        const uint64_t total = blocks.back().first_record + blocks.back().n_records;
        if (o.r_first >= total) croak("-R %llu:%llu: the archive holds %llu records", (unsigned long long)o.r_first, (unsigned long long)o.r_count, (unsigned long long)total);
        r_lo = o.r_first; r_hi = o.r_count > total - r_lo ? total : r_lo + o.r_count;
    }
    // -W: pairs [w_first, w_first + w_count) are records [r_lo, r_hi) too; what -R does per segment holds with pairs for records
    const bool ranged = o.range || o.window;
    if (o.window) {
        const uint64_t total = (blocks.back().first_record + blocks.back().n_records) / 2;
        if (o.w_first >= total) croak("-W %llu:%llu: the archive holds %llu pairs", (unsigned long long)o.w_first, (unsigned long long)o.w_count, (unsigned long long)total);
        r_lo = 2 * o.w_first; r_hi = o.w_count > total - o.w_first ? 2 * total : r_lo + 2 * o.w_count;
    }
    const bool paired = !o.pair.empty();
    // -k: an archive written from paired files keeps or drops whole pairs, split (-p, -W) or not
    const bool sel_pairs = o.select && a.get_long("usr.pair", 0) == 1;
    if (o.select && o.sel_either && !sel_pairs) croak("-k either: %s was not written from paired files (no usr.pair in its info): its records stand alone", fil.c_str());
    if (paired && a.get_long("usr.pair", 0) != 1) croak("-p: %s was not written from paired files (no usr.pair in its info): decode it without -p", fil.c_str());
    // -o: pairs are the archive's, and no pair lies across two segments (-W's rule, found here before an output file is opened)
    if (o.ovl) {
        size_t at = 0;
        for (const sfqc::Segment& g : segs) {
            if (g.nblocks == 0 || g.nblocks > blocks.size() - at) croak("bad segment index");
            const uint64_t seg0 = blocks[at].first_record, seg_end = blocks[at + g.nblocks - 1].first_record + blocks[at + g.nblocks - 1].n_records;
            if ((seg0 | seg_end) & 1) croak("-o: segment %zu holds records %llu..%llu, not whole pairs: %s was not written by -p",
                                            (size_t)(&g - segs.data()), (unsigned long long)seg0, (unsigned long long)seg_end, fil.c_str());
            at += g.nblocks;
        }
    }
    FILE* of = stdout;
    FILE* of2 = nullptr;
    FILE* of3 = nullptr;                                                // -o merge=PATH: the merged records of every segment
    const bool merging = o.ovl && !o.ovl_merge.empty();
    if (merging) {
        if (!o.overwrite && access(o.ovl_merge.c_str(), F_OK) == 0) { fprintf(stderr, "Can't write file '%s': File exists\n", o.ovl_merge.c_str()); exit(1); }
        if (!o.overwrite && !usr.empty() && access(usr.c_str(), F_OK) == 0) { fprintf(stderr, "Can't write file '%s': File exists\n", usr.c_str()); exit(1); }
        if (!o.overwrite && paired && access(o.pair.c_str(), F_OK) == 0) { fprintf(stderr, "Can't write file '%s': File exists\n", o.pair.c_str()); exit(1); }
        of3 = fopen(o.ovl_merge.c_str(), "wb");
        if (!of3) { fprintf(stderr, "Can't write file '%s'\n", o.ovl_merge.c_str()); exit(1); }
    }
    if (paired) {
        if (!o.overwrite && access(o.pair.c_str(), F_OK) == 0) { fprintf(stderr, "Can't write file '%s': File exists\n", o.pair.c_str()); exit(1); }
        if (!o.overwrite && access(usr.c_str(), F_OK) == 0) { fprintf(stderr, "Can't write file '%s': File exists\n", usr.c_str()); exit(1); }
        of2 = fopen(o.pair.c_str(), "wb");
        if (!of2) { fprintf(stderr, "Can't write file '%s'\n", o.pair.c_str()); exit(1); }
    }
    if (!usr.empty()) {
        if (!o.overwrite && access(usr.c_str(), F_OK) == 0) {
            if (g_batch) croak("Can't write file '%s': File exists", usr.c_str());
            fprintf(stderr, "Can't write file '%s': File exists\n", usr.c_str()); exit(1);
        }
        of = fopen(usr.c_str(), "wb");
        if (!of) {
            if (g_batch) croak("Can't write file '%s'", usr.c_str());
            fprintf(stderr, "Can't write file '%s'\n", usr.c_str()); exit(1);
        }
    }
    sfq_params p; memset(&p, 0, sizeof p);
    p.level = level; p.version = version >= kBlockVersionMin ? kInternalVersion : (uint32_t)version;
    // (a -b worker keeps its context from job to job: a -K encode before this job left the pass on; installed checksums run it)
    if (sfq_ctx_set_checksums(ctx, 0)) croak("%s", sfq_last_error(ctx));
    if (sfq_ctx_set_pair_split(ctx, paired && !o.demux ? 1 : 0)) croak("%s", sfq_last_error(ctx));      // (-X splits every sample's mates itself)
    // -X: a file a part, opened now and appended to segment by segment; the unassigned units go to -u (and -p)
    const bool dmx_pairs = o.demux && (paired || a.get_long("usr.pair", 0) == 1);
    std::vector<FILE*> dmx_files;
    std::vector<uint64_t> dmx_units(o.demux_names.size() + 1, 0), dmx_off, dmx_got;
    sfq_demux_report dmx_sum; memset(&dmx_sum, 0, sizeof dmx_sum);
    if (sfq_ctx_set_demux(ctx, nullptr, nullptr)) croak("%s", sfq_last_error(ctx));
    if (o.demux) {
        for (const std::string& nm : o.demux_names)
            for (int g = 0; g < (paired ? 2 : 1); g++) {
                const std::string f = o.demux_out + nm + (paired ? (g ? "_R2" : "_R1") : "") + (o.bgzf ? ".fastq.gz" : ".fastq");
                FILE* h = fopen(f.c_str(), "wb");
                if (!h) croak("-X: can't write file '%s'", f.c_str());
                dmx_files.push_back(h);
            }
        dmx_files.push_back(of);
        if (paired) dmx_files.push_back(of2);
        dmx_off.resize(dmx_files.size() + 1); dmx_got.resize(dmx_files.size() + 1);
    }
    if (sfq_ctx_set_pick(ctx, o.pick)) croak("%s", sfq_last_error(ctx));
    if (sfq_ctx_set_bgzf(ctx, o.bgzf ? 1 : 0)) croak("%s", sfq_last_error(ctx));
    sfq_bgzf_report bgz_sum; memset(&bgz_sum, 0, sizeof bgz_sum);
    if (sfq_ctx_set_select(ctx, nullptr)) croak("%s", sfq_last_error(ctx));       // (set per segment: the range and the index base are the segment's)
    uint64_t sel_kept = 0, sel_seen = 0, sel_bytes = 0, sel_text = 0;
    if (sfq_ctx_set_trim(ctx, o.trim ? &o.trim_rule : nullptr)) croak("-c: %s", sfq_last_error(ctx));
    uint64_t trim_recs = 0, trim_changed = 0, trim_emptied = 0, trim_in = 0, trim_out = 0;
    if (sfq_ctx_set_overlap(ctx, nullptr)) croak("%s", sfq_last_error(ctx));      // (set per segment: the range is the segment's)
    sfq_overlap_report ovl_sum; memset(&ovl_sum, 0, sizeof ovl_sum);
    if (sfq_ctx_set_merge(ctx, nullptr)) croak("%s", sfq_last_error(ctx));
    uint64_t mrg_merged = 0, mrg_bases = 0;                             // (the rest of a merge's report is summed in ovl_sum)
    // -D: one set for the whole run, so that duplicates are found across segments.  Keys: the archive's records (the range's; pairs:
    // half); key bytes: the segments' text, a bound that is loose by about 2x (a key is the base line of a record of four lines)
    const bool dd_pairs = o.dedup && (paired || o.window || merging || a.get_long("usr.pair", 0) == 1);      // (merge= wants pairs behind it)
    uint64_t dd_units = 0, dd_kept = 0;
    if (sfq_ctx_set_dedup(ctx, nullptr) || sfq_dedup_set_destroy(ctx)) croak("%s", sfq_last_error(ctx));       // (set per segment: the range is the segment's)
    if (o.dedup) {
        uint64_t keys = ranged ? r_hi - r_lo : blocks.back().first_record + blocks.back().n_records, bytes = 0;
        if (dd_pairs) keys = (keys + 1) / 2;
        size_t at = 0;
        for (const sfqc::Segment& g : segs) {
            if (g.nblocks == 0 || g.nblocks > blocks.size() - at) croak("bad segment index");
            uint64_t coded = 0;                                         // (a segment without raw_bytes: the size its decode reserves)
            for (size_t b = at; b < at + g.nblocks; b++) for (int s = 0; s < SFQ_NSTREAMS; s++) coded += blocks[b].size[s];
            bytes += g.raw_bytes ? g.raw_bytes : coded * 8 + (1 << 20);
            at += g.nblocks;
        }
        if (sfq_dedup_set_create(ctx, std::max<uint64_t>(keys, 1), std::max<uint64_t>(bytes, 1), dd_pairs ? 1 : 0)) croak("-D: %s", sfq_last_error(ctx));
        tick("sfq_dedup_set_create");
    }
    // -G: one set of k-mers for the whole run: at most one k-mer a byte of the flattened references.  Records are pairs where -D's are.
    const bool scr_pairs = o.screen && (paired || o.window || merging || a.get_long("usr.pair", 0) == 1);
    uint64_t scr_units = 0, scr_kept = 0, scr_kmers = 0;
    if (sfq_ctx_set_screen(ctx, nullptr) || sfq_screen_set_destroy(ctx)) croak("%s", sfq_last_error(ctx));     // (set per segment: the range is the segment's)
    if (o.screen) {
        if (o.screen_rule.pairs == 2 && !scr_pairs) croak("-G both: the records of %s stand alone: it was not written from paired files, and neither -p nor -W is given", fil.c_str());
        uint64_t total = 0;
        for (const auto& q : o.screen_seqs) total += q.size();
        if (sfq_screen_set_create(ctx, o.screen_k, std::max<uint64_t>(total, 1))) croak("-G: %s", sfq_last_error(ctx));
        for (const auto& q : o.screen_seqs) if (sfq_screen_set_add(ctx, q.data(), q.size())) croak("-G: %s", sfq_last_error(ctx));
        if (sfq_screen_set_info(ctx, nullptr, &scr_kmers, nullptr) != 1) croak("-G: the library holds no set");
        tick("sfq_screen_set_add");
    }
    const uint64_t rec_lines = !o.pick ? 4 : o.pick == SFQ_PICK_FASTA ? 2 : 1;      // the lines of a record in what a call hands back
    // walk the segments: each one's blocks, its slice of every stream (streams are segment-major), its prior
    size_t b0 = 0, pri_off = 0, chn_off = 0, rpr_off = 0;
    uint64_t spos[SFQ_NSTREAMS] = {0};
    std::vector<uint8_t> data;
    Bytes out;
    // several segments of known size: the text of one is written (a thread) while the next is decoded, out of two
    // page-locked buffers (kept for the life of the process, like the encoder's)
    static uint8_t* opin[2] = { nullptr, nullptr }; static size_t opin_cap = 0;
    size_t max_raw = 0; bool sized = segs.size() > 1 && !ranged;
    for (const sfqc::Segment& g : segs) { max_raw = std::max<size_t>(max_raw, (size_t)g.raw_bytes); if (!g.raw_bytes) sized = false; }
    if (sized && opin_cap < max_raw + 64) {
        for (auto& q : opin) { if (q) sfq_host_free(ctx, q); q = nullptr; }
        opin[0] = (uint8_t*)sfq_host_alloc(ctx, max_raw + 64); opin[1] = (uint8_t*)sfq_host_alloc(ctx, max_raw + 64);
        opin_cap = (opin[0] && opin[1]) ? max_raw + 64 : 0;
        if (!opin_cap) sized = false;
        tick("pinned buffers");
    }
    std::atomic<int> wbad{0}; int ob = 0;
    Joiner writer;                                                      // (declared after what its thread uses: joined first when the scope unwinds)
    for (const sfqc::Segment& g : segs) {
        if (g.nblocks == 0 || g.nblocks > blocks.size() - b0) croak("bad segment index");
        if (pri ? g.prior_bytes > pri->size() - pri_off : g.prior_bytes != 0) croak("bad segment index");
        if (chn ? g.chain_bytes > chn->size() - chn_off : g.chain_bytes != 0) croak("bad segment index");
        if (rpr ? g.recpri_bytes > rpr->size() - rpr_off : g.recpri_bytes != 0) croak("bad segment index");
        std::vector<sfq_block_info> sb(blocks.begin() + (ptrdiff_t)b0, blocks.begin() + (ptrdiff_t)(b0 + g.nblocks));
        const uint64_t rec0 = sb[0].first_record, h0 = sb[0].first_hdr_off;
        uint64_t need[SFQ_NSTREAMS] = {0}, hbytes = 0;
        for (auto& b : sb) { b.first_record -= rec0; b.first_hdr_off -= h0; hbytes += b.first_hdr_len; for (int s = 0; s < SFQ_NSTREAMS; s++) need[s] += b.size[s]; }
        if (h0 + hbytes > first.size()) croak("bad block index (first headers)");
        // -R: the segment's blocks that hold records of the range; a segment without any is passed over (its priors still count for a
        // later segment that shares them)
        uint32_t w0 = 0, wn = (uint32_t)sb.size();
        bool touched = true;
        uint64_t wp0 = 0, wpn = 0;                                      // -W: the segment's pairs of the window, counted from its first
        if (ranged) {
            const uint64_t seg_end = rec0 + sb.back().first_record + sb.back().n_records, br = sb[0].n_records;
            // (a -p encode takes the same number of records from both files per slab: a segment holds whole pairs)
            if (o.window && ((rec0 | seg_end) & 1)) croak("-W: segment %zu holds records %llu..%llu, not whole pairs: %s was not written by -p",
                                                          (size_t)(&g - segs.data()), (unsigned long long)rec0, (unsigned long long)seg_end, fil.c_str());
            touched = r_lo < seg_end && r_hi > rec0 && br;
            if (touched) {
                const uint64_t lo = std::max(r_lo, rec0) - rec0, hi = std::min(r_hi, seg_end) - rec0;
                w0 = (uint32_t)(lo / br); wn = (uint32_t)((hi - 1) / br) - w0 + 1;
                wp0 = lo / 2; wpn = (hi - lo) / 2;
                if (o.window && sfq_pair_window_blocks(sb.data(), (uint32_t)sb.size(), wp0, wpn, &w0, &wn)) croak("bad block index (a segment's records)");
            }
        }
        if (!touched) for (int s = 0; s < SFQ_NSTREAMS; s++) spos[s] += need[s];
        data.clear();
        uint64_t soff[SFQ_NSTREAMS];
        for (int s = 0; touched && s < SFQ_NSTREAMS; s++) {
            soff[s] = data.size();
            if (!need[s]) continue;
            const std::vector<uint8_t>* v = a.find(sfq_stream_name(s));
            if (!v || spos[s] + need[s] > v->size()) croak("stream %s is shorter than its block index says", sfq_stream_name(s));
            data.insert(data.end(), v->begin() + (ptrdiff_t)spos[s], v->begin() + (ptrdiff_t)(spos[s] + need[s]));
            spos[s] += need[s];
        }
        // (seg.shared_prior: a segment without priors of its own codes from the previous segment's, e.g. the ranks of a multi-GPU job)
        if (g.prior_bytes) { if (sfq_set_qlt_prior(ctx, pri->data() + pri_off, g.prior_bytes)) croak("%s", sfq_last_error(ctx)); }
        else if (!shared_prior) sfq_set_qlt_prior(ctx, nullptr, 0);
        if (sfq_set_chain_index(ctx, g.chain_bytes ? chn->data() + chn_off : nullptr, g.chain_bytes)) croak("%s", sfq_last_error(ctx));
        if (g.recpri_bytes) { if (sfq_set_rec_prior(ctx, rpr->data() + rpr_off, g.recpri_bytes)) croak("%s", sfq_last_error(ctx)); }
        else if (!shared_prior) sfq_set_rec_prior(ctx, nullptr, 0);
        if (!touched) { b0 += g.nblocks; pri_off += g.prior_bytes; chn_off += g.chain_bytes; rpr_off += g.recpri_bytes; continue; }
        uint64_t cap = g.raw_bytes, got = 0;
        if (!cap) cap = data.size() * 8 + (1 << 20);
        // (a window: its share of the segment's text and as much again; the call reports what it needs where that is too little --
        //  or, where the window's lines alone outgrow it, a damaged stream: then the segment's size is tried)
        const uint64_t cap_seg = cap;
        if (ranged && wn < sb.size()) cap = std::min<uint64_t>(cap_seg, cap_seg / sb.size() * wn * 2 + (1 << 20));
        if (o.select) {
            // the range: the segment's share of -R, counted from the decoded text's first record (-W: the library cuts to the window's
            // pairs itself); index_base: that record's number in the archive, so that a sample does not depend on segments or windows
            sfq_select sel = o.sel;
            const uint64_t text0 = rec0 + sb[w0].first_record;
            sel.pairs = sel_pairs ? (o.sel_either ? SFQ_SELECT_EITHER : SFQ_SELECT_BOTH) : 0;
            sel.index_base = text0;
            if (o.range) {
                uint64_t wrecs = 0;
                for (uint32_t b = w0; b < w0 + wn; b++) wrecs += sb[b].n_records;
                const uint64_t lo = std::max(r_lo, text0), hi = std::min(r_hi, text0 + wrecs);
                sel.first_record = lo - text0; sel.n_records = hi - lo;
            }
            if (sel.pairs && (text0 & 1)) croak("-k: the blocks of %s hold odd numbers of records, so that a decoded text begins at a second mate (record %llu): "
                                                "pairs are selected from archives written with an even -B", fil.c_str(), (unsigned long long)text0);
            if (sfq_ctx_set_select(ctx, &sel))
                croak("-k: %s%s", sfq_last_error(ctx), sel.pairs ? " (an archive written with -p is selected pair by pair: a range begins at a first mate)" : "");
        }
        if (o.ovl) {
            // the range: from the decoded text's first record whose archive number is even, whole pairs (-W: the library's own)
            sfq_overlap rule = o.ovl_rule;
            if (!o.window) {
                uint64_t wrecs = 0;
                for (uint32_t b = w0; b < w0 + wn; b++) wrecs += sb[b].n_records;
                rule.first_record = (rec0 + sb[w0].first_record) & 1;
                rule.n_records = (wrecs - rule.first_record) & ~1ull;
            }
            if (merging) {
                // records outside a merge's range are dropped: under -R the range is the segment's share of -R itself (whole pairs), and
                // behind -k, -G or -D the text that they kept (each has cut to the range already)
                if (o.select || o.dedup || o.screen) { rule.first_record = 0; rule.n_records = ~0ull; }
                else if (o.range) {
                    uint64_t wrecs = 0;
                    for (uint32_t b = w0; b < w0 + wn; b++) wrecs += sb[b].n_records;
                    const uint64_t text0 = rec0 + sb[w0].first_record, lo = std::max(r_lo, text0), hi = std::min(r_hi, text0 + wrecs);
                    rule.first_record = lo - text0; rule.n_records = hi - lo;
                }
                const sfq_merge m{ rule.first_record, rule.n_records, rule.min_overlap, rule.max_mm, rule.max_mm_pct, 33 };
                if (!o.window && !m.n_records) { if (sfq_ctx_set_merge(ctx, nullptr)) croak("%s", sfq_last_error(ctx)); }
                else if (sfq_ctx_set_merge(ctx, &m)) croak("-o: %s", sfq_last_error(ctx));
            }
            else if (!o.window && !rule.n_records) { if (sfq_ctx_set_overlap(ctx, nullptr)) croak("%s", sfq_last_error(ctx)); }
            else if (sfq_ctx_set_overlap(ctx, &rule)) croak("-o: %s", sfq_last_error(ctx));
        }
        if (o.screen) {
            // the range: the segment's share of -R, as -k's (behind -k the text that -k kept; -W: the library cuts to the window's pairs itself)
            sfq_screen rule = o.screen_rule;
            rule.pairs = !scr_pairs ? 0u : rule.pairs == 2 ? 2u : 1u;
            const uint64_t text0 = rec0 + sb[w0].first_record;
            if (o.range && !o.select) {
                uint64_t wrecs = 0;
                for (uint32_t b = w0; b < w0 + wn; b++) wrecs += sb[b].n_records;
                const uint64_t lo = std::max(r_lo, text0), hi = std::min(r_hi, text0 + wrecs);
                rule.first_record = lo - text0; rule.n_records = hi - lo;
            }
            if (scr_pairs && !o.window && !o.select) {
                if (text0 & 1) croak("-G: the blocks of %s hold odd numbers of records, so that a decoded text begins at a second mate (record %llu): "
                                     "pairs are screened in archives written with an even -B", fil.c_str(), (unsigned long long)text0);
                if (rule.first_record & 1) croak("-G: -R begins at record %llu, a second mate: the reads of an archive written from paired files are screened "
                                                 "as pairs, and a range begins at a first mate (-W F:N names pairs)", (unsigned long long)(text0 + rule.first_record));
            }
            if (sfq_ctx_set_screen(ctx, &rule)) croak("-G: %s", sfq_last_error(ctx));
        }
        if (o.dedup) {
            // the range: the segment's share of -R, as -k's (behind -k or -G the text that they kept; -W: the library cuts to the window's pairs itself)
            sfq_dedup rule{ 0, ~0ull, dd_pairs ? 1u : 0u, 1u };
            const uint64_t text0 = rec0 + sb[w0].first_record;
            if (o.range && !o.select && !o.screen) {
                uint64_t wrecs = 0;
                for (uint32_t b = w0; b < w0 + wn; b++) wrecs += sb[b].n_records;
                const uint64_t lo = std::max(r_lo, text0), hi = std::min(r_hi, text0 + wrecs);
                rule.first_record = lo - text0; rule.n_records = hi - lo;
            }
            if (dd_pairs && !o.window && !o.select && !o.screen) {
                if (text0 & 1) croak("-D: the blocks of %s hold odd numbers of records, so that a decoded text begins at a second mate (record %llu): "
                                     "duplicates of pairs are dropped from archives written with an even -B", fil.c_str(), (unsigned long long)text0);
                if (rule.first_record & 1) croak("-D: -R begins at record %llu, a second mate: duplicates of an archive written from paired files are pairs, "
                                                 "and a range begins at a first mate (-W F:N names pairs)", (unsigned long long)(text0 + rule.first_record));
            }
            if (sfq_ctx_set_dedup(ctx, &rule)) croak("-D: %s", sfq_last_error(ctx));
        }
        if (o.demux) {
            // the range: the segment's share of -R, as -D's (behind -k, -G or -D the text that they kept)
            sfq_demux rule = o.demux_rule;
            rule.pairs = dmx_pairs ? 1 : 0; rule.split_mates = paired ? 1 : 0;
            const uint64_t text0 = rec0 + sb[w0].first_record;
            if (o.range && !o.select && !o.screen && !o.dedup) {
                uint64_t wrecs = 0;
                for (uint32_t b = w0; b < w0 + wn; b++) wrecs += sb[b].n_records;
                const uint64_t lo = std::max(r_lo, text0), hi = std::min(r_hi, text0 + wrecs);
                rule.first_record = lo - text0; rule.n_records = hi - lo;
            }
            if (dmx_pairs && !o.select && !o.screen && !o.dedup) {
                if (text0 & 1) croak("-X: the blocks of %s hold odd numbers of records, so that a decoded text begins at a second mate (record %llu): "
                                     "pairs are sorted by sample in archives written with an even -B", fil.c_str(), (unsigned long long)text0);
                if (rule.first_record & 1) croak("-X: -R begins at record %llu, a second mate: the units of an archive written from paired files are pairs, "
                                                 "and a range begins at a first mate", (unsigned long long)(text0 + rule.first_record));
            }
            if (sfq_ctx_set_demux(ctx, &rule, o.demux_codes.data())) croak("-X: %s", sfq_last_error(ctx));
        }
        sfq_result res;
        int rc = 0;
        uint8_t* dst = nullptr;
        uint64_t wsplit = 0;
        for (int attempt = 0; attempt < (ranged ? 3 : 2); attempt++) {
            if (sized && cap + 16 <= opin_cap) dst = opin[ob];
            else {
                if (!out.reserve((size_t)cap + 16)) croak("out of memory");
                out.touch((size_t)cap);
                dst = out.p;
            }
            // (the expected checksums are consumed by the call they are installed for)
            if (!crcs.empty() && sfq_set_block_checksums(ctx, crcs.data() + b0 + w0, wn)) croak("%s", sfq_last_error(ctx));
            if (o.window) rc = sfq_decode_pair_range_host(ctx, &p, sb.data(), (uint32_t)sb.size(), first.data() + h0, hbytes,
                                                          data.data(), data.size(), soff, wp0, wpn, dst, cap, &got, &wsplit, &res);
            else if (o.range) rc = sfq_decode_block_range_host(ctx, &p, sb.data(), (uint32_t)sb.size(), first.data() + h0, hbytes,
                                                          data.data(), data.size(), soff, w0, wn, dst, cap, &got, &res);
            else
            rc = sfq_decode_blocks_host(ctx, &p, sb.data(), (uint32_t)sb.size(), first.data() + h0, hbytes,
                                        data.data(), data.size(), soff, dst, cap, &got, &res);
            if (ranged && rc == SFQ_E_CORRUPT && cap < cap_seg) { cap = cap_seg; continue; }
            if (rc != SFQ_E_OVERFLOW || got <= cap) break;
            cap = got;                                                 // the call reports the size it needs
        }
        if (rc && segs.size() > 1)                                     // (the library numbers the blocks of its call: one segment)
            croak("segment %zu of %zu (archive blocks %zu..%zu): %s", (size_t)(&g - segs.data()), segs.size(), b0, b0 + (size_t)g.nblocks - 1,
                  sfq_last_error(ctx));
        if (rc) croak("%s", sfq_last_error(ctx));
        tick("sfq_decode_blocks_host");
        const bool in_out = dst == out.p;                              // (not a page-locked buffer: written before the next segment reuses it)
        if (o.bgzf) {
            sfq_bgzf_report rep;
            const int did = sfq_get_bgzf(ctx, &rep, nullptr, nullptr, 0);      // (0: the passes in front left nothing)
            if (did < 0) croak("-Z: the library did not deflate");
            if (did == 1) { bgz_sum.text_bytes += rep.text_bytes; bgz_sum.out_bytes += rep.out_bytes; bgz_sum.members += rep.members; bgz_sum.stored_members += rep.stored_members; }
        }
        if (o.select) {
            sfq_select_report rep;
            if (sfq_get_select(ctx, &rep) != 1) croak("-k: the library did not select");
            sel_kept += rep.n_kept; sel_seen += rep.n_in_range; sel_bytes += rep.kept_bytes; sel_text += rep.text_bytes;
        }
        if (o.screen) {
            sfq_screen_report rep;
            const int did = sfq_get_screen(ctx, &rep);                 // (0: a selection in front kept nothing)
            if (did < 0) croak("-G: the library did not screen");
            if (did == 1) { scr_units += rep.n_units; scr_kept += rep.n_kept; }
        }
        if (o.dedup) {
            sfq_dedup_report rep;
            const int did = sfq_get_dedup(ctx, &rep);                  // (0: a selection in front kept nothing)
            if (did < 0) croak("-D: the library did not look for duplicates");
            if (did == 1) { dd_units += rep.n_units; dd_kept += rep.n_kept; }
        }
        if (o.trim) {
            sfq_trim_report rep;
            if (sfq_get_trim(ctx, &rep) != 1) croak("-c: the library did not trim");
            trim_recs += rep.n_records; trim_changed += rep.n_changed; trim_emptied += rep.n_emptied; trim_in += rep.bases_in; trim_out += rep.bases_out;
        }
        uint64_t mbytes = 0;                                           // -o merge=: the call handed back the merged records first
        if (merging) {
            static sfq_merge_report rep;
            const int did = sfq_get_merge(ctx, &rep, &mbytes);
            if (did < 0) croak("-o: the library did not merge the pairs");
            if (did == 1) {
                ovl_sum.n_pairs += rep.n_pairs; ovl_sum.n_skipped += rep.n_skipped; mrg_merged += rep.n_merged; mrg_bases += rep.bases_merged;
                for (size_t i = 0; i <= 2 * SFQ_OVERLAP_MAX_LEN; i++) ovl_sum.insert_hist[i] += rep.insert_hist[i];
            }
        } else if (o.ovl) {
            sfq_overlap_report rep;
            const int did = sfq_get_overlap(ctx, &rep);
            if (did < 0) croak("-o: the library did not search the pairs");
            if (did == 1) {
                ovl_sum.n_pairs += rep.n_pairs; ovl_sum.n_skipped += rep.n_skipped; ovl_sum.n_overlap += rep.n_overlap; ovl_sum.n_cut += rep.n_cut;
                ovl_sum.bases_in += rep.bases_in; ovl_sum.bases_out += rep.bases_out; ovl_sum.mismatches += rep.mismatches;
                for (size_t i = 0; i <= 2 * SFQ_OVERLAP_MAX_LEN; i++) ovl_sum.insert_hist[i] += rep.insert_hist[i];
            }
        }
        if (o.demux) {                                                 // the parts, one behind the other: each to its file
            sfq_demux_report rep;
            const int had = sfq_get_demux(ctx, &rep, dmx_off.data(), dmx_got.data(), dmx_off.size());       // (0: a pass in front left nothing)
            if (had < 0) croak("-X: the library did not sort the records");
            writer.join();
            if (wbad) croak("USR: Error writing output");
            if (had == 1) {
                for (size_t c = 0; c < dmx_files.size(); c++)
                    if (fwrite(dst + dmx_off[c], 1, (size_t)(dmx_off[c + 1] - dmx_off[c]), dmx_files[c]) != dmx_off[c + 1] - dmx_off[c]) croak("USR: Error writing output");
                for (size_t i = 0; i < dmx_units.size(); i++) dmx_units[i] += dmx_got[i];
                dmx_sum.n_units += rep.n_units; dmx_sum.n_assigned += rep.n_assigned; dmx_sum.n_perfect += rep.n_perfect; dmx_sum.n_short += rep.n_short;
                dmx_sum.n_far += rep.n_far; dmx_sum.n_ambiguous += rep.n_ambiguous; dmx_sum.bases_clipped += rep.bases_clipped;
            }
            tick("write output");
            b0 += g.nblocks; pri_off += g.prior_bytes; chn_off += g.chain_bytes; rpr_off += g.recpri_bytes;
            continue;
        }
        if (o.range && !o.select && !merging && !o.dedup && !o.screen) {                        // the window's first and last block, cut to records: rec_lines lines each
            const uint64_t wrec0 = rec0 + (uint64_t)w0 * sb[0].n_records;
            const uint64_t lo = std::max(r_lo, wrec0), hi = std::min(r_hi, wrec0 + res.n_records);
            const size_t from = records_end(dst, (size_t)got, lo - wrec0, rec_lines);
            const size_t to = from + records_end(dst + from, (size_t)got - from, hi - lo, rec_lines);
            dst += from; got = to - from;
        }
        // -p: the call handed back the first mates, then (from `first` on) the second mates
        uint64_t first = got;
        if (paired && got && sfq_get_pair_split(ctx, &first, nullptr) != 1) croak("-p: the library did not split the text");
        if (first < mbytes) first = got;                               // (nothing was split: no rest, or nothing kept)
        auto write_out = [dst, got, first, mbytes, of, of2, of3]() {
            return (!mbytes || fwrite(dst, 1, (size_t)mbytes, of3) == mbytes) && fwrite(dst + mbytes, 1, (size_t)(first - mbytes), of) == first - mbytes &&
                   (got == first || fwrite(dst + first, 1, (size_t)(got - first), of2) == got - first);
        };
        writer.join();
        if (wbad) croak("USR: Error writing output");
        if (in_out) { if (!write_out()) croak("USR: Error writing output"); }
        else {
            writer.start([write_out, &wbad]() { if (!write_out()) wbad = 1; });
            ob ^= 1;
        }
        tick("write output");
        b0 += g.nblocks; pri_off += g.prior_bytes; chn_off += g.chain_bytes; rpr_off += g.recpri_bytes;
    }
    writer.join();
    if (wbad) croak("USR: Error writing output");
    if (o.bgzf) {                                                      // every file ends with the end-of-file block, once
        uint8_t eof[28];
        sfq_bgzf_eof(eof);
        std::vector<FILE*> all(dmx_files.begin(), dmx_files.end());
        if (!o.demux) { all.push_back(of); if (of2) all.push_back(of2); }
        if (of3) all.push_back(of3);
        for (FILE* f : all) if (fwrite(eof, 1, 28, f) != 28) croak("USR: Error writing output");
        if (sfq_ctx_set_bgzf(ctx, 0)) croak("%s", sfq_last_error(ctx));
    }
    if (o.demux) {
        if (sfq_ctx_set_demux(ctx, nullptr, nullptr)) croak("%s", sfq_last_error(ctx));
        for (size_t c = 0; c < o.demux_names.size() * (paired ? 2 : 1); c++) if (fclose(dmx_files[c])) croak("-X: error writing a sample's file");
        if (!o.demux_counts.empty()) {
            FILE* cf = fopen(o.demux_counts.c_str(), "w");
            if (!cf) croak("-X counts=%s: can't write the file", o.demux_counts.c_str());
            const size_t B = o.demux_rule.part[0].len + o.demux_rule.part[1].len, l0 = o.demux_rule.part[0].len;
            for (size_t s = 0; s < o.demux_names.size(); s++) {
                const std::string code((const char*)o.demux_codes.data() + s * B, B);
                fprintf(cf, "%s\t%s%s%s\t%llu\n", o.demux_names[s].c_str(), code.substr(0, l0).c_str(), B > l0 ? "+" : "", code.substr(l0).c_str(), (unsigned long long)dmx_units[s]);
            }
            fprintf(cf, "unassigned\t\t%llu\n", (unsigned long long)dmx_units.back());
            if (fclose(cf)) croak("-X counts=%s: error writing the file", o.demux_counts.c_str());
        }
        if (!o.quiet)
            fprintf(stderr, "demultiplexed %llu %s: %llu assigned (%llu perfect), %llu short, %llu far, %llu ambiguous\n", (unsigned long long)dmx_sum.n_units,
                    dmx_pairs ? "pairs" : "reads", (unsigned long long)dmx_sum.n_assigned, (unsigned long long)dmx_sum.n_perfect, (unsigned long long)dmx_sum.n_short,
                    (unsigned long long)dmx_sum.n_far, (unsigned long long)dmx_sum.n_ambiguous);
    }
    if (of != stdout) fclose(of); else fflush(stdout);
    if (of2) fclose(of2);
    if (of3 && fclose(of3)) croak("-o merge=%s: error writing the file", o.ovl_merge.c_str());
    if (o.trim && !o.quiet)
        fprintf(stderr, "trimmed %llu of %llu records, %llu to nothing (%llu of %llu bases left)\n", (unsigned long long)trim_changed, (unsigned long long)trim_recs,
                (unsigned long long)trim_emptied, (unsigned long long)trim_out, (unsigned long long)trim_in);
    if (o.ovl && !o.ovl_hist.empty()) {
        FILE* hf = fopen(o.ovl_hist.c_str(), "w");
        if (!hf) croak("-o hist=%s: can't write the file", o.ovl_hist.c_str());
        fprintf(hf, "insert\tpairs\n");
        for (size_t i = 0; i <= 2 * SFQ_OVERLAP_MAX_LEN; i++)
            if (ovl_sum.insert_hist[i]) fprintf(hf, "%zu\t%llu\n", i, (unsigned long long)ovl_sum.insert_hist[i]);
        if (fclose(hf)) croak("-o hist=%s: error writing the file", o.ovl_hist.c_str());
    }
    if (merging && !o.quiet) {
        uint64_t seen = 0; size_t median = 0;                           // the median insert of the pairs that merged
        for (size_t i = 1; i <= 2 * SFQ_OVERLAP_MAX_LEN && !median; i++) { seen += ovl_sum.insert_hist[i]; if (mrg_merged && 2 * seen >= mrg_merged) median = i; }
        fprintf(stderr, "merged %llu of %llu pairs (%llu bases), median insert %zu\n", (unsigned long long)mrg_merged, (unsigned long long)ovl_sum.n_pairs,
                (unsigned long long)mrg_bases, median);
    } else if (o.ovl && !o.quiet) {
        // the median insert of the pairs that overlap
        uint64_t seen = 0; size_t median = 0;
        for (size_t i = 1; i <= 2 * SFQ_OVERLAP_MAX_LEN && !median; i++) { seen += ovl_sum.insert_hist[i]; if (ovl_sum.n_overlap && 2 * seen >= ovl_sum.n_overlap) median = i; }
        fprintf(stderr, "overlapped %llu of %llu pairs, cut %llu (%llu bases removed), median insert %zu\n", (unsigned long long)ovl_sum.n_overlap,
                (unsigned long long)ovl_sum.n_pairs, (unsigned long long)ovl_sum.n_cut, (unsigned long long)(ovl_sum.bases_in - ovl_sum.bases_out), median);
    }
    if (o.select && !o.quiet)
        fprintf(stderr, "kept %llu of %llu records (%llu of %llu bytes)\n", (unsigned long long)sel_kept, (unsigned long long)sel_seen,
                (unsigned long long)sel_bytes, (unsigned long long)sel_text);
    if (o.screen) {
        if (sfq_ctx_set_screen(ctx, nullptr) || sfq_screen_set_destroy(ctx)) croak("%s", sfq_last_error(ctx));
        const uint64_t matched = o.screen_rule.keep_matched ? scr_kept : scr_units - scr_kept;
        if (!o.quiet)
            fprintf(stderr, "screened %llu %s: %llu matched (%.2f %%), %llu kept (%llu k-mers of %u bases in the set)\n", (unsigned long long)scr_units,
                    scr_pairs ? "pairs" : "reads", (unsigned long long)matched, scr_units ? 100.0 * (double)matched / (double)scr_units : 0.0,
                    (unsigned long long)scr_kept, (unsigned long long)scr_kmers, o.screen_k);
    }
    if (o.bgzf && !o.quiet)
        fprintf(stderr, "deflated %llu bytes of text to %llu bytes in %llu members (%llu stored)\n", (unsigned long long)bgz_sum.text_bytes,
                (unsigned long long)bgz_sum.out_bytes, (unsigned long long)bgz_sum.members, (unsigned long long)bgz_sum.stored_members);
    if (o.dedup) {
        if (sfq_ctx_set_dedup(ctx, nullptr) || sfq_dedup_set_destroy(ctx)) croak("%s", sfq_last_error(ctx));
        if (!o.quiet)
            fprintf(stderr, "kept %llu of %llu %s (%llu duplicates, %.2f %%)\n", (unsigned long long)dd_kept, (unsigned long long)dd_units, dd_pairs ? "pairs" : "reads",
                    (unsigned long long)(dd_units - dd_kept), dd_units ? 100.0 * (double)(dd_units - dd_kept) / (double)dd_units : 0.0);
    }
}

int main(int argc, char** argv) {
    std::string fil;
    Opts o;
    bool statistics = false;
    if (argc == 1) usage();
    for (int opt; (opt = getopt(argc, argv, "qPsvhdObzZAFKYMD1234u:f:l:B:g:S:T:C:t:R:Q:p:W:x:k:c:o:G:X:")) != -1;) {
        switch (opt) {
        case 'u': g_usr = optarg; break;
        case 'f': fil = optarg; break;
        case 'l': o.level = (int)strtoll(optarg, 0, 0); break;
        case '1': case '2': case '3': case '4': o.level = opt - '0'; break;
        case 'd': g_encode = false; break;
        case 'O': o.overwrite = true; break;
        case 'P': break;
        case 'q': o.quiet = true; break;
        case 'B': o.block_reads = strtol(optarg, 0, 0); break;
        case 'S': o.slab_bytes = (uint64_t)std::max<long long>(1, strtoll(optarg, 0, 0)) << 20; break;
        case 'g': o.device = atoi(optarg); break;
        case 'T': o.table_pct = std::min(90, std::max(1, atoi(optarg))); break;
        case 'b': g_batch = true; break;
        case 'z': g_timing = true; break;
        case 'Z': o.bgzf = true; break;
        case 'A': o.adaptive = true; break;
        case 'F': o.force_frozen = true; break;
        case 'K': o.checksum = true; break;
        case 'Y': o.stats = true; break;
        case 'Q':
            o.qmap_name = optarg;
            o.qmap = o.qmap_name == "illumina8" ? SFQ_QMAP_ILLUMINA8 : o.qmap_name == "novaseq4" ? SFQ_QMAP_NOVASEQ4 : -1;
            break;
        case 'p': o.pair = optarg; break;
        case 'R': if (!parse_range(optarg, o.r_first, o.r_count)) usage(); o.range = true; break;
        case 'W':
            if (!parse_range(optarg, o.w_first, o.w_count) || o.w_first > (~0ull >> 2) || o.w_count > (~0ull >> 2)) {
                fprintf(stderr, "slimfastq: -W %s: a window of pairs is first:count, both decimal, count above 0\n", optarg);
                return 1;
            }
            o.window = true;
            break;
        case 'M': o.mates = true; break;
        case 'x':
            o.pick_name = optarg;
            o.pick = o.pick_name == "fasta" ? SFQ_PICK_FASTA : o.pick_name == "names" ? SFQ_PICK_NAMES : o.pick_name == "bases" ? SFQ_PICK_BASES :
                     o.pick_name == "quals" ? SFQ_PICK_QUALS : -1;
            break;
        case 'k': o.select = true; o.select_spec = optarg; break;
        case 'c': o.trim = true; o.trim_spec = optarg; break;
        case 'o': o.ovl = true; o.ovl_spec = optarg; break;
        case 'D': o.dedup = true; break;
        case 'G': o.screen = true; o.screen_spec = optarg; break;
        case 'X': o.demux = true; o.demux_spec = optarg; break;
        case 'C': o.chain_reads = strtol(optarg, 0, 0); break;
        case 't': o.io_threads = std::min(64, std::max(1, atoi(optarg))); break;
        case 'v': printf("Version %s\nInternal format version=%u (block format %u)\n", kUserVersion, kInternalVersion, kBlockVersion); exit(0);
        case 'h': usage();
        case 's': statistics = true; g_encode = false; break;
        default: fprintf(stderr, "slimfastq: Ilagal args: use -h for help\n"); exit(1);
        }
    }
    o.level = clamp_level(o.level);                                    // clamp at parse time (the reference records the clamped value only)
    if (o.checksum && o.block_reads == 0) {
        fprintf(stderr, "slimfastq: -K (checksums) needs the block format: -B 0 writes the reference's own format-6 file, which has no place for them\n");
        return 1;
    }

    if (o.qmap < 0) {
        fprintf(stderr, "slimfastq: -Q %s: no such quality map (illumina8 or novaseq4)\n", o.qmap_name.c_str());
        return 1;
    }
    if (o.qmap && !g_encode) {
        fprintf(stderr, "slimfastq: -Q (quality binning) goes with a compress run: it changes the text before it is coded, a decode writes what the archive holds\n");
        return 1;
    }

    if (o.bgzf && (g_encode || statistics)) {
        fprintf(stderr, "slimfastq: -Z (BGZF output) goes with -d: it compresses the text a decode writes%s\n", statistics ? "; -s writes no text" : "");
        return 1;
    }
    if (o.bgzf && o.range) {
        fprintf(stderr, "slimfastq: -Z does not go with -R: -R cuts the decoded text to its records on the host, and compressed bytes cannot be cut there "
                        "(-W cuts on the device and goes with -Z)\n");
        return 1;
    }
    if (o.range && g_encode) {
        fprintf(stderr, "slimfastq: -R (a range of records) goes with -d: it picks what a decode writes\n");
        return 1;
    }

    if (o.window && (g_encode || g_batch || o.range || o.pair.empty())) {
        fprintf(stderr, "slimfastq: -W (a window of pairs) goes with -d and -p: it picks the pairs a decode writes to -u and -p%s\n",
                o.range ? "; it does not go with -R, which counts records" : g_batch ? "; it does not go with -b" : "");
        return 1;
    }
    if (o.mates && (!g_encode || o.pair.empty())) {
        fprintf(stderr, "slimfastq: -M (the mates' names are compared) goes with -p on a compress run: %s\n",
                !g_encode ? "a decode writes what the archive holds" : "it compares the records of -u with those of -p");
        return 1;
    }

    if (o.pick < 0) {
        fprintf(stderr, "slimfastq: -x %s: no such selection (fasta, names, bases or quals)\n", o.pick_name.c_str());
        return 1;
    }
    if (o.pick && (g_encode || statistics)) {
        fprintf(stderr, "slimfastq: -x (picked lines) goes with -d: it picks the lines a decode writes%s\n", statistics ? "; -s writes no text" : "");
        return 1;
    }

    if (o.select) {
        char err[256] = "";
        int either = 0;
        if (sfq_select_parse(o.select_spec.c_str(), &o.sel, &either, err, sizeof err)) {
            fprintf(stderr, "slimfastq: -k %s: %s\n", o.select_spec.c_str(), err);
            return 1;
        }
        o.sel_either = either != 0;
        if (g_encode || statistics) {
            fprintf(stderr, "slimfastq: -k (selected records) goes with -d: it chooses the records a decode writes%s\n", statistics ? "; -s writes no text" : "");
            return 1;
        }
    }

    if (o.trim) {
        char err[256] = "";
        if (sfq_trim_parse(o.trim_spec.c_str(), &o.trim_rule, err, sizeof err)) {
            fprintf(stderr, "slimfastq: -c %s: %s\n", o.trim_spec.c_str(), err);
            return 1;
        }
        if (g_encode || statistics) {
            fprintf(stderr, "slimfastq: -c (trimmed records) goes with -d: it trims the records a decode writes%s\n", statistics ? "; -s writes no text" : "");
            return 1;
        }
    }

    if (o.ovl) {
        // hist=PATH is the CLI's own term: the library parses the others
        std::string rest;
        bool listed = false, others = false, merges = false;
        for (size_t at = 0; at <= o.ovl_spec.size(); ) {
            const size_t comma = std::min(o.ovl_spec.find(',', at), o.ovl_spec.size());
            const std::string term = o.ovl_spec.substr(at, comma - at);
            at = comma + 1;
            if (term.compare(0, 5, "hist=") == 0) { o.ovl_hist = term.substr(5); listed = true; continue; }
            if (term.compare(0, 6, "merge=") == 0) { o.ovl_merge = term.substr(6); merges = true; continue; }
            if (others) rest += ",";
            rest += term; others = true;
        }
        if ((listed || merges) && !others) rest = "default";           // hist=PATH, merge=PATH alone: the default rule
        char err[256] = "";
        if (listed && o.ovl_hist.empty()) snprintf(err, sizeof err, "hist=: names no file");
        else if (merges && o.ovl_merge.empty()) snprintf(err, sizeof err, "merge=: names no file");
        else if (sfq_overlap_parse(rest.c_str(), &o.ovl_rule, err, sizeof err) == 0) err[0] = 0;
        else if (!err[0]) snprintf(err, sizeof err, "not a list of terms");
        if (err[0]) {
            fprintf(stderr, "slimfastq: -o %s: %s\n", o.ovl_spec.c_str(), err);
            return 1;
        }
        if (merges && !o.ovl_rule.cut) {
            fprintf(stderr, "slimfastq: -o %s: nocut does not go with merge=PATH: a pair is merged or left whole, nothing is cut\n", o.ovl_spec.c_str());
            return 1;
        }
        if (merges && o.range && ((o.r_first | o.r_count) & 1)) {
            fprintf(stderr, "slimfastq: -o merge= with -R %llu:%llu: pairs are merged, so a range is whole pairs (an even first record and an even count); "
                            "-W F:N names pairs\n", (unsigned long long)o.r_first, (unsigned long long)o.r_count);
            return 1;
        }
        if (g_encode || statistics || g_batch) {
            fprintf(stderr, "slimfastq: -o (overlapping mates) goes with -d: it cuts the records a decode writes%s\n",
                    statistics ? "; -s writes no text" : g_batch ? "; it does not go with -b" : "");
            return 1;
        }
    }

    if (o.screen) {
        // ref=PATH is the CLI's own term: the library checks the others (and skips these)
        char err[256] = "";
        if (sfq_screen_parse(o.screen_spec.c_str(), &o.screen_rule, &o.screen_k, err, sizeof err)) {
            fprintf(stderr, "slimfastq: -G %s: %s\n", o.screen_spec.c_str(), err[0] ? err : "not a list of terms");
            return 1;
        }
        if (g_encode || statistics || g_batch) {
            fprintf(stderr, "slimfastq: -G (screened records) goes with -d: it screens the records a decode writes%s\n",
                    statistics ? "; -s writes no text" : g_batch ? "; it does not go with -b" : "");
            return 1;
        }
        // the references are read and flattened here: an unreadable or empty one ends the run before anything is decoded
        for (size_t at = 0; at <= o.screen_spec.size(); ) {
            const size_t comma = std::min(o.screen_spec.find(',', at), o.screen_spec.size());
            const std::string term = o.screen_spec.substr(at, comma - at);
            at = comma + 1;
            if (term.compare(0, 4, "ref=") != 0) continue;
            const std::string path = term.substr(4);
            FILE* rf = fopen(path.c_str(), "rb");
            if (!rf) { fprintf(stderr, "slimfastq: -G: can't read the reference '%s'\n", path.c_str()); return 1; }
            std::vector<uint8_t> fa;
            uint8_t buf[1 << 16];
            for (size_t got; (got = fread(buf, 1, sizeof buf, rf)) > 0; ) fa.insert(fa.end(), buf, buf + got);
            const bool bad = ferror(rf) != 0;
            fclose(rf);
            if (bad) { fprintf(stderr, "slimfastq: -G: can't read the reference '%s'\n", path.c_str()); return 1; }
            const int64_t need = sfq_fasta_sequences(fa.data(), fa.size(), nullptr, 0);
            std::vector<uint8_t> seq((size_t)std::max<int64_t>(need, 0));
            if (need <= 0 || sfq_fasta_sequences(fa.data(), fa.size(), seq.data(), seq.size()) != need ||
                std::all_of(seq.begin(), seq.end(), [](uint8_t c) { return c == '\n'; })) {    // (nothing but names)
                fprintf(stderr, "slimfastq: -G: the reference '%s' holds no sequence\n", path.c_str());
                return 1;
            }
            o.screen_seqs.push_back(std::move(seq));
        }
        if (o.screen_seqs.empty()) {
            fprintf(stderr, "slimfastq: -G %s: names no reference (ref=PATH, a FASTA file)\n", o.screen_spec.c_str());
            return 1;
        }
    }

    if (o.dedup && (g_encode || statistics || g_batch)) {
        fprintf(stderr, "slimfastq: -D (distinct records) goes with -d: it drops the duplicates of what a decode writes%s\n",
                statistics ? "; -s writes no text" : g_batch ? "; it does not go with -b" : "");
        return 1;
    }

    if (o.demux) {
        // the sheet (the first term) and the file terms are the CLI's own: the library checks the others (and skips these)
        char err[256] = "";
        if (g_encode || statistics || g_batch) {
            fprintf(stderr, "slimfastq: -X (demultiplexed records) goes with -d: it sorts the records a decode writes by sample%s\n",
                    statistics ? "; -s writes no text" : g_batch ? "; it does not go with -b" : "");
            return 1;
        }
        if (o.pick || o.window || !o.ovl_merge.empty()) {
            fprintf(stderr, "slimfastq: -X (demultiplexed records) does not go with %s\n", o.pick ? "-x: the sample files are whole records" :
                    o.window ? "-W: a window of pairs is not sorted by sample" : "-o merge=: merged pairs are not sorted by sample");
            return 1;
        }
        if (sfq_demux_parse(o.demux_spec.c_str(), &o.demux_rule, err, sizeof err)) {
            fprintf(stderr, "slimfastq: -X %s: %s\n", o.demux_spec.c_str(), err[0] ? err : "not a list of terms");
            return 1;
        }
        std::string sheet;
        for (size_t at = 0, i = 0; at <= o.demux_spec.size(); i++) {
            const size_t comma = std::min(o.demux_spec.find(',', at), o.demux_spec.size());
            const std::string term = o.demux_spec.substr(at, comma - at);
            at = comma + 1;
            if (!i) sheet = term;
            else if (term.compare(0, 4, "out=") == 0) o.demux_out = term.substr(4);
            else if (term.compare(0, 7, "counts=") == 0) o.demux_counts = term.substr(7);
        }
        if (o.demux_out.empty()) { fprintf(stderr, "slimfastq: -X %s: names no sample files (out=PREFIX)\n", o.demux_spec.c_str()); return 1; }
        FILE* sf = fopen(sheet.c_str(), "rb");
        if (!sf) { fprintf(stderr, "slimfastq: -X: can't read the sample sheet '%s'\n", sheet.c_str()); return 1; }
        std::string text;
        char buf[1 << 16];
        for (size_t got; (got = fread(buf, 1, sizeof buf, sf)) > 0; ) text.append(buf, got);
        fclose(sf);
        std::vector<char> names((size_t)SFQ_DEMUX_MAX_SAMPLES * 65);
        o.demux_codes.resize((size_t)SFQ_DEMUX_MAX_SAMPLES * 32);
        uint32_t ns = 0, l0 = 0, l1 = 0;
        if (sfq_demux_sheet(text.data(), text.size(), SFQ_DEMUX_MAX_SAMPLES, names.data(), o.demux_codes.data(), &ns, &l0, &l1, err, sizeof err)) {
            fprintf(stderr, "slimfastq: -X %s: %s\n", sheet.c_str(), err);
            return 1;
        }
        for (uint32_t i = 0; i < ns; i++) o.demux_names.push_back(names.data() + (size_t)i * 65);
        sfq_demux& d = o.demux_rule;
        d.n_samples = ns;
        d.part[0].len = l0;
        if (l1 && d.part[1].src == 0) d.part[1] = sfq_demux_part{ SFQ_DEMUX_BASES, 0, 0, d.part[0].pos + l0, 0 };      // inline alone: part 1 follows part 0
        d.part[1].len = l1;
        const bool paired = !o.pair.empty();
        if (d.part[1].len && d.part[1].mate && !paired) { fprintf(stderr, "slimfastq: -X inline2 reads the second mates: it needs -p\n"); return 1; }
        d.pairs = paired ? 1 : 0; d.split_mates = d.pairs;
        if (sfq_demux_check(&d, o.demux_codes.data())) {
            fprintf(stderr, "slimfastq: -X %s: the library refuses the rule (mm=%u with barcodes of %u bases?)\n", o.demux_spec.c_str(), d.max_mm, l0 + l1);
            return 1;
        }
        d.pairs = 0;                                                   // (decided per archive: units are pairs where -D's are)
        // the files: two a sample with -p, the unassigned ones' (-u, -p), the counts
        struct rlimit rl;
        const unsigned long long files = (unsigned long long)ns * (paired ? 2 : 1) + (paired ? 2 : 1) + (o.demux_counts.empty() ? 0 : 1);
        if (getrlimit(RLIMIT_NOFILE, &rl) == 0 && rl.rlim_cur != RLIM_INFINITY && files + 16 > (unsigned long long)rl.rlim_cur) {
            fprintf(stderr, "slimfastq: -X: %llu files are more than this process may hold open (%llu, of which 16 are kept back): raise the limit (ulimit -n)\n",
                    files, (unsigned long long)rl.rlim_cur);
            return 1;
        }
        if (!o.overwrite) {
            std::vector<std::string> all;
            for (const std::string& nm : o.demux_names)
                for (int g = 0; g < (paired ? 2 : 1); g++) all.push_back(o.demux_out + nm + (paired ? (g ? "_R2" : "_R1") : "") + ".fastq");
            if (!o.demux_counts.empty()) all.push_back(o.demux_counts);
            for (const std::string& f : all)
                if (access(f.c_str(), F_OK) == 0) { fprintf(stderr, "Can't write file '%s': File exists\n", f.c_str()); return 1; }
        }
    }

    if (!o.pair.empty() && g_batch) {
        fprintf(stderr, "slimfastq: -p (paired files) names one file: it does not go with -b, whose jobs name theirs\n");
        return 1;
    }
    if (!o.pair.empty() && o.range) {
        fprintf(stderr, "slimfastq: -p (paired files) does not go with -R: a range may start at a second mate\n");
        return 1;
    }

    if (g_batch) {
        sfq_ctx* ctx = nullptr;
        const int rc = sfq_ctx_create(&ctx, o.device);
        if (rc) { fprintf(stderr, "slimfastq: no usable HIP device (error %d): this build has no CPU path\n", rc); return 1; }
        if (o.table_pct) sfq_ctx_set_table_budget(ctx, sfq_ctx_device_memory(ctx) / 100 * (uint64_t)o.table_pct);
        char* line = nullptr; size_t cap = 0; ssize_t n;
        int failed = 0;
        while ((n = getline(&line, &cap, stdin)) > 0) {
            while (n > 0 && (line[n - 1] == '\n' || line[n - 1] == '\r')) line[--n] = 0;
            if (!n) continue;
            char* tab = strchr(line, '\t');
            if (!tab) { printf("fail\t%s\texpected '<source>\\t<target>'\n", line); fflush(stdout); failed++; continue; }
            *tab = 0;
            const std::string src = line, dst = tab + 1;
            try {
                if (g_encode) encode_file(ctx, o, src, dst); else decode_file(ctx, o, dst, src);
                printf("ok\t%s\t%s\n", src.c_str(), dst.c_str());
            } catch (const JobError& e) {
                printf("fail\t%s\t%s\n", src.c_str(), e.msg.c_str());
                failed++;
            } catch (const std::exception& e) {                        // e.g. bad_alloc on a hostile archive: the job fails, the worker lives
                if (!g_partial.empty()) { unlink(g_partial.c_str()); g_partial.clear(); }
                printf("fail\t%s\t%s\n", src.c_str(), e.what());
                failed++;
            }
            fflush(stdout);
        }
        free(line);
        sfq_ctx_destroy(ctx);
        return failed ? 2 : 0;
    }

    while (optind < argc) {                                            // DWIM, config.cpp:279-325 (simplified)
        const char* file = argv[optind++];
        FILE* fh = fopen(file, "rb");
        char head[20] = {0};
        size_t cnt = fh ? fread(head, 1, 19, fh) : 0;
        if (fh) fclose(fh);
        if (cnt && fil.empty() && !strncmp(head, "whoami=slimfastq", 16)) { fil = file; g_encode = !g_usr.empty(); }
        else if (cnt && g_usr.empty() && head[0] == '@') g_usr = file;
        else if (!g_encode && g_usr.empty()) g_usr = file;
        else if (g_encode && fil.empty()) fil = file;
        else { fprintf(stderr, "What am I suppose to do with '%s'?\n (please specify explicitly with -f/-u prefix)\n", file); exit(1); }
    }
    if (!o.pair.empty() && !statistics && g_usr.empty()) {
        fprintf(stderr, "slimfastq: -p (paired files) needs -u: the first mates are a file, not %s\n", g_encode ? "stdin" : "stdout");
        return 1;
    }
    if (fil.empty()) { fprintf(stderr, "Missing essential argument: -f\n"); exit(1); }

    try {
    std::string err;
    if (statistics) {                                                  // config.cpp:76-85
        sfqc::Archive a;
        if (!sfqc::read_file(fil, a, err)) croak("%s", err.c_str());
        fprintf(stderr, ":::: Info ::::\n");
        for (auto& kv : a.info) fprintf(stderr, "%-16s = %s\n", kv.first.c_str(), kv.second.c_str());
        fprintf(stderr, "\n:::: Files stream ::::\n i: name      : bytes\n");
        int i = 1;
        for (auto& s : a.streams) fprintf(stderr, "%2d: %-10s: %zu\n", i++, s.first.c_str(), s.second.size());
        if (const std::vector<uint8_t>* ts = a.find("txt.stat")) print_text_stats(*ts);
        return 0;
    }

    sfq_ctx* ctx = nullptr;
    tick("process start");
    const int rc = sfq_ctx_create(&ctx, o.device);
    if (rc) croak("no usable HIP device (error %d): this build has no CPU path", rc);
    tick("sfq_ctx_create");
    if (o.table_pct) sfq_ctx_set_table_budget(ctx, sfq_ctx_device_memory(ctx) / 100 * (uint64_t)o.table_pct);
    if (g_encode) encode_file(ctx, o, g_usr, fil); else decode_file(ctx, o, g_usr, fil);
    tick("done");
    } catch (const JobError& e) {                                      // croak(): config.cpp:54-68
        fprintf(stderr, "slimfastq: %s %s: %s\n", g_encode ? "encoding" : "decoding", g_usr.empty() ? "<< stdin >>" : g_usr.c_str(), e.msg.c_str());
        fflush(nullptr);
        _exit(1);
    }
    // a one-shot process: the driver reclaims the context's 10s of GB faster than freeing them one by one
    fflush(nullptr);
    _exit(0);
}

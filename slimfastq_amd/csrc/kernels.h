// kernels.h -- launch wrappers exported by the .hip translation units to the C-ABI host code.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_common.h"

// Arguments shared by every model kernel.  Block b of a launch uses table slot (b - batch0).
struct ModelArgs {
    const u8*  fq;          // FASTQ text (encode) -- device
    const u64* line_off;    // line_off[k] = offset of line k; line_off[nlines] = nbytes
    BlockDesc* blocks;
    u32 nblocks;            // total
    u32 batch0, nbatch;     // this launch covers blocks [batch0, batch0+nbatch)
    u8* arena;              // per-block stream regions (BlockDesc::out_off/out_cap)
    i32 level;
    u32 lossless;           // the block format's rules (dev_common.h): string fallback for header numbers, "gen.lc", the '+' line check
    u32 epoch_base;         // block b runs with epoch epoch_base + b + 1
    // tables
    u32* q_slots; RowHdr* q_hdr; u32 q_rows;     // Log64 rows per slot: 4096 (level 1) or 65536
    u32* p_slots; RowHdr* p_hdr;                 // PR_ROWS PowerRanger rows per slot
    u32* g_tab;   u32 g_bits;                    // (1 << g_bits) Base2 dwords per slot
    // quality warm start (prior.hip); all null = cold rows, the reference's behaviour
    const u32* prior_w; const u32* prior_wovf;   // wave layout [q_rows][64] + overflow [q_rows][4]
    const u32* prior_ls; const RowHdr* prior_lh; // lane-per-block layout
    // format 6 with oversize records (frame.hip): the model kernels see the text without them; rec_map[k] = the file number
    // (0-based) of the k-th record they see -- the exception streams count records in file numbers (g_record_count).  Null: k itself.
    const u32* rec_map;
};
// g_record_count (config.cpp:43) of record r of a block that starts at base: block-relative, 1-based
__device__ __forceinline__ u64 rec_count_of(const ModelArgs& a, u64 r, u64 base) { return a.rec_map ? (u64)a.rec_map[r] + 1 : r - base + 1; }

// Decode-side extras.
struct DecodeArgs {
    ModelArgs m;
    const u8*  streams;                     // compact streams (device)
    const u64* blk_stream_off;              // [nblocks][SFQ_NSTREAMS] absolute offsets into streams
    const u8*  first_hdrs;                  // blob (device)
    u32* slen; u32* qlen;                   // per record (device), filled by the usr kernel
    u8*  pfg;  u8* pfq;                     // per record solid prefixes
    const u64* soff; const u64* qoff;       // exclusive scans of slen/qlen
    const u64* boff;                        // match model (gm.hip): soff[r] = boff[r] + r -- a '\n' behind every staged base line; null: soff is the plain scan
    u8*  seq_stage; u8* qual_stage;         // decoded bases / qualities
    u8*  hdr_stage; u32* hlen;              // decoded headers, back to back per block
    const u64* hdr_stage_off;               // per block base into hdr_stage
    const u32* hdr_stage_cap;
    u64* hoff;                              // per record offset into hdr_stage (filled by rec decode)
    u32  block_reads;                       // records per block (uniform; the last block may be short)
    u32  version;                           // archive format version (recs.cpp:400: < 5 takes load_pre5)
    u32  max_line;                          // a base / quality line longer than this is a corrupt stream (the caller's output capacity bounds it)
};

// ---- lane-per-chain kernels with frozen tables (chains.hip, dev_chain.h) ----------------------------------------
struct ChainGeoArgs { u32 chain_reads, cpb, nchains; };     // chain c = chain c % cpb of block c / cpb
#define RDEC_LDS_ROWS 16u              // header rows (decoder's form) a workgroup of the fast header decoder stages in LDS
#define GEN_MAX_GENERATIONS 40
struct ChainArgs {
    ModelArgs m;
    ChainGeoArgs geo;           // chains of the quality and base streams
    ChainGeoArgs rgeo;          // chains of the header stream (longer: each starts from the block's first header)
    u32* rhb;                   // [rgeo.nchains] header bytes of each header chain (encode: written)
    u64 nbytes;                 // size of the FASTQ text (encode)
    u32 block_reads;            // records per block (uniform; the last block may be short)
    u32* csz;                   // [nchains] sizes of the stream being coded (encode: written; decode: read)
    const u64* coff;            // decode: [nchains] absolute offsets of the chains' streams
    // quality: frozen rows, total 2^16 each
    const u32* qrows;           // [q_rows][64] cum | freq << 16, in symbol order, indexed by the context
    const u16* qdec;            // decode: [q_rows][72] u16: the cum of every 8th symbol, then the cums of symbols 1 .. 64 (chains.hip QDEC_ROW)
    u32 q_rows;                 // quality contexts: 4096 (level 1) or 65536
    u32 q_hot;                  // room for that many rows in the LDS image of the quality chains' workgroups (0 = no staging)
    const u8* qh_img;           // the hot image: map, then rows (chains.hip k_hot_select)
    const u32* qh_info;         // [0] = rows staged
    const u32* qesc;            // escape row (256 entries), qlts.cpp:80-86
    // headers: frozen PowerRanger rows, total 2^16 each
    const u32* rrows;           // [PR_REC_ROWS][256] cum | freq << 16
    const u16* rdec;            // decode: [PR_REC_ROWS][272] u16: the cum at every 16th symbol, then of all 256 (chains.hip RDEC_ROW)
    const u16* rmap; const u16* rhot; u32 r_hot;   // rows staged in LDS: row -> place by weight (0xFFFF = none; a kernel stages the first few), place -> row, how many to stage
    u8* exc_flag;               // encode: [records] set to 1 by the quality / base chains where a record holds a '!' / an N (null = not wanted)
    // chains that are PARTS of one record (long reads; chains.hip "segments"): seg_len != 0, geo.chain_reads = 1
    u32 seg_len;                // symbols per segment asked for; a record of M = max(bases, qualities) symbols is cut into
                                // n = ceil(M / seg_len) segments of ceil(M / n) symbols, a chain each, in both streams
    const u64* seg_off;         // [records + 1] chains before each record
    const u32* seg_rec;         // [nchains] the record a chain belongs to
    // bases: where a counting pass reads them (decode: the staged bases; null = the FASTQ text through line_off)
    const u8* st_buf; u64 st_bytes; const u64* st_off; const u32* st_len;
    // bases: generation tables
    u32 g_ngen;                 // 0 = every chain codes with the initial row
    u32 g_bound[GEN_MAX_GENERATIONS + 1];      // generation g = blocks [g_bound[g], g_bound[g + 1])
    const u32* g_rows[GEN_MAX_GENERATIONS];    // its rows (null = the initial row)
    const u32* g_init;          // encode: one dword holding the initial row (3, 3, 3, 3), read where a generation has no rows
    u32 flat_quads;             // bases without a model (round 5, "chn.idx" flag CHN_FLAT_QUADS): a line's bases four at a time, one symbol of 4^k equally likely ones
    u32 flat_raw;               // bases without a model (round 5b, "chn.idx" flag CHN_FLAT_RAW, block format 10): a chain's bases two bits each, four a byte, no coder
                                // (k = 4, fewer at a line's end) instead of 3 of 12 a base
};
void launch_hot_rows(const u32* hist, const u32* rows66, const u32* qrows, u32 q_rows, u32 want, u32* ctot /* [q_rows] */,
                     u8* img /* q_rows / 4 bytes of map + want x 100 bytes of rows */, u32* info, hipStream_t st);
void launch_hot_rows_dec(const u32* rows66, const u16* qdec, u32 q_rows, u32 want, u32* ctot /* [q_rows] */,
                         u8* img /* q_rows / 4 bytes of map + want x 16 bytes of coarse lists */, u32* info, hipStream_t st);
u32 hot_rows_dec_max(void);     // how many coarse lists a workgroup's LDS holds beside the map
void launch_qlt_frozen_rows(const u32* rows66, u32 q_rows, u32* qrows, u16* qdec /* decode; may be null */, hipStream_t st);
void launch_qlt_encode_c(const ChainArgs& a, hipStream_t st);
void launch_gen_count(const ChainArgs& a, u32 b0, u32 b1, u64 nrec_range, u32 max_line /* the longest base line (picks lane per record / per stretch) */,
                      u32* cnt, const u32* rows, const u16* log2fp, u64* cost, hipStream_t st,
                      u32 sub = 0 /* 0 every selected record, 1 every GEN_PRE-th of them, 2 the others */, u32 do_count = 1 /* 0: the cost only */);
void launch_gen_rows(const u32* cnt, u32* rows, u64 nctx, u32 step, hipStream_t st);
// ---- bases under the generation MATCH model (gm.hip, round 5) ----
void launch_gm_lens(const u64* line_off, const BlockDesc* blocks, u32 block_reads, u64 n, u32* slen, hipStream_t st);       // base-line lengths of records [0, n)
void launch_gm_soff(const u64* boff, u64 n, u64* soff, hipStream_t st);                                                       // soff[r] = boff[r] + r, r in [0, n]
void launch_gm_sentinels(u8* stage, const u64* soff, const u32* slen, u64 n, hipStream_t st);
void launch_gm_stage(const ModelArgs& m, u32 block_reads, u64 r0, u64 r1, u64 nbytes /* of the text */, u8* stage, const u64* soff, const u32* slen, u8* exc_flag /* or null */, hipStream_t st);
// (a: ChainArgs whose st_buf / st_off / st_len describe the stage)
void launch_gm_insert(const ChainArgs& a, u32 b0, u32 b1, u64 nrec_range, u32 max_line, u64* T, u32 tb, hipStream_t st);
void launch_gm_plan(const ChainArgs& a, u64 nlanes /* records, or chains where they are segments */, const u8* stage, u64 stage_bytes, const u64* soff, const u32* slen,
                    const u64* T, u32 tb, u8* tok, hipStream_t st);
void launch_gm_price(const ChainArgs& a, u64 r0, u64 r1, u64 step, u32 max_line /* the call's longest base line: a lane per 256 bases of a record */, u64 lim_rec, const u8* stage, u64 stage_bytes, const u64* soff, const u32* slen, const u64* T, u32 tb,
                     const u16* costs /* hit[4], miss[4] in 1/1024 bit */, u64* cost /* [0] += cost, [1] += bases */, hipStream_t st);
void launch_gm_code(const ChainArgs& a, const u8* tok, hipStream_t st);
void launch_gm_decode_c(const ChainArgs& a, const struct DecodeArgs& da, u32 c0, u32 c1, u64 lim_rec, const u64* T, u32 tb, u64 stage_bytes, hipStream_t st);
// the same counts through bins (chains.hip "counting through bins": two streaming passes instead of a global atomic per base);
// rows_out != null: the rows of the sums are written as well (launch_gen_rows folded in).  bins / fill: scratch, fill zeroed by the caller
#define GEN_BIN_BATCH (1ull << 27)      /* keys a pair of passes takes at most (the bins hold twice that, 2 bytes a key) */
struct GenBins { u16* bins; u32* fill; u32 cap, g_bits; u64 batch, bins_bytes, fill_bytes; };
GenBins gen_bins_plan(u32 g_bits, u64 max_keys /* the bases a counting pass can meet (the call's text is a bound) */);
void launch_gen_count_binned(const ChainArgs& a, u32 b0, u32 b1, u64 nrec_range, u32 max_line, const GenBins& gb, u32* cnt, u32* rows_out, u32 step,
                             hipStream_t st, u32 sub = 0);
void launch_gen_encode_c(const ChainArgs& a, hipStream_t st, u32 c0 = 0, u32 c1 = 0 /* chains [c0, c1); 0, 0 = all */, bool flat = false /* every chain: the initial row */);
// gen.Ns / gen.Nn side streams, a wave per block (models_w.hip); flags: the records that may hold an exception (null = look at all)
// "chn.idx": the flag byte behind the records per chain.  The ONE definition of its bits: api.cpp writes and reads by these names
// (tests/util.py parse_chain_index mirrors the numbers on purpose)
enum ChnFlag : u32 {
    CHN_GEN_ON     = 1u << 0,   // the bases' generation tables (or, with CHN_GEN_MATCH, their match model) are in use
    CHN_REC_CHAINS = 1u << 1,   // the headers are coded chain by chain: their geometry and two more lists follow
    CHN_DELTAS     = 1u << 2,   // every list of sizes as zigzag differences to the entry before (version-8 archives: plain)
    CHN_SEGMENTS   = 1u << 3,   // chains are segments of one record (long reads): their length and the blocks' shares follow
    CHN_EXC_RICE   = 1u << 4,   // the base exceptions are Rice-coded gap lists (exc.hip)
    CHN_GEN_MATCH  = 1u << 5,   // the bases are coded under the match model (gm.hip): the index's bits and the base chains' geometry follow
    CHN_FLAT_QUADS = 1u << 6,   // bases without a model, four a symbol through the coder (block format 9; still read)
    CHN_FLAT_RAW   = 1u << 7,   // bases without a model, two bits each, no coder (block format 10)
    CHN_KNOWN      = (1u << 8) - 1
};
// "chn.idx": the size lists csz[0 .. n) (lists [0, b1), [b1, b2), [b2, b3), [b3, n)) as zigzag-difference varints, back to back in
// out; len[n], off[n + 1], scan_tmp: scratch; info[0] = bytes before list b2, info[1] = all
void launch_chain_index_bytes(const u32* csz, u32 n, u32 b1, u32 b2, u32 b3, u32* len, u64* off, u64* scan_tmp, u8* out, u64* info, hipStream_t st);
void launch_gen_exc_w(const ModelArgs& a, const u8* flags, u32* ticket, hipStream_t st);
// the same lists as adaptive Rice codes (models_w.hip k_gen_exc_w<true>, dev_rice.h; frozen tables, "chn.idx" flag CHN_EXC_RICE) and the way back, a lane per block (exc.hip)
void launch_gen_exc_r(const ModelArgs& a, const u8* flags, u32* ticket, hipStream_t st);
void launch_gen_exc_decode_r(const struct DecodeArgs& a, u32 b0, u32 b1 /* blocks [b0, b1) */, hipStream_t st);
#define REC_COUNT_COPIES 32u        // the header prior's counting pass counts into this many copies of the table (chains.hip k_rec_count_sum)
void launch_rec_count(const ModelArgs& a, u64 nrec, u64 stride, u32 run, u32 nruns, u32* cnt /* [REC_COUNT_COPIES][PR_REC_ROWS][256], zeroed; the sums end up in copy 0 */,
                      u32* flags /* [nruns], zeroed */, hipStream_t st);
void launch_rec_frozen_rows(const u32* f, u32 nrows, u32* rrows, u16* rdec /* the decoder's form; may be null */, hipStream_t st);
// counts -> the transmitted prior's frequencies f[nrows][256], the rows' sums rtot[nrows], and the nh heaviest rows (map[nrows], hot[nh])
void launch_rec_prior_freqs(const u32* cnt, u32 nrows, u32* f, u32* rtot, u32 nh, u16* map, u16* hot, hipStream_t st);
// one header chain per lane; a.csz / a.rhb per chain; max_hdr = the call's longest header (picks the LDS image of the fast kernel)
void launch_rec_encode_c(const ChainArgs& a, u32* flags /* [rgeo.nchains], zeroed */, u32* flags2 /* the same */, u32* tok /* rec_token_bytes(records) */, u32* ntok /* [rgeo.nchains] */,
                         u32 n_hot, u32 max_hdr, hipStream_t st,
                         u32 min_hdr = 0 /* the call's shortest header: over 127 = every chain to the general kernel, nothing else launched */,
                         hipEvent_t after_tokens = nullptr /* recorded behind the token step (the longest kernel of the five), for sfq_result.coder_ms */);
u64 rec_token_bytes(u64 nrec);
// segments: chains per record (from the text's line index, or from the decoder's line lengths), then the chains' records
void launch_seg_count(const u64* line_off, const BlockDesc* blocks, u32 block_reads, u64 nrec, u32 seg_len, u32* nseg, hipStream_t st);
void launch_seg_count_dec(const u32* slen, const u32* qlen, u64 nrec, u32 seg_len, u32* nseg, hipStream_t st);
void launch_seg_fill(const u64* seg_off, u64 nrec, u32* seg_rec, hipStream_t st);
void launch_chain_block_sizes(const ChainArgs& a, const ChainGeoArgs& geo, int stream, const u32* csz, const u32* rhb /* or null */, hipStream_t st);
void launch_compact_chains(const ChainArgs& a, const ChainGeoArgs& geo, int stream, u32 num, u32 den, const u32* csz, const u64* blk_stream_off,
                           const u64* stream_base, u8* out, hipStream_t st, const u32* gate /* frame.hip k_stream_gate */);
#define GEN_STEP 4u             // a counted base adds GEN_STEP to its row entry (chains.hip)
// A generation of n records (its blocks x block_reads: the last block of a call may be short) is counted through every
// s-th record, s = ceil(n / GEN_COUNT_CAP): half a million records tell a row's shape, and the counting -- a
// scattered atomic per base into a table of 2^gen_bits x 16 bytes -- was most of the time of inputs whose bases can be
// learned (half of a 10 M-read call: 50 ms).  The decoder counts the same records.
#ifndef GEN_COUNT_CAP
#define GEN_COUNT_CAP 524288ull
#endif
#define GEN_PRE 8u                      /* the pre-verdict looks at every 8th of the records a counting pass takes (api.cpp gen_tables_begin) */
static inline u32 gen_count_stride(u64 n) { return (u32)((n + GEN_COUNT_CAP - 1) / GEN_COUNT_CAP ? (n + GEN_COUNT_CAP - 1) / GEN_COUNT_CAP : 1); }

// framing
void launch_max_u32(const u32* v, u64 n, u32* out /* raised to the largest of v */, hipStream_t st);
// format 6's oversize records (frame.hip, models_w.hip)
void launch_over_first(const u64* line_off, u64 nrec, u32* first /* 0xFFFFFFFF */, hipStream_t st);
void launch_over_solid(const u8* fq, const u64* line_off, u64 r, u32* out, hipStream_t st);
void launch_over_flags(const u64* line_off, u64 nrec, u32 solid, u32* flags, u32* kbytes, u32* status, hipStream_t st);
void launch_over_split(const u8* fq, const u64* line_off, u64 nrec, const u32* flags, const u64* fpos, const u64* koff, u8* filt, u32* rec_map, u32* over_list, hipStream_t st);
void launch_over_encode_w(const ModelArgs& a, const u8* fq, const u64* line_off, const u32* over_list, u32 n_over, const u64 out_off[3], const u32 out_cap[3], hipStream_t st);
void launch_over_mark(const u64* over_no, u32 n_over, u64 total, u32* flags /* zeroed */, u32* status, hipStream_t st);
void launch_over_map(const u32* flags, const u64* fpos, u64 total, u32* rec_map, hipStream_t st);
void launch_over_decode_w(const ModelArgs& a, const u8* stream, u32 size, u32 which, u32 store, u32 n_over, u64* cnt, u64* no, u64* piece, u8* txt, u64 cap, hipStream_t st);
void launch_over_place(u32 n_over, const u64* no, const u64* piece, const u8* lrec_txt, const u8* lgen_txt, const u8* lqlt_txt, const u64* roff_all, u8* out, hipStream_t st);
void launch_over_sizes(const u32* rec_map, const u32* rsize, u64 n_kept, const u64* no, const u64* piece, u32 n_over, u32* size_all, hipStream_t st);
void launch_gather_u64(const u64* src, const u32* idx, u64 n, u64* dst, hipStream_t st);
void launch_block_prepare(const u8* fq, const u64* line_off, u64 nrec, u32 block_reads, BlockDesc* blocks, u32 nblocks,
                          u64 nbytes, i32 level, i32 gen_bits_req, hipStream_t st);
// framing in one pass (frame.hip k_frame): the line index (at most cap entries behind entry 0 are written), the '@' / '+' checks into
// status[0], the marks of the exception pass; frame_out: { u64 lines, u32 look-back guard tripped }
u32 frame_tiles(u64 n);
void launch_frame(const u8* fq, u64 n, u64* tstat /* [frame_tiles(n)], zeroed */, u64* line_off, u64 cap, u32* status, u8* exc_flag /* or null */, u64 ecap /* its entries */,
                  void* frame_out /* 16 bytes, zeroed */, hipStream_t st);
void launch_validate_lines(const u64* line_off, u64 nrec, u32 max_hdr, u32 max_line, u32* status, hipStream_t st);
void launch_text_fingerprint(const u8* fq, u64 n, u64* out /* zeroed */, hipStream_t st);
#define FRAME_CHUNK 16384u

// generic exclusive scan u32 -> u64 (out has n+1 entries)
void launch_scan_u32(const u32* in, u64* out, u64 n, u64* tmp /* >= n/1024+2 */, hipStream_t st, u32 pad = 0 /* 2^k - 1: the values rounded up to multiples of 2^k */);

// models, lane-per-block reference kernels
void launch_qlt_encode_l(const ModelArgs& a, hipStream_t st);
void launch_gen_encode_l(const ModelArgs& a, hipStream_t st);
void launch_rec_encode_l(const ModelArgs& a, hipStream_t st);
void launch_usr_encode_l(const ModelArgs& a, hipStream_t st);
void launch_fill_u32(u32* p, u64 n, u32 v, hipStream_t st);

// models, wave-per-block throughput kernels (persistent: one workgroup per pair of table slots -- a.nbatch is even --
// blocks 0..a.nblocks-1 are handed out through *ticket, which must be 0)
void launch_qlt_encode_k(const ModelArgs& a, u32* ticket, hipStream_t st);
void launch_gen_encode_k(const ModelArgs& a, u32* ticket, hipStream_t st);
void launch_rec_encode_w(const ModelArgs& a, u32* ticket_fast, u32* ticket_slow, hipStream_t st);
void launch_usr_encode_w(const ModelArgs& a, hipStream_t st);      // framing exceptions, a wave per block; blocks [batch0, batch0 + nbatch), slot = workgroup

void launch_qlt_decode_c(const ChainArgs& a, const DecodeArgs& da, u32 c0, u32 c1 /* chains [c0, c1) */, hipStream_t st);
void launch_gen_decode_c(const ChainArgs& a, const DecodeArgs& da, u32 c0, u32 c1 /* chains [c0, c1) */, hipStream_t st);
void launch_rec_decode_c(const ChainArgs& a, const DecodeArgs& da, u32* flags /* [rgeo.nchains], zeroed; null = general path only */, hipStream_t st,
                         u32* dtok = nullptr /* rec_dtok_bytes(records); null = the lane kernels alone */, u32* dtoff = nullptr /* [records] */, u32* dflags = nullptr /* [rgeo.nchains], zeroed */,
                         u32 c0 = 0, u32 c1 = 0 /* header chains [c0, c1); 0, 0 = all */);
u64 rec_dtok_bytes(u64 nrec);
void launch_gen_exc_decode_l(const DecodeArgs& a, hipStream_t st);          // applies gen.Ns / gen.Nn to the staged bases
void launch_gen_exc_decode_w(const DecodeArgs& a, hipStream_t st);          // the same, a wave per block (models_w.hip); blocks [batch0, batch0 + nbatch), slot = workgroup
void launch_usr_decode_l(const DecodeArgs& a, hipStream_t st, u32 prefilled = 0);          // prefilled: launch_usr_fill has written the blocks without framing exceptions
void launch_usr_decode_w(const DecodeArgs& a, hipStream_t st, u32 prefilled);     // the same, a wave per block (decode_w.hip); blocks [batch0, batch0 + nbatch), slot = workgroup
void launch_usr_fill(const DecodeArgs& a, u64 r0, u64 r1, hipStream_t st);                          // block format: the records [r0, r1) of blocks whose four usr.* streams are empty
void launch_qlt_decode_l(const DecodeArgs& a, hipStream_t st);
void launch_gen_decode_l(const DecodeArgs& a, hipStream_t st);
void launch_rec_decode_l(const DecodeArgs& a, hipStream_t st);
// the same chains, a wavefront per block (decode_w.hip): blocks [batch0, batch0 + nbatch), slot = workgroup
void launch_qlt_decode_w(const DecodeArgs& a, hipStream_t st);
void launch_gen_decode_w(const DecodeArgs& a, hipStream_t st);          // (gen_bits >= 6)
void launch_rec_decode_w(const DecodeArgs& a, hipStream_t st);

// packing
void launch_block_stream_offsets(BlockDesc* blocks, u32 nblocks, u64* blk_stream_off, u64* stream_total, hipStream_t st);      // every stream of the call
void launch_compact(const BlockDesc* blocks, u32 nblocks, const u8* arena, const u64* blk_stream_off,
                    const u64* stream_base, u8* out, u32 skip_streams /* bit s: stream s is packed by launch_compact_chains */, hipStream_t st, const u32* gate);
void launch_stream_gate(const BlockDesc* blocks, u32 nblocks, const u64* stream_total, u64 out_cap, u64* stream_base /* [SFQ_NSTREAMS] */, u32* gate /* [2]: go, worst status */, hipStream_t st);
// records [r0, r1) -- a window of the call's blocks, or all of them; every per-record array is indexed by the call's record number
void launch_record_sizes(const DecodeArgs& a, u64 r0, u64 r1, u32* rsize, hipStream_t st);
void launch_assemble(const DecodeArgs& a, u64 r0, u64 r1, const u64* roff /* record r goes to out + roff[r] */, u8* out, hipStream_t st);
void launch_first_hdr_lens(const BlockDesc* blocks, u32 nblocks, u32* lens, hipStream_t st);
void launch_gather_first_hdrs(const BlockDesc* blocks, u32 nblocks, const u8* fq, const u64* blob_off, u8* blob, u64 cap, hipStream_t st);

// quality prior (prior.hip)
void launch_qlt_hist(const u8* fq, u64 nbytes, const u64* line_off, const BlockDesc* blocks, u32 block_reads, u64 nrec, u32 step,
                     int level, u32 cap /* symbols counted per sampled record */, u32* hist, hipStream_t st);
#define PRIOR_SYMBOLS 4096u
void launch_prior_rows(const u32* hist, u32 q_rows, u32* rows66, u32* w_rows, u32* w_ovf, u32* l_slots, RowHdr* l_hdr, hipStream_t st);
// the listed rows of rows66 back to back: slot[q_rows] scratch; list[4 + 67 n]: [0] = n, then per row its context and 66 words
void launch_prior_list(const u32* rows66, u32 q_rows, u32* slot, u32* list, hipStream_t st);
void launch_prior_scatter(const u32* ctxs, const u32* rows /* [n][66] */, u32 n, u32* rows66 /* zeroed */, hipStream_t st);
void launch_prior_spread(const u32* rows66, u32 q_rows, u32* w_rows, u32* w_ovf, u32* l_slots, RowHdr* l_hdr, hipStream_t st);

// CRC-32 of ranges of a device buffer (crc.hip): zlib.crc32 of [d + bounds[i], d + bounds[i+1]) into out[i], i < n_ranges, and with
// whole != 0 of [d + bounds[0], d + bounds[n_ranges]) into out[n_ranges].  lo / hi = bounds[0] / bounds[n_ranges] (non-decreasing
// bounds); tile_crc / grp_crc: scratch of crc_scratch_words(lo, hi, d) words; tab: crc_table_words() words from crc_build_tables.
struct CrcScratch { u64 ntiles = 0, ngroups = 0; };
CrcScratch crc_scratch_words(u64 lo, u64 hi, const u8* d);
u32  crc_table_words();
void crc_build_tables(u32* tab);
u32  crc32_combine_host(u32 crc_a, u32 crc_b, u64 len_b);
void launch_crc32(const u8* d, const u64* d_bounds, u32 n_ranges, u32 whole, u64 lo, u64 hi, u32* tile_crc, u32* grp_crc, u32* out,
                  const u32* tab, hipStream_t st);
// bounds[0..nblocks] of a call's blocks: 0, offs[b * stride] (0 < b < nblocks), total
void launch_crc_block_bounds(const u64* offs, u64 stride, u32 nblocks, u64 total, u64* bounds, hipStream_t st);

// The statistics of a text (stats.hip, sfq_text_stats): acc = text_stats_acc_bytes() zeroed bytes, which begin with the struct once
// the three kernels are through; line_off: the index of the text's 4 * nrec lines (line_off[4 * nrec] = n)
u64  text_stats_acc_bytes();
void launch_text_stats(const u8* fq, u64 n, const u64* line_off, u64 nrec, void* acc, hipStream_t st);

// Quality binning (qmap.hip): every byte of every 4th line of the text [d, d + n) through the 256-byte table d_lut, in place; the
// bytes whose value changed are added to *d_changed (zeroed by the caller).  scratch: qmap_scratch(d, n).bytes bytes, 16-byte
// aligned.  Reads the whole aligned 16-byte units of the text's first and last byte, writes nothing outside the text.
struct QmapScratch { u64 nspans = 0, cnt_off = 0, before_off = 0, tmp_off = 0, bytes = 0; };
QmapScratch qmap_scratch(const u8* d, u64 n);
void launch_quality_map(u8* d, u64 n, const u8* d_lut, u8* scratch, u64* d_changed, hipStream_t st);
// its first step alone: the '\n' bytes of every span of [d, d + n) into cnt[qmap_scratch(d, n).nspans]
void launch_newline_counts(const u8* d, u64 n, u32* cnt, hipStream_t st);

// Paired files (pair.hip): two texts record by record into one (A0 B0 A1 B1 ...), and such a text back into its even records followed
// by its odd ones.  Both passes find the records themselves -- the line ends per span, their scan, then the offset of every fourth
// line end -- check what they found and copy only where it holds: *info tells the host, which synchronises once.
enum PairStatus : u32 {
    PAIR_OK = 0,
    PAIR_LINES_A,           // the (first) text's lines are no multiple of four
    PAIR_LINES_B,
    PAIR_COUNTS,            // A and B hold different record counts
    PAIR_A_END,             // A does not end in '\n'
    PAIR_ODD,               // an odd number of records to split
    PAIR_LONG,              // a record of 4 GiB or more
    PAIR_CAP,               // more records than the start arrays hold: info->recs says how many, nothing else was done
    PAIR_RANGE,             // a window of records that ends behind the text's last record
    PAIR_ROOM               // a window's records need more than the output holds: info->nout says how much
};
// pieces, win0, nout: what k_pair_check found the copy to be -- P of its 2 P pieces, the source offset of a split's first record, the
// output's bytes (known to the host unless a window is cut).  mm_*: the name pass (k_pair_names), untouched where it does not run.
struct PairInfo { u64 lines[2], recs[2], split; u32 status, pad; u64 pieces, win0, nout; u64 mm_count, mm_first, mm_off[2]; };
// a text and what the passes over it need: scratch = qmap_scratch(d, n).bytes bytes, 16-byte aligned; starts: cap + 1 entries
struct PairText { const u8* d; u64 n; u8* scratch; u64* starts; };
// a split's window: records [r0, r0 + nr) alone, nr even and > 0, into an output of out_cap bytes; on = 0: the whole text
struct PairWindow { u32 on, pad; u64 r0, nr, out_cap; };
// info: zeroed by the caller.  out: a.n + b.n bytes; nothing outside them is written, and nothing at all unless info->status stays 0.
// names: k_pair_names runs between the check and the copy (the copy does not wait for what it finds: info->mm_count tells the host)
void launch_pair_interleave(const PairText& a, const PairText& b, u64 cap /* records a start array holds */, bool names, u8* out, PairInfo* info, hipStream_t st);
// out: t.n bytes (a window: info->nout, at most win.out_cap), the even records then (from info->split on) the odd ones; lens[cap / 2 + 1],
// offa[cap / 2 + 2], scan_tmp as launch_scan_u32 wants it for cap / 2 + 1
void launch_pair_split(const PairText& t, u64 cap, const PairWindow& win, u32* lens, u64* offa, u64* scan_tmp, u8* out, PairInfo* info, hipStream_t st);
// the record starts, the rules and the name pass, no copy: b.d null = t is interleaved (record 2k against 2k + 1, a split's rules),
// else record i of a against record i of b (an interleave's rules).  Writes info alone.
void launch_pair_names(const PairText& a, const PairText& b, u64 cap, PairInfo* info, hipStream_t st);

// Picked lines (pick.hip): of every record of a text one contiguous piece -- lines 1 and 2 with a '>' in front, the name, the base line
// or the quality line -- the pieces of records [r0, r0 + nr) one behind the other.  Like pair.hip the pass finds the lines itself,
// checks what it found and copies only where it holds: *info tells the host, which synchronises once.
enum PickWhat : u32 { PICK_FASTA = 1, PICK_NAMES = 2, PICK_BASES = 3, PICK_QUALS = 4 };      // SFQ_PICK_*
enum PickStatus : u32 {
    PICK_OK = 0,
    PICK_LINES,             // the text's lines are no multiple of four
    PICK_RANGE,             // records that end behind the text's last record
    PICK_CAP,               // more records than the arrays hold: info->recs says how many, nothing else was done
    PICK_LONG,              // a piece of 4 GiB or more
    PICK_AT,                // FASTA, NAMES: a record of the range does not begin with '@': info->bad_first (the smallest), info->bad_off
    PICK_ROOM               // the pieces need more than the output holds: info->nout says how much
};
// r0, pieces: the range as the check found it; nout: the result's bytes; mark_off: where piece job.mark went (nout behind the last)
struct PickInfo { u64 lines, recs; u32 status, pad; u64 r0, pieces, nout, mark_off, bad_first, bad_off; };
// Record r's piece is text[from[r], to[r]): from[r] = where line fl of the record begins, plus skip; to[r] = where line tl of the
// record begins (tl = 4: the next record, or the text's end).  cap entries each.
struct PickLines { u64* from; u64* to; u64 cap; u32 fl, tl, skip; };
// nr = ~0: to the text's last record; mark: a piece of the range, counted from r0
struct PickJob { u32 what, pad; u64 r0, nr, out_cap, mark; };
// t.starts: from[cap]; to[cap]; lens[nlens], dst[nlens + 1], scan_tmp as launch_scan_u32 wants it for nlens, where nlens = min(nr, cap);
// info: zeroed by the caller.  out: job.out_cap bytes, of which info->nout are written, and none unless info->status stays 0.
void launch_pick(const PairText& t, u64* to, u64 cap, const PickJob& job, u32* lens, u64* dst, u64* scan_tmp, u64 nlens, u8* out, PickInfo* info, hipStream_t st);
// its copy alone, for the passes whose pieces are whole records (sel.hip): P = info->pieces pieces, piece k = text[from[info->r0 + k] ..) to
// out + dst[k], dst[P] = info->nout; bound: what the output can hold at most (the grid).  Nothing runs where info->status is set.
void launch_pick_copy(const u64* dst, const u64* from, const u8* text, u64 bound, u8* out, PickInfo* info, hipStream_t st);
// the same into out + *shift, where only the device knows where the pieces' part of a result begins (mrg.hip)
void launch_pick_copy_at(const u64* dst, const u64* from, const u8* text, u64 bound, u8* out, const u64* shift, PickInfo* info, hipStream_t st);

// Selected records (sel.hip): the records of [r0, r0 + nr) that pass a filter on their content -- the base line's length, its N count,
// the quality line's mean, a motif in the base line -- and a reproducible sample, whole and in order.  Like pick.hip the pass finds the
// lines itself, decides every refusal on the device and copies with pick.hip's copy; *info tells the host, which synchronises once.
enum SelStatus : u32 {
    SEL_OK = 0,
    SEL_LINES,              // the text's lines are no multiple of four
    SEL_RANGE,              // records that end behind the text's last record
    SEL_CAP,                // more records than the arrays hold: info->recs says how many, nothing else was done
    SEL_LONG,               // a record of 4 GiB or more
    SEL_ODD,                // pairs: an odd number of records in the range
    SEL_ROOM                // the kept records need more than the output holds: info->copy.nout says how much
};
// copy: what k_pick_copy reads -- r0 = 0, pieces = the records kept, nout = their bytes, status != 0 wherever there is nothing to copy
// (a refusal, or no record kept: SEL_NOTHING there while status stays SEL_OK).  r0, nr: the range as the check found it.
constexpr u32 SEL_NOTHING = 0x100;
struct SelInfo { PickInfo copy; u64 lines, recs, r0, nr; u32 status, pad; u64 n_fail[4]; };
// the rule (slimfastq_amd.h sfq_select); motif, motif_rev: two bits a base, (byte >> 1) & 3, the first base in the lowest bits
// (motif_rev = motif where the reverse complement does not count); nr = ~0: to the text's last record
struct SelJob {
    u64 r0, nr, out_cap;
    u32 min_len, max_len, max_n, min_q, qual_base, motif_len, invert, pairs, sample, pad;
    u64 seed, index_base, motif, motif_rev;
};
// ls[4 cap + 1]: where every line begins (ls[lines] = the text's end, one more where its last line has no '\n': a line's length is
// ls[l + 1] - ls[l] - 1 throughout); acc[2 cap]: per base line its N count, per quality line its byte sum; hit[cap]: the motif occurs;
// keep, rlen, lens, from: nlens entries, pos, dst: nlens + 1, tmp as launch_scan_u32 wants it for nlens; nlens = min(nr, cap)
struct SelArrays { u64* ls; u64* acc; u8* hit; u32* keep; u32* rlen; u64* pos; u32* lens; u64* from; u64* dst; u64* tmp; u64 cap, nlens; };
// t.starts is not used (A.ls is the pass's own); info: zeroed by the caller.  out: job.out_cap bytes, of which info->copy.nout are
// written, and none unless info->status and info->copy.status stay 0.
void launch_select(const PairText& t, const SelArrays& A, const SelJob& job, u8* out, SelInfo* info, hipStream_t st);
// its first two steps alone, for the passes that want the starts of ALL lines (trim.hip): t.scratch's line-end counts and their scan
// (before[] = the line ends in front of every span, before[nspans] = all of them), then ls[l] = where line l begins for every l in
// 1 .. lcap that a line end in the text gives; ls[0] and the entry behind the last line are the caller's check's.
void launch_line_starts(const PairText& t, u64* ls, u64 lcap, hipStream_t st);

// Trimmed records (trim.hip): every record of a text with bytes [s, e) of its lines 2 and 4 alone, where s and e come from crops, quality
// cuts and an adapter (slimfastq_amd.h "trimmed records").  Like sel.hip the pass finds the lines itself, decides every refusal on the
// device and copies with pick.hip's copy; *info tells the host, which synchronises once.
enum TrimStatus : u32 {
    TRIM_OK = 0,
    TRIM_LINES,             // the text's lines are no multiple of four
    TRIM_CAP,               // more records than the arrays hold: info->recs says how many, nothing else was done
    TRIM_ROOM               // the result needs more than the output holds: info->copy.nout says how much
};
// copy: what k_pick_copy reads -- r0 = 0, pieces = the non-empty pieces of all records, nout = their bytes, status != 0 wherever there
// is nothing to copy.  stop: some refusal, whichever kernel found it; bad_first, bad_off: the smallest record whose lines 2 and 4 differ
// in length (~0: none) and where it begins; toolong: a line (or a piece of the copy) of 4 GiB or more.
struct TrimInfo {
    PickInfo copy; u64 lines, recs; u32 status, stop, toolong, pad; u64 bad_first, bad_off;
    u64 n_changed, n_emptied, bases_in, bases_out, n_cut[4];
};
// the rule, made ready by the host: lead_thr, trail_thr = the smallest BYTE that satisfies the quality cut (0: the term is off, above
// 255: no byte does); win_sum: a window fails where its byte sum is below it; adapter: two bits a base, (byte >> 1) & 3, the first base
// in the lowest bits; ad_len = 0: no adapter
struct TrimJob {
    u64 out_cap, adapter;
    u32 head, tail, max_len, lead_thr, trail_thr, win_len, win_sum, ad_len, ad_mm, ad_min;
};
// ls[4 cap + 1] as SelArrays'; lead, trail, win, ad[cap]: per record the terms' positions (trail as the complement of the cut, so that
// all four are minima; all ones = none); se[cap]: s | e << 32; cnt[cap]: the record's non-empty pieces, at[cap + 1] their scan;
// rlen[cap]: the bytes left of the record, rdst[cap + 1] their scan; from[5 cap], dst[5 cap]: the pieces' sources and destinations;
// tmp as launch_scan_u32 wants it for cap
struct TrimArrays { u64* ls; u32* lead; u32* trail; u32* win; u32* ad; u64* se; u32* cnt; u64* at; u32* rlen; u64* rdst; u64* from; u64* dst; u64* tmp; u64 cap; };
// t.starts is not used; info: zeroed by the caller.  out: job.out_cap bytes, of which info->copy.nout are written, and none unless
// info->stop stays 0.
void launch_trim(const PairText& t, const TrimArrays& A, const TrimJob& job, u8* out, TrimInfo* info, hipStream_t st);

// Overlapping mates (ovl.hip): for every pair of a range of records the offset at which the first mate and the reverse complement of
// the second agree (slimfastq_amd.h "overlapping mates"), the insert sizes' histogram, and with job.cut the text with what lies behind
// the insert cut off lines 2 and 4 of both mates.  Like trim.hip the pass finds the lines itself, decides every refusal on the device and
// copies with pick.hip's copy; *info tells the host, which synchronises once.
constexpr u32 OVL_MAX_LEN = 512;            // SFQ_OVERLAP_MAX_LEN
constexpr u32 OVL_SKIPPED = 0xFFFFFFFFu;    // ins[]: a pair with a mate above OVL_MAX_LEN
enum OvlStatus : u32 {
    OVL_OK = 0,
    OVL_LINES,              // the text's lines are no multiple of four
    OVL_RANGE,              // a range that ends behind the text's last record
    OVL_ODD,                // an odd number of records in the range
    OVL_CAP,                // more records than the arrays hold: info->recs says how many, nothing else was done
    OVL_ROOM                // the result needs more than the output holds: info->copy.nout says how much
};
// copy, stop, bad_first, bad_off, toolong: as TrimInfo's (bad_first among the range's records alone); r0, nr: the range as the check
// found it; hist[I]: the searched pairs whose insert is I, hist[0]: those without an accepted offset
struct OvlInfo {
    PickInfo copy; u64 lines, recs, r0, nr; u32 status, stop, toolong, pad; u64 bad_first, bad_off;
    u64 n_pairs, n_skipped, n_overlap, n_cut, bases_in, bases_out, mismatches;
    u64 hist[2 * OVL_MAX_LEN + 1];
};
// nr = ~0: to the text's last record; cut = 0: the searches and the counts alone, no copy (out is not touched)
struct OvlJob { u64 r0, nr, out_cap; u32 min_ov, max_mm, max_pct, cut; };
// ls[4 cap + 1] as SelArrays'; ins, mm[cap / 2 + 1]: per pair of the range its insert (0: no offset accepted, OVL_SKIPPED) and the
// winner's mismatches; keep[cap]: what is left of the record's lines 2 and 4; cnt, at, rlen, rdst, tmp as TrimArrays';
// from[3 cap], dst[3 cap]: the pieces' sources and destinations (a cut that begins at 0 leaves a record at most three pieces)
struct OvlArrays { u64* ls; u32* ins; u32* mm; u32* keep; u32* cnt; u64* at; u32* rlen; u64* rdst; u64* from; u64* dst; u64* tmp; u64 cap; };
// t.starts is not used; info: zeroed by the caller.  out: job.out_cap bytes, of which info->copy.nout are written, and none unless
// info->stop stays 0 and job.cut is set.
void launch_overlap(const PairText& t, const OvlArrays& A, const OvlJob& job, u8* out, OvlInfo* info, hipStream_t st);
// its steps in front of the cut alone, for the passes that want the winners (mrg.hip): the line starts, the rules (info->status, stop,
// bad_first, bad_off, toolong, r0, nr) and the search.  Of A it uses ls, ins, mm and cap.
void launch_overlap_search(const PairText& t, const OvlArrays& A, const OvlJob& job, OvlInfo* info, hipStream_t st);

// Merged mates (mrg.hip): every pair of a range of records that has an accepted offset as ONE record -- consensus bases, combined
// qualities (slimfastq_amd.h "merged mates") -- then the range's other pairs whole.  The search is ovl.hip's; the merged records are
// computed and written by k_mrg_write, the others copied with pick.hip's copy.  *info tells the host, which synchronises once.
// o: the search's (status OVL_*, stop, bad_first, toolong; n_pairs, n_skipped, bases_in, mismatches, hist as the report's; copy: the
// piece copy of the unmerged part, copy.status != 0 wherever there is nothing to copy); merged_bytes: where that part begins;
// out_bytes: the whole result, on OVL_ROOM the size needed
constexpr u32 MRG_NOTHING = 0x100;
struct MrgInfo { OvlInfo o; u64 merged_bytes, out_bytes, n_merged, bases_merged, n_x_wins, n_y_wins; };
struct MrgJob { u64 r0, nr, out_cap; u32 min_ov, max_mm, max_pct, qual_base; };
// ls, ins, mm as OvlArrays'.  Per pair of the range, P = cap / 2 + 1 entries (the scans' results one more): mlen, mdst: the merged
// record's bytes (0: the pair does not merge) and where it goes; ulen, udst: the unmerged pair's bytes and where they go, counted from
// merged_bytes; flag, mpos: 1 where the pair merges, and the merged pairs in front of it; list: the merged pairs; from, dst: the
// unmerged pairs' pieces; tmp as launch_scan_u32 wants it for P
struct MrgArrays { u64* ls; u32* ins; u32* mm; u32* mlen; u64* mdst; u32* ulen; u64* udst; u32* flag; u64* mpos; u64* list; u64* from; u64* dst; u64* tmp; u64 cap; };
// t.starts is not used; info: zeroed by the caller.  out: job.out_cap bytes, of which info->out_bytes are written, and none unless
// info->o.stop stays 0.
void launch_merge(const PairText& t, const MrgArrays& A, const MrgJob& job, u8* out, MrgInfo* info, hipStream_t st);

// Distinct records (dd.hip): the units (records; under pairs, pairs) of [r0, r0 + nr) whose key -- line 2 with 'a'..'z' folded, under
// pairs both mates' in order -- no earlier unit of the range has and, with a set, no unit an earlier call kept; whole and in order.
// Like sel.hip the pass finds the lines itself, decides every refusal on the device and copies with pick.hip's copy.
enum DdStatus : u32 {
    DD_OK = 0,
    DD_LINES,               // the text's lines are no multiple of four
    DD_RANGE,               // records that end behind the text's last record
    DD_CAP,                 // more records than the arrays hold: info->recs says how many, nothing else was done
    DD_LONG,                // a record of 4 GiB or more, or a pair whose keys hold as much together
    DD_ODD,                 // pairs: an odd number of records in the range
    DD_ROOM,                // the kept records need more than the output holds: info->copy.nout says how much
    DD_NOMEM,               // the set has no room for the new keys: info->new_keys, new_bytes say what the call adds
    DD_PROBE                // a probe sequence found no slot (cannot be: a table holds twice its keys)
};
constexpr u32 DD_NOTHING = 0x100;                              // copy.status where no unit is kept (status stays DD_OK), as SEL_NOTHING
// copy: what k_pick_copy reads, as SelInfo's.  units: the range's; tmask: the call's table's slots - 1; new_keys, new_bytes: the kept
// units and (with a set) their keys' bytes
struct DdInfo { PickInfo copy; u64 lines, recs, r0, nr; u32 status, pad; u64 units, tmask, n_dup_set, n_dup_call, new_keys, new_bytes; };
struct DdJob { u64 r0, nr, out_cap; u32 pairs, use_set; };
// The set of a context, on the device: slots[smask + 1] (a power of two of at least 2 max_keys): 0, or bit 63 | a 23-bit fingerprint of
// the key's hash | the key's number k; koff[k]: where key k begins in the arena, klen[k] (pairs: klen[2 k], klen[2 k + 1]): its
// lines' lengths, one behind the other there; arena: max_bytes bytes (allocated to a multiple of 16).  keys, bytes: what it holds
// BEFORE the call -- the host keeps the counts and adds info->new_keys, new_bytes after a call that succeeds.
struct DdSetDev { u64* slots; u64 smask; u64* koff; u32* klen; u8* arena; u64 max_keys, max_bytes, keys, bytes; };
// ls[4 cap + 1] as SelArrays'; per unit, ucap = (nlens + G - 1) / G entries (G = 2 under pairs): hash, slot (the unit's slot in the
// call's table), inset (the key is in the set; written for the earliest unit of a key alone), kb (the key bytes a kept unit adds),
// koffs[ucap + 1] their scan; table[tcap]: the call's table, tcap a power of two of at least 2 ucap; keep, rlen, lens, from: nlens
// entries, pos, dst: nlens + 1, tmp as launch_scan_u32 wants it for nlens; nlens = min(nr, cap)
struct DdArrays {
    u64* ls; u64* hash; u64* slot; u8* inset; u32* kb; u64* koffs; u64* table; u32* keep; u32* rlen; u64* pos; u32* lens; u64* from; u64* dst; u64* tmp;
    u64 cap, nlens, ucap, tcap;
};
// t.starts is not used; info: zeroed by the caller; S: all zero without job.use_set.  out: job.out_cap bytes, of which info->copy.nout
// are written, and none unless info->status and info->copy.status stay 0.  The set is written only where info->status stays 0.
void launch_dedup(const PairText& t, const DdArrays& A, const DdJob& job, const DdSetDev& S, u8* out, DdInfo* info, hipStream_t st);

// Screened records (scr.hip): the units (records; under pairs, pairs) of [r0, r0 + nr) whose line 2 shares enough k-mers with a set of
// reference k-mers -- or, with keep_matched, only those.  A k-mer's canonical value (the smaller of its 2-bit value and its reverse
// complement's) is what the set holds, whole: membership is exact.  Like dd.hip the pass finds the lines itself, decides every refusal
// on the device and copies with pick.hip's copy; the set is only read.
enum ScrStatus : u32 {
    SCR_OK = 0,
    SCR_LINES,              // the text's lines are no multiple of four
    SCR_RANGE,              // records that end behind the text's last record
    SCR_CAP,                // more records than the arrays hold: info->recs says how many, nothing else was done
    SCR_LONG,               // a record of 4 GiB or more
    SCR_ODD,                // pairs: an odd number of records in the range
    SCR_ROOM                // the kept records need more than the output holds: info->copy.nout says how much
};
constexpr u32 SCR_NOTHING = 0x100;                             // copy.status where no unit is kept (status stays SCR_OK), as SEL_NOTHING
constexpr u64 SCR_OCC = 1ull << 63;                            // a slot: 0 (empty) or SCR_OCC | the canonical value (k <= 31: below 2^62)
// the set on the device: slots[smask + 1], a power of two of at least 2 max_kmers; a k-mer's home slot is the top bits of
// canonical * 0x9E3779B97F4A7C15, that is the product >> shift with shift = 64 - log2(slots); probing is linear from there
struct ScrSetDev { u64* slots; u64 smask; u32 k, shift; };
// copy: what k_pick_copy reads, as SelInfo's.  units, kept: the range's and the kept ones; matched, windows, hits: sums over the range's records
struct ScrInfo { PickInfo copy; u64 lines, recs, r0, nr; u32 status, pad; u64 units, kept, matched, windows, hits; };
struct ScrJob { u64 r0, nr, out_cap; u32 pairs, min_hits, min_pct, keep_matched; };
// ls[4 cap + 1] as SelArrays'; hits, wins: H and W per record of the range; keep, rlen, lens, from: nlens entries, pos, dst: nlens + 1,
// tmp as launch_scan_u32 wants it for nlens; nlens = min(nr, cap)
struct ScrArrays { u64* ls; u32* hits; u32* wins; u32* keep; u32* rlen; u64* pos; u32* lens; u64* from; u64* dst; u64* tmp; u64 cap, nlens; };
// what sfq_screen_set_add reads back: kmers = the slots claimed since the set was emptied; full: a probe sequence found no empty slot
struct ScrAddInfo { u64 kmers; u32 full, pad; };
// the windows of the sequence text seq[0, n) (device memory) into the set; max_kmers: where the lanes stop inserting (the host refuses
// the call and empties the set).  info is NOT zeroed by the caller between the adds of one set: kmers runs on.
void launch_screen_add(const u8* seq, u64 n, const ScrSetDev& S, u64 max_kmers, ScrAddInfo* info, hipStream_t st);
// lanes: the lanes that share a record in k_scr_count, 8 unless a measurement asks for 1, 4 or 16 (profiles/screen_pass.py).
// t.starts is not used; info: zeroed by the caller.  out: job.out_cap bytes, of which info->copy.nout are written, and none unless
// info->status and info->copy.status stay 0.  The set is never written.
void launch_screen(const PairText& t, const ScrArrays& A, const ScrJob& job, const ScrSetDev& S, u32 lanes, u8* out, ScrInfo* info, hipStream_t st);

// Demultiplexed records (dmx.hip): the units (records; under pairs, pairs) of [r0, r0 + nr) sorted STABLY into NP parts by the sample
// whose barcode the unit's observed bytes match (slimfastq_amd.h "demultiplexed records"), the parts back to back.  Like dd.hip the
// pass finds the lines itself, decides every refusal on the device and copies with pick.hip's copy; what is new is the classifier and
// the stable multi-way partition, an LSD radix sort of the records by class over digits of 8 bits.
enum DmxStatus : u32 {
    DMX_OK = 0,
    DMX_LINES,              // the text's lines are no multiple of four
    DMX_END,                // the text does not end in '\n'
    DMX_RANGE,              // records that end behind the text's last record
    DMX_ODD,                // pairs: an odd number of records in the range
    DMX_CAP,                // more records than the arrays hold: info->recs says how many, nothing else was done
    DMX_LONG,               // a record of 4 GiB or more
    DMX_CLIP,               // clip: a record of the range whose lines 2 and 4 differ in length: info->bad_first, bad_off
    DMX_ROOM                // the parts need more than the output holds: info->copy.nout says how much
};
constexpr u32 DMX_TILE = 1024;                                 // records a workgroup ranks in one digit pass
constexpr u32 DMX_MAX_SAMPLES = 4096;
struct DmxPart { u32 src, mate, sub, pos, len; };              // sfq_demux_part
// copy: what k_pick_copy reads, as SelInfo's.  units: the range's; the verdicts' counts; bad_first: the smallest record the clip refuses
struct DmxInfo { PickInfo copy; u64 lines, recs, r0, nr; u32 status, pad; u64 units, n_assigned, n_perfect, n_short, n_far, n_ambiguous, bad_first, bad_off; };
// np: the parts, n_samples + 1 or twice that with split; clip0, clip1: what an assigned unit's mate 0 and mate 1 lose in front (0 without clip)
struct DmxJob { u64 r0, nr, out_cap; u32 pairs, split, max_mm, clip, n_samples, np, clip0, clip1; DmxPart part[2]; };
// ls[4 cap + 1] as SelArrays'; codes[n_samples]: the barcodes, two bits a base ((byte >> 1) & 3), base i in bits 2 i, 2 i + 1; cls[nlens]:
// the class of every record of the range; ord_a, ord_b[nlens]: the records (counted from r0) sorted by the class's low digit, by the
// class; hist[256 ntiles], hoff one more: the digit counts of every tile, DIGIT-major, and their scan; cnt[nlens], at[nlens + 1] (clip
// alone): the pieces of the record at every sorted position and their scan; lens, from: pcap entries (pcap = nlens, with clip 3 nlens),
// dst one more; tmp as launch_scan_u32 wants it for max(pcap, 256 ntiles); bounds[2 (np + 1)]: part_off[np + 1], then for every
// part the sorted position of its first record (np + 1 entries, the last = nr); ntiles = ceil(nlens / DMX_TILE), nlens = min(nr, cap)
struct DmxArrays {
    u64* ls; const u64* codes; u32* cls; u64* ord_a; u64* ord_b; u32* hist; u64* hoff; u32* cnt; u64* at; u32* lens; u64* from; u64* dst; u64* tmp; u64* bounds;
    u64 cap, nlens, ucap, ntiles, pcap;
};
// t.starts is not used; info: zeroed by the caller.  out: job.out_cap bytes, of which info->copy.nout are written, and none unless
// info->status and info->copy.status stay 0.
void launch_demux(const PairText& t, const DmxArrays& A, const DmxJob& job, u8* out, DmxInfo* info, hipStream_t st);

// BGZF members (bgz.hip): member m of n_members holds text[mb[m], mb[m + 1]), 1 .. 65280 bytes; crc[m]: its CRC-32 (crc.hip's range
// pass over the same bounds).  A wavefront deflates a member into slot m of slots (bgz_slot_bytes), through the workgroup's piece of
// toks (bgz_token_bytes(workgroups)); msize[m] = the member's bytes, dst[n_members + 1] their scan (scan_tmp as launch_scan_u32 wants
// it), from[m] = where the member lies in slots; *n_stored (zeroed by the caller) counts the members that hold a stored block.  Then
// pick.hip's copy packs the members into out: info (zeroed by the caller) ends up with pieces = n_members, nout = their bytes and
// status = PICK_ROOM where they exceed out_cap -- nothing is written to out then.
u32  bgz_workgroups(u32 n_members, u32 cus);
u64  bgz_token_bytes(u32 workgroups);
u64  bgz_slot_bytes(u32 n_members);
void launch_bgz_deflate(const u8* text, const u64* mb, u32 n_members, const u32* crc, u32 workgroups, u32* toks, u8* slots, u32* msize, u64* from,
                        u64* dst, u64* scan_tmp, u32* n_stored, u64 out_cap, u8* out, PickInfo* info, hipStream_t st);

/*
 * slimfastq_amd.h -- C ABI of the MI355X-native slimfastq hot path.
 *
 * This is the drop-in boundary: everything the reference does between `UsrSave::encode()` /
 * `UsrLoad::decode()` (usrs.cpp:392-407 / 539-574) and `FilerSave::put()` / `FilerLoad::get()`
 * (filer.hpp:70-75, 94-97) -- i.e. the stream models qlts.cpp / gens.cpp / recs.cpp, the rangers
 * (base2_ranger.hpp, log64_ranger.hpp, power_ranger.hpp), the range coder (coder.hpp) and the
 * exception side streams (xfile.cpp) -- runs behind these entry points as hand-written gfx950 HIP
 * kernels.  The reference has no FFI of its own; each entry point names the C++ call it replaces.
 *
 * Conventions: extern "C", plain pointers and sizes, int status (0 = ok, <0 = error, never exit(),
 * no exceptions across the boundary).  The caller owns every buffer it passes; the context owns
 * device tables, scratch and its HIP stream.  One context per host thread per GPU; calls on
 * different contexts are concurrent-safe.  Pointers named d_* are DEVICE pointers, h_* are host
 * pointers.  There is no CPU fallback: without a HIP device sfq_ctx_create fails.
 */
#ifndef SLIMFASTQ_AMD_H
#define SLIMFASTQ_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFQ_ABI_VERSION 3

/* status codes */
#define SFQ_OK              0
#define SFQ_E_ARG          -1   /* bad argument                                              */
#define SFQ_E_HIP          -2   /* HIP runtime error / no device                             */
#define SFQ_E_NOMEM        -3   /* device or host allocation failed                          */
#define SFQ_E_FORMAT       -4   /* input is not 4-line FASTQ (reference: croak, usrs.cpp:162-172) */
#define SFQ_E_OVERFLOW     -5   /* an output arena was too small                             */
#define SFQ_E_CORRUPT      -6   /* compressed stream inconsistent                            */
#define SFQ_E_UNSUPPORTED  -7   /* e.g. the block format and a '+' line that is neither empty nor the record's header (the reference
                                   would silently replace it, usrs.cpp:236-239 / 518-523)                                       */
#define SFQ_E_GENCHAR      -8   /* unexpected genome char (gens.cpp:125-126) / switched N byte (gens.cpp:107-108) */

/* Stream ids: the reference's stream names (FilerSave(name) call sites). */
enum sfq_stream {
    SFQ_S_REC = 0,      /* "rec"     recs.cpp:40      */
    SFQ_S_GEN = 1,      /* "gen"     gens.cpp:63      */
    SFQ_S_QLT = 2,      /* "qlt"     qlts.cpp:46      */
    SFQ_S_GEN_NS = 3,   /* "gen.Ns"  gens.cpp:69      */
    SFQ_S_GEN_NN = 4,   /* "gen.Nn"  gens.cpp:70      */
    SFQ_S_REC_X = 5,    /* "rec.x"   recs.cpp:44      */
    SFQ_S_USR_X = 6,    /* "usr.x"   usrs.cpp:48      */
    SFQ_S_USR_XQ = 7,   /* "usr.x.q" usrs.cpp:49      */
    SFQ_S_USR_PFG = 8,  /* "usr.pfg" usrs.cpp:50      */
    SFQ_S_USR_PFQ = 9,  /* "usr.pfq" usrs.cpp:51      */
    SFQ_S_GEN_LC = 10,  /* "gen.lc"  block format only: positions of the lowercase bases (the reference accepts them,
                           gens.cpp:73-77, and gives them back uppercase, gens.cpp:171-178), gap-coded like "gen.Ns"     */
    SFQ_S_USR_LREC = 11,/* "usr.lrec" usrs.cpp:55: oversize records -- gap, header line, '+' line, raw            */
    SFQ_S_USR_LGEN = 12,/* "usr.lgen" usrs.cpp:53: their base lines                                              */
    SFQ_S_USR_LQLT = 13,/* "usr.lqlt" usrs.cpp:54: their quality lines                                           */
    SFQ_NSTREAMS = 14
};
const char* sfq_stream_name(int stream);

/* Which models to run (config C2 of BASELINE.json runs SFQ_M_QLT alone). */
#define SFQ_M_REC 1u
#define SFQ_M_GEN 2u
#define SFQ_M_QLT 4u
#define SFQ_M_USR 8u
#define SFQ_M_ALL 15u

typedef struct sfq_ctx sfq_ctx;

typedef struct sfq_params {
    int32_t  level;        /* 1..4 : conf.level (config.cpp:260-263, clamped like config.cpp:232-237) */
    uint32_t block_reads;  /* records per independent block; 0 = a single block, i.e. streams that are
                              byte-identical to the reference's own (format 6), its quirks included: lowercase bases
                              come back uppercase, an emptied header field comes back "0" (SURVEY H7);
                              SFQ_BLOCK_AUTO = about 376 KiB of text per block (1024 records of 150 bp, a handful of
                              long reads).  The block format is LOSSLESS: where the reference would alter the text,
                              its blocks depart from the reference's bytes (a header field that would not print back
                              is coded as a string, lowercase bases are listed in "gen.lc") or refuse the input    */
    int32_t  gen_bits;     /* base-model context bits; 0 = the level's (gens.hpp:43-53) capped by block size.  (The table they size is
                              the adaptive modes' and kernel = 2's; the default frozen mode's match model has no table of rows) */
    uint32_t models;       /* SFQ_M_* mask; 0 = SFQ_M_ALL                                             */
    uint32_t kernel;       /* 0 = default kernels; 1 = lane-per-block reference kernels (the reference loop on one lane:
                              slow, the cross-check of the default kernels; adaptive tables); 2 = the default kernels, but
                              with frozen tables the base exceptions (gen.Ns / gen.Nn / gen.lc) keep the reference's own
                              coding -- XFile streams through adaptive PowerRanger rows, what archives written before
                              round 4 hold -- instead of Rice-coded gap lists ("chn.idx" flag CHN_EXC_RICE -- csrc/kernels.h ChnFlag --), and the
                              BASES keep round 4's coding: generation tables of Base2 rows where they pay, the initial row's 3 of 12
                              a base where they do not -- instead of the generation match model ("chn.idx" flag CHN_GEN_MATCH: a chain
                              follows a pointer into the earlier generations' bases, gm.hip) and, where they have nothing to learn, two bits a
                              base without a coder (CHN_FLAT_RAW, block format 10)   */
    uint32_t version;      /* decode only: archive "version" info key (config.cpp:373); 0 = current (6).
                              Versions < 5 take RecLoad::load_pre5 (recs.cpp:400-401)                      */
    uint32_t prior_step;   /* encode, block mode only: 0 = cold blocks (each block == the reference run on that block);
                              N > 0 = warm start: quality rows start from a prior counted over every N-th record
                              (its first 4096 quality symbols)
                              (SFQ_PRIOR_AUTO picks N from the input size; frozen tables always have a prior)       */
    uint32_t tables;       /* block mode only: SFQ_TABLES_ADAPTIVE (0) = every block runs the reference's adaptive rows
                              (Log64Ranger / Base2Ranger updated per symbol), a wavefront per block;
                              SFQ_TABLES_FROZEN (1) = the rows are built by counting passes and frozen while a chain
                              is coded -- qualities from the transmitted prior, bases from the counts of the earlier
                              generations of the same call (round 5: read as such -- the match model, DESIGN.md 4.3 --, not
                              counted into a table) -- one chain per LANE                              */
    uint32_t chain_reads;  /* frozen tables: records per chain; 0 = automatic (about 262 144 chains a call -- csrc/api.cpp SFQ_CHAINS_WANT --, of 4 KiB of text or more; long
                              reads -- fewer than 204 800 records, each a chain's worth or more -- are cut into SEGMENTS of one record);
                              SFQ_CHAIN_SEGMENT(n): chains of (at most) n quality symbols / bases of ONE record                     */
    uint32_t lds_rows;     /* frozen tables: quality rows staged in LDS by every workgroup of the quality chains.  Encode: the N most used
                              rows (up to 1024); 0 = automatic (800 rows where the call has 150 000 chains or more: 17.3 -> 15.9 ms per 3.7 GB
                              call), SFQ_LDS_ROWS_NONE = none.  Decode: the coarse lists (16 bytes) of the N contexts the prior gives the most
                              weight (up to 6000); 0 = automatic (6000 where the call has 150 000 chains or more: 23.0 -> 20.0 ms),
                              SFQ_LDS_ROWS_NONE = none.  Where the rows come from never shows in the streams.                          */
} sfq_params;
#define SFQ_CHAIN_SEGMENT_FLAG 0x80000000u
#define SFQ_CHAIN_SEGMENT(n) (SFQ_CHAIN_SEGMENT_FLAG | (uint32_t)(n))
#define SFQ_TABLES_ADAPTIVE 0u
#define SFQ_TABLES_FROZEN   1u
#define SFQ_TABLES_AUTO     2u   /* by the size of the text: frozen tables from 64 MiB on; below that their transmitted priors weigh too
                                    much (samples/tst7.fq, 3.9 MB: 1.15 x the reference's bytes) and a GPU has nothing to win on so
                                    little text -- adaptive tables in blocks of 65536 records (SFQ_BLOCK_AUTO), i.e. the reference's
                                    own streams for a file of up to that many records */
#define SFQ_LDS_ROWS_NONE  0xFFFFFFFFu
#define SFQ_PRIOR_AUTO  0xFFFFFFFFu
#define SFQ_PRIOR_GIVEN 0xFFFFFFFEu  /* prior_step: the priors installed with sfq_set_qlt_prior / sfq_set_rec_prior */
#define SFQ_PRIOR_COUNTS 0xFFFFFFFDu /* prior_step: the sample COUNTS installed with sfq_set_prior_counts stand for this call's own sample */
#define SFQ_BLOCK_AUTO 0xFFFFFFFFu

/* One entry per block: what a decoder needs besides the stream bytes (the "block index").
 * The per-block stream bytes are the reference's streams for a FASTQ consisting of that block alone,
 * with g_record_count / g_genofs_count (config.cpp:43-44) restarting at the block. */
typedef struct sfq_block_info {
    uint64_t first_record;                 /* 0-based index of the block's first record           */
    uint32_t n_records;                    /* num_records (usrs.cpp:405)                          */
    uint32_t llen;                         /* "llen"      (usrs.cpp:265)                          */
    uint8_t  solid;                        /* "usr.solid" (usrs.cpp:262)                          */
    uint8_t  two_id;                       /* "usr.2id"   (usrs.cpp:266)                          */
    uint8_t  n_byte;                       /* "gen.N_byte" (gens.cpp:104), 0 = none seen          */
    uint8_t  gen_bits;                     /* context bits used by the base model of this block   */
    uint32_t extra_hi;                     /* "qlt.extra.hi" (qlts.cpp:57-61)                     */
    uint32_t first_hdr_len;                /* "rec.first" length (recs.cpp:68-75)                 */
    uint64_t first_hdr_off;                /* its offset in the first-header blob                 */
    uint64_t size[SFQ_NSTREAMS];           /* bytes of each stream of this block (0 = absent); 64 bit: a format-6
                                              archive is ONE block, and the reference writes streams over 4 GiB  */
    uint32_t status;                       /* 0 or -SFQ_E_* for this block                        */
    uint32_t hdr_bytes;                    /* sum of header-line lengths (sizes the decoder's staging; 0 = unknown) */
} sfq_block_info;

typedef struct sfq_result {
    uint64_t n_records;
    uint32_t n_blocks;
    uint32_t abi_version;
    uint64_t stream_bytes[SFQ_NSTREAMS];   /* per stream: sum over blocks                          */
    uint64_t stream_offset[SFQ_NSTREAMS];  /* per stream: where its block-concatenation starts in d_out */
    uint64_t total_bytes;                  /* bytes used in d_out                                  */
    uint64_t first_hdr_bytes;              /* size of the first-header blob (see sfq_get_first_headers) */
    uint32_t n_chains;                     /* frozen tables: chains per chain-coded stream (else 0); sfq_decode_block_range: quality chains decoded */
    uint32_t reserved;
    double   kernel_ms[8];                 /* device time of the last call, by phase (see SFQ_T_*): a model's phase is
                                              everything on its stream -- counting passes, row building, the coding kernel */
    double   coder_ms[4];                  /* encode: the coding kernel alone (HIP events around its launch on its stream):
                                              [0] quality, [1] bases, [2] headers, [3] the framing kernel (k_frame).  What a kernel trace shows as
                                              k_qlt_encode_c / k_gen_encode_c (k_gm_code under the match model) / k_rec_tokens -- the longest of the
                                              header chains' kernels; the coder behind it, k_rec_code, is in the phase -- (k_*_encode_k / _w with
                                              adaptive tables) */
} sfq_result;

#define SFQ_T_FRAME   0   /* line index + block descriptors                     */
#define SFQ_T_QLT     1   /* quality model kernel(s)                            */
#define SFQ_T_GEN     2   /* base model kernel(s)                               */
#define SFQ_T_REC     3   /* header model kernel(s)                             */
#define SFQ_T_USR     4   /* framing-exception kernel(s)                        */
#define SFQ_T_PACK    5   /* size scan + compaction / FASTQ assembly            */
#define SFQ_T_TOTAL   6   /* first launch -> last launch of the call            */

/* ---- context ------------------------------------------------------------------------------- */
/* Replaces the reference's process-wide singletons (conf, onef, g_record_count, g_genofs_count:
 * config.hpp:62-64) with an explicit, re-entrant object bound to one HIP device. */
int  sfq_ctx_create(sfq_ctx** out, int hip_device);
void sfq_ctx_destroy(sfq_ctx* ctx);
const char* sfq_last_error(const sfq_ctx* ctx);         /* replaces croak() text (config.cpp:54-68) */
/* Upper bound on device bytes the context may hold for model tables (default: 70 % of the device). */
int  sfq_ctx_set_table_budget(sfq_ctx* ctx, uint64_t bytes);
/* Total memory of the context's device, in bytes (to share a GPU between contexts: budget = a fraction of it). */
uint64_t sfq_ctx_device_memory(const sfq_ctx* ctx);
/* The HIP stream the context launches on (a hipStream_t), for callers that order work against it. */
void* sfq_ctx_stream(sfq_ctx* ctx);
int  sfq_ctx_synchronize(sfq_ctx* ctx);
/* Page-locked host memory for the buffers handed to the *_host entry points: the copy engine reads / writes it at the
 * link's rate (a pageable buffer is staged through the driver page by page).  The reference has no counterpart: its
 * I/O is fread / fwrite into static buffers (usrs.cpp:95-118, filer.cpp).  NULL when the allocation fails. */
void* sfq_host_alloc(sfq_ctx* ctx, uint64_t bytes);
void  sfq_host_free(sfq_ctx* ctx, void* p);

/* ---- compress ------------------------------------------------------------------------------
 * Replaces the body of UsrSave::encode()'s record loop (usrs.cpp:400-404: gen.save / rec.save /
 * qlt.save per record) plus UsrSave::get_record()'s framing (usrs.cpp:303-390) for a whole buffer
 * of FASTQ text resident on the device.  d_out receives, stream after stream, the concatenation of
 * every block's bytes for that stream; sfq_get_block_index() tells the per-block sizes.
 * Worst-case d_out size: sfq_encode_bound(nbytes). Asynchronous errors are reported at return
 * (the call synchronizes the context's stream once, at the end).
 * PLACEMENT (sfq_encode_blocks, sfq_encode_qlt_blocks, sfq_build_priors, sfq_count_priors; sfq_decode_blocks and
 * sfq_decode_block_range below): d_fastq, d_streams and either output may lie at ANY address, whatever its alignment, inside a
 * larger buffer with live data on both sides.  No byte outside [d_fastq, d_fastq + nbytes) influences a result, and none outside
 * the extents of the streams -- [d_streams + stream_offset[s], + the sum of the blocks' size[s]) for every stream s -- does; an
 * input is never written.  Nothing outside [d_out, d_out + out_cap) / [d_fastq_out, d_fastq_out + out_cap) is written (inside it,
 * bytes behind the result may be).  Unlike sfq_crc32 and the other side passes, which read the whole aligned 16-byte units of their
 * text's first and last byte, these entries READ no byte outside those extents either: every wide load of the text and of a
 * stream is bounded by the extent's end and falls back to single bytes there, and the few loads that run past a LINE's end (a
 * header's last dword) stay inside the text, which goes on behind every header.  tests/test_placement.py holds the first three
 * statements at every kind of offset from a 16-byte boundary, between guard bytes that would show; the last is by reading the
 * kernels. */
uint64_t sfq_encode_bound(uint64_t fastq_bytes);
int sfq_encode_blocks(sfq_ctx* ctx, const uint8_t* d_fastq, uint64_t nbytes, const sfq_params* params,
                      uint8_t* d_out, uint64_t out_cap, sfq_result* result);
/* BASELINE.json config C2: the quality model alone == QltSave::save over all records (qlts.hpp:82-90). */
int sfq_encode_qlt_blocks(sfq_ctx* ctx, const uint8_t* d_fastq, uint64_t nbytes, const sfq_params* params,
                          uint8_t* d_out, uint64_t out_cap, sfq_result* result);
/* The priors of a text without coding it: afterwards sfq_get_qlt_prior (and, with frozen tables, sfq_get_rec_prior) hold what
 * an sfq_encode_blocks call with the same parameters would have built.  For several contexts / GPUs that compress parts
 * of one file from ONE prior: build it once, install it everywhere (sfq_set_*_prior), encode with prior_step = SFQ_PRIOR_GIVEN. */
int sfq_build_priors(sfq_ctx* ctx, const uint8_t* d_fastq, uint64_t nbytes, const sfq_params* params);
/* Several GPUs, one file, NO serial head: every rank counts the sample of ITS share of the file (sfq_count_priors: every
 * sample_scale-th record of what one call alone would sample -- sample_scale = the number of ranks keeps the job's sample the size
 * of one call's), the ranks add their counts up (an all-reduce of two u32 arrays: sfq_get_prior_counts -> the caller's device
 * buffers -> sfq_set_prior_counts), and every rank codes with prior_step = SFQ_PRIOR_COUNTS: identical priors everywhere, nobody
 * waits for a rank that builds them.  Array sizes in u32 words: sfq_prior_counts_words.
 * An sfq_encode_blocks with SFQ_PRIOR_COUNTS that follows sfq_count_priors on the same context, buffer and size keeps that
 * call's line index (the text is framed once per step, not twice): the text must not change between the two calls. */
int  sfq_count_priors(sfq_ctx* ctx, const uint8_t* d_fastq, uint64_t nbytes, const sfq_params* params, uint32_t sample_scale);
void sfq_prior_counts_words(int level, uint64_t* qlt_words, uint64_t* rec_words);
int  sfq_get_prior_counts(sfq_ctx* ctx, int level, uint32_t* d_qlt, uint32_t* d_rec);
int  sfq_set_prior_counts(sfq_ctx* ctx, int level, const uint32_t* d_qlt, const uint32_t* d_rec);
/* Same with host buffers (stages through the context's device memory; PCIe-inclusive). */
int sfq_encode_blocks_host(sfq_ctx* ctx, const uint8_t* h_fastq, uint64_t nbytes, const sfq_params* params,
                           uint8_t* h_out, uint64_t out_cap, sfq_result* result);

/* Block index / first headers of the LAST encode call on this context (host copies). */
int sfq_get_block_index(sfq_ctx* ctx, sfq_block_info* h_blocks, uint32_t cap);
int sfq_get_first_headers(sfq_ctx* ctx, uint8_t* h_blob, uint64_t cap);

/* Quality warm-start prior of the LAST encode call (the "qlt.pri" stream): returns its size, copies it if
 * cap allows; 0 = the call used cold blocks. */
int64_t sfq_get_qlt_prior(sfq_ctx* ctx, uint8_t* h_blob, uint64_t cap);
/* Install the prior the next sfq_decode_blocks call must start its quality rows from (n = 0: cold). */
int sfq_set_qlt_prior(sfq_ctx* ctx, const uint8_t* h_blob, uint64_t n);
/* Frozen tables: the header prior of the LAST encode call (the "rec.pri" stream: scaled symbol counts of the header
 * model's rows); same conventions.  0 = the call coded its headers with adaptive rows. */
int64_t sfq_get_rec_prior(sfq_ctx* ctx, uint8_t* h_blob, uint64_t cap);
int sfq_set_rec_prior(sfq_ctx* ctx, const uint8_t* h_blob, uint64_t n);
/* Frozen tables: the chain index of the LAST encode call (the "chn.idx" stream: records per chain, flags, and the size
 * of every chain's qlt and gen stream); returns its size, copies it if cap allows; 0 = the call used adaptive tables.
 * A decoder installs it before sfq_decode_blocks (n = 0: the archive has none, i.e. adaptive tables). */
int64_t sfq_get_chain_index(sfq_ctx* ctx, uint8_t* h_blob, uint64_t cap);
int sfq_set_chain_index(sfq_ctx* ctx, const uint8_t* h_blob, uint64_t n);

/* ---- decompress ----------------------------------------------------------------------------
 * Replaces UsrLoad::decode()'s loop (usrs.cpp:555-571: rec.load / qlt.load / gen.load / save).
 * d_streams holds the streams laid out as sfq_encode_blocks wrote them (stream_offset[] + running
 * sum of sfq_block_info.size[]); a reference-written format-6 archive is the one-block case with
 * gen_bits = the level's.  h_first_hdrs is the first-header blob (one "rec.first" per block).
 * Writes the FASTQ text to d_fastq_out; *out_bytes = its length. */
int sfq_decode_blocks(sfq_ctx* ctx, const sfq_params* params, const sfq_block_info* h_blocks, uint32_t n_blocks,
                      const uint8_t* h_first_hdrs, uint64_t first_hdr_bytes,
                      const uint8_t* d_streams, const uint64_t stream_offset[SFQ_NSTREAMS],
                      uint8_t* d_fastq_out, uint64_t out_cap, uint64_t* out_bytes, sfq_result* result);
int sfq_decode_blocks_host(sfq_ctx* ctx, const sfq_params* params, const sfq_block_info* h_blocks, uint32_t n_blocks,
                           const uint8_t* h_first_hdrs, uint64_t first_hdr_bytes,
                           const uint8_t* h_streams, uint64_t streams_bytes, const uint64_t stream_offset[SFQ_NSTREAMS],
                           uint8_t* h_fastq_out, uint64_t out_cap, uint64_t* out_bytes, sfq_result* result);
/* A WINDOW of the call's blocks -- blocks [first_block, first_block + n_window) -- without decoding the rest (the reference has no
 * counterpart: UsrLoad::decode reads a file from its first record on).  h_blocks, n_blocks, the first-header blob, stream_offset and the
 * installed blobs (sfq_set_qlt_prior / sfq_set_rec_prior / sfq_set_chain_index) describe the WHOLE call, exactly as for
 * sfq_decode_blocks; the output is the text of the window's records and nothing else, from byte 0 of the output buffer, *out_bytes its
 * length (SFQ_E_OVERFLOW: the size needed).  result->n_records / n_blocks are the window's; result->n_chains = the quality chains
 * the call decoded (0 with adaptive tables).  What is decoded outside the window is what the format forces: with
 * frozen tables and a base model ("chn.idx" flag bit 0) the line lengths of the blocks in front and the bases of the generations
 * before the window's last block's; otherwise nothing.  n_window = 0 or a window past n_blocks: SFQ_E_ARG; a one-block archive with
 * oversize records (usr.lrec): SFQ_E_UNSUPPORTED.  Checksums installed with sfq_set_block_checksums are the WINDOW's blocks' (n must
 * equal n_window), and sfq_get_checksums returns n_window values.  The _host entry copies to the device only the byte ranges of
 * every stream that the call reads. */
int sfq_decode_block_range(sfq_ctx* ctx, const sfq_params* params, const sfq_block_info* h_blocks, uint32_t n_blocks,
                           const uint8_t* h_first_hdrs, uint64_t first_hdr_bytes,
                           const uint8_t* d_streams, const uint64_t stream_offset[SFQ_NSTREAMS],
                           uint32_t first_block, uint32_t n_window,
                           uint8_t* d_fastq_out, uint64_t out_cap, uint64_t* out_bytes, sfq_result* result);
int sfq_decode_block_range_host(sfq_ctx* ctx, const sfq_params* params, const sfq_block_info* h_blocks, uint32_t n_blocks,
                                const uint8_t* h_first_hdrs, uint64_t first_hdr_bytes,
                                const uint8_t* h_streams, uint64_t streams_bytes, const uint64_t stream_offset[SFQ_NSTREAMS],
                                uint32_t first_block, uint32_t n_window,
                                uint8_t* h_fastq_out, uint64_t out_cap, uint64_t* out_bytes, sfq_result* result);

/* ---- checksums ------------------------------------------------------------------------------------------------------
 * CRC-32 (IEEE 802.3, reflected, polynomial 0xEDB88320, init and final XOR 0xFFFFFFFF: the value of zlib's crc32) computed
 * on the device (crc.hip).  The reference has none: its usage() (config.cpp:191-193) asks users to keep an md5sum.
 * sfq_crc32: the CRC of every range [h_bounds[i], h_bounds[i+1]) of d_data, i < n_ranges, into h_crc[i] (bounds non-decreasing).
 * The pass reads whole aligned 16-byte units: up to 15 bytes before d_data + h_bounds[0] and after d_data + h_bounds[n_ranges]
 * are read (never used), within the aligned 16-byte units of the first and last byte -- so never across a page, but possibly
 * outside the caller's allocation.  The encode and decode passes below read their text the same way. */
int sfq_crc32(sfq_ctx* ctx, const uint8_t* d_data, const uint64_t* h_bounds, uint32_t n_ranges, uint32_t* h_crc);
/* zlib's crc32_combine: the CRC of A followed by B from crc(A), crc(B) and the length of B (host only, no GPU). */
uint32_t sfq_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* on != 0: every encode call computes one CRC per block -- block b covers the input from its first record's header line up to
 * the next block's first record (to the end of the text for the last block) -- and the CRC of its whole text, on a stream of its
 * own; every decode call computes them of its output.  Default off: no pass, no event, no buffer. */
int sfq_ctx_set_checksums(sfq_ctx* ctx, int on);
/* The last call's per-block CRCs (if cap allows) and the CRC of its whole text; returns the number of blocks (0: the call
 * computed none). */
int sfq_get_checksums(sfq_ctx* ctx, uint32_t* h_block_crc, uint32_t cap, uint32_t* h_text_crc);
/* The expected CRCs of the blocks of the NEXT decode call, consumed by it: that call checks its output against them and returns
 * SFQ_E_CORRUPT on a mismatch (sfq_last_error names the first bad block; the text stays in the output buffer, and
 * sfq_get_checksums lists what was computed); n must equal its n_blocks, or it returns SFQ_E_ARG. */
int sfq_set_block_checksums(sfq_ctx* ctx, const uint32_t* h_crc, uint32_t n);

/* ---- text statistics ---------------------------------------------------------------------------------------------------
 * What the first questions about a FASTQ file need -- bases, GC and N share, Q20 / Q30 share, read-length range, mean quality per
 * cycle -- counted on the device while the text is resident for an encode (stats.hip), on a stream of its own.  The reference has
 * none.  A line is what the call's line index says it is: the bytes between two '\n', so the leading '@' / '+' and a SOLiD prefix
 * character are counted, a '\n' never.  The statistics cover the whole input text, format 6's oversize records included.
 * Only the encode calls compute them (sfq_encode_blocks, sfq_encode_blocks_host, sfq_encode_qlt_blocks); the priors-only calls
 * (sfq_build_priors, sfq_count_priors) do not, and -- deliberately -- no decode does: a decoder's text is the encoder's, whose
 * statistics the archive carries ("txt.stat"), and a decode call has no line index of its output to count from. */
#define SFQ_STATS_CYCLES 512
typedef struct sfq_text_stats {
    uint64_t n_records;
    uint64_t hdr_bytes, seq_bytes, plus_bytes, qlt_bytes; /* sum of the lengths of lines 1..4 of every record */
    uint32_t seq_len_min, seq_len_max;                    /* over line 2 */
    uint64_t seq_hist[256];                               /* byte histogram of all lines 2 */
    uint64_t qlt_hist[256];                               /* byte histogram of all lines 4 */
    uint64_t cyc_n[SFQ_STATS_CYCLES + 1];                 /* [c]: quality bytes at position c of their line; [512]: all at positions >= 512 */
    uint64_t cyc_qsum[SFQ_STATS_CYCLES + 1];              /* the sum of those bytes' values (raw byte values: the Phred offset is the reader's) */
} sfq_text_stats;
/* on != 0: every encode call counts the statistics of its text.  Default off: no pass, no event, no buffer; the encoded bytes
 * are the same either way. */
int  sfq_ctx_set_stats(sfq_ctx* ctx, int on);
/* 1: *out = the last encode call's statistics; 0: it computed none (the switch was off, the call failed, or it was not an encode). */
int  sfq_get_text_stats(sfq_ctx* ctx, sfq_text_stats* out);
/* The statistics of two texts into those of both (host only): sums add, the length range widens; merging into an all-zero
 * struct copies. */
void sfq_text_stats_merge(sfq_text_stats* into, const sfq_text_stats* add);
/* The "txt.stat" stream; returns its size (out == NULL: size only), SFQ_E_OVERFLOW where cap is short. */
int64_t sfq_pack_text_stats(const sfq_text_stats* stats, uint8_t* out, uint64_t cap);
/* SFQ_E_CORRUPT: truncated, trailing bytes, an unknown version, an array longer than the struct's. */
int  sfq_unpack_text_stats(const uint8_t* bytes, uint64_t n, sfq_text_stats* out);

/* ---- quality binning ---------------------------------------------------------------------------------------------------
 * The one LOSSY option, strictly opt-in: every byte of every 4th line of a FASTQ text (line number & 3 == 3 counted from the start
 * of the buffer; the '\n' excluded) goes through a 256-byte table, in place on the device (qmap.hip), before an encode frames the
 * text.  The pass is text to text: the streams, the checksums, the statistics and every decoder see the mapped text and nothing
 * else.  The reference has no counterpart.  A text without a final '\n' is handled: its last line is a line.  Like sfq_crc32 the
 * pass reads the whole aligned 16-byte units of the text's first and last byte; it writes nothing outside the text.
 * Presets, Phred+33 (Q = byte - 33); Q0 and Q1 ('!' and '"': "no call", and the '!' <-> N coupling of gens.cpp) stay, both are idempotent:
 *   SFQ_QMAP_ILLUMINA8: 2-9 -> 6, 10-19 -> 15, 20-24 -> 22, 25-29 -> 27, 30-34 -> 33, 35-39 -> 37, 40-93 -> 40
 *   SFQ_QMAP_NOVASEQ4:  2 -> 2, 3-14 -> 12, 15-29 -> 23, 30-93 -> 37   (the values of sfq_synth_fastq kind 2: such a text is a fixed point) */
#define SFQ_QMAP_ILLUMINA8 1
#define SFQ_QMAP_NOVASEQ4  2
/* host only, no GPU: fills lut[256]; SFQ_E_ARG for an unknown preset */
int sfq_quality_map_preset(int preset, uint8_t lut[256]);
/* host only: SFQ_OK, or SFQ_E_ARG unless lut[b] == b for every b < 33 or b > 126, and 33 <= lut[b] <= 126 for every other b
 * (a table can neither move nor make a line end, a control byte or a byte outside ASCII) */
int sfq_quality_map_check(const uint8_t lut[256]);
/* in place, on the context's stream, synchronises once; *changed (may be NULL) = bytes whose value changed.  SFQ_E_ARG for a table
 * that sfq_quality_map_check refuses (the text is not touched). */
int sfq_map_qualities(sfq_ctx* ctx, uint8_t* d_fastq, uint64_t nbytes, const uint8_t lut[256], uint64_t* changed);
/* lut != NULL: every *_host encode entry (sfq_encode_blocks_host) maps its staged copy of the text before it frames it; the
 * caller's host buffer is not touched.  NULL: off (default): nothing is launched or allocated.  SFQ_E_ARG for a table that
 * sfq_quality_map_check refuses (the installed map stays as it was).
 * The entries that take CONST device text -- sfq_encode_blocks, sfq_encode_qlt_blocks, sfq_build_priors, sfq_count_priors --
 * cannot apply a map: while one is installed they return SFQ_E_UNSUPPORTED (call sfq_map_qualities on the buffer instead). */
int sfq_ctx_set_quality_map(sfq_ctx* ctx, const uint8_t* lut);
/* bytes changed by the last encode call's map (0 where none ran) */
uint64_t sfq_get_quality_map_changed(const sfq_ctx* ctx);

/* ---- paired files --------------------------------------------------------------------------------------------------------
 * Two FASTQ texts whose record i are mates (R1 / R2) are coded as ONE text, A0 B0 A1 B1 ...: the header model then codes a mate's
 * header as the one field that differs from its partner's.  Interleaving and splitting are text-to-text passes on the device
 * (pair.hip), in front of an encode's framing and behind a decode's assembly; no stream, coder or block format knows of them.  A
 * record is four lines; a text without a final '\n' ends in a line all the same.
 * Every entry: SFQ_E_ARG for a null pointer or an empty text; SFQ_E_FORMAT for a text whose lines are no multiple of four, for
 * A and B of different record counts (sfq_last_error gives both), for an odd number of records to split, and for an A that does
 * not end in '\n' (its last record would run into its mate; B may lack the final '\n', the output then lacks it too and a split
 * gives it back exactly); SFQ_E_UNSUPPORTED for a record of 4 GiB or more.  A refused call writes nothing to its output.  Each
 * call runs on the context's stream and synchronises once.  Like sfq_crc32 the passes read the whole aligned 16-byte units of a
 * text's first and last byte; they write nothing outside the output's bytes. */
/* out = A0 B0 A1 B1 ...; *out_bytes = na + nb (on SFQ_E_OVERFLOW: the size needed); *n_pairs may be NULL; d_out overlaps neither text */
int sfq_interleave(sfq_ctx* ctx, const uint8_t* d_a, uint64_t na, const uint8_t* d_b, uint64_t nb,
                   uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes, uint64_t* n_pairs);
/* d_out[0, *split) = the even records in order, d_out[*split, n) = the odd ones; d_out must not overlap d_text; *n_pairs may be NULL */
int sfq_split_pairs(sfq_ctx* ctx, const uint8_t* d_text, uint64_t n, uint8_t* d_out, uint64_t out_cap,
                    uint64_t* split, uint64_t* n_pairs);
/* sfq_encode_blocks_host of the interleaved text: both files staged, interleaved on the device, then the installed quality map,
 * then the call as it is.  The host buffers are not touched.  The statistics, the checksums and the quality map of the call are
 * those of the INTERLEAVED text (sfq_result.raw sizes too): that text is what the archive describes. */
int sfq_encode_pairs_host(sfq_ctx* ctx, const uint8_t* h_a, uint64_t na, const uint8_t* h_b, uint64_t nb,
                          const sfq_params* params, uint8_t* h_out, uint64_t out_cap, sfq_result* result);
/* on != 0: sfq_decode_blocks_host hands back the split layout (sfq_split_pairs) instead of the interleaved text, split behind the
 * checksum pass: the CRCs, installed ones included, are those of the interleaved text.  Costs one more device buffer of the
 * text's size, held while the switch is on.  While it is on, sfq_decode_block_range and sfq_decode_block_range_host return
 * SFQ_E_UNSUPPORTED (a window may start at a second mate).  sfq_decode_blocks writes into the caller's device buffer and is not
 * affected: call sfq_split_pairs on its output.  Default off: nothing is launched or allocated. */
int sfq_ctx_set_pair_split(sfq_ctx* ctx, int on);
/* 1: the last decode call split its text, *first_bytes = where the second mates begin; 0: it did not (both set to 0) */
int sfq_get_pair_split(const sfq_ctx* ctx, uint64_t* first_bytes, uint64_t* n_pairs);

/* Records [first_record, first_record + n_records) of d_text, split: d_out[0, *split) = the window's records 0, 2, 4, ... (counted from
 * first_record), d_out[*split, *out_bytes) = its records 1, 3, 5, ...  *out_bytes = the bytes of those records (on SFQ_E_OVERFLOW: the
 * size needed).  first_record may be odd or even; n_records must be even and > 0 (SFQ_E_FORMAT otherwise); a range that ends behind the
 * text's last record: SFQ_E_ARG.  The text's own record count may be odd.  Everything else as sfq_split_pairs: one copy cuts and
 * splits, a refused call writes nothing, and with first_record = 0 and all records the output is sfq_split_pairs' byte for byte. */
int sfq_split_pairs_range(sfq_ctx* ctx, const uint8_t* d_text, uint64_t n, uint64_t first_record, uint64_t n_records,
                          uint8_t* d_out, uint64_t out_cap, uint64_t* split, uint64_t* out_bytes);

/* Mates by name.  A record's NAME is the bytes of its first line behind the line's first byte (the '@'), up to but not including the
 * first ' ', '\t' or the line end; if what remains is two bytes or longer and ends in "/1" or "/2", those two bytes are dropped.  Two
 * records are mates by name if their names have the same length and the same bytes: "@r/1" and "@r/2", "@r 1:N:0:ACGT" and
 * "@r 2:N:0:ACGT", "@r/1" and "@r", two empty names are; "@r1" and "@r10", "@ra" and "@rb" are not. */
typedef struct sfq_mate_report {
    uint64_t n_pairs, n_mismatch;
    uint64_t first_mismatch;               /* pair index, the smallest; valid where n_mismatch                         */
    uint64_t first_off_a, first_off_b;     /* byte offsets of that pair's header lines in their texts                   */
} sfq_mate_report;
/* d_b != NULL: record i of d_a against record i of d_b (the refusals of sfq_interleave: line counts, record counts, an A without its
 * final line end).  d_b == NULL: d_a is an interleaved text, record 2k against record 2k + 1 (the refusals of sfq_split_pairs; both
 * offsets are d_a's).  Mismatches are REPORTED, not refused: SFQ_OK with n_mismatch > 0.  Writes nothing to either text; reads them
 * like the other passes; synchronises once. */
int sfq_check_mates(sfq_ctx* ctx, const uint8_t* d_a, uint64_t na, const uint8_t* d_b, uint64_t nb, sfq_mate_report* report);
/* on != 0: sfq_encode_pairs_host compares the names before it codes (between the record starts and the copy: no second counting pass,
 * no second synchronise) and returns SFQ_E_FORMAT where a pair differs -- sfq_last_error gives the count, the first pair's index and
 * both names (each cut at 64 bytes) -- with nothing written to h_out.  Default off: nothing is launched, allocated or copied that is
 * not today. */
int sfq_ctx_set_mate_check(sfq_ctx* ctx, int on);
/* 1: the last sfq_encode_pairs_host ran the check, *out = what it found; 0: it did not (*out zeroed) */
int sfq_get_mate_report(const sfq_ctx* ctx, sfq_mate_report* out);

/* host only: the blocks that hold records [2*first_pair, 2*(first_pair + n_pairs)) of a call's block index (by the blocks' n_records);
 * SFQ_E_ARG where the range ends behind the last record or n_pairs == 0 */
int sfq_pair_window_blocks(const sfq_block_info* h_blocks, uint32_t n_blocks, uint64_t first_pair, uint64_t n_pairs,
                           uint32_t* first_block, uint32_t* n_window);
/* Pairs [first_pair, first_pair + n_pairs) of a call written from paired files, split: h_out[0, *split) the first mates,
 * h_out[*split, *out_bytes) the second.  Decodes the blocks sfq_pair_window_blocks names exactly as sfq_decode_block_range_host does
 * (same arguments, same partial upload, same dependence on what lies in front), then cuts to the records and splits ON THE DEVICE
 * (sfq_split_pairs_range); only the result crosses the link.  out_cap sizes the decoded window of blocks (SFQ_E_OVERFLOW: *out_bytes =
 * the size needed); h_out holds out_cap bytes.  Works whatever sfq_ctx_set_pair_split says and answers sfq_get_pair_split afterwards.
 * Installed block checksums are those of the window's blocks (of the interleaved text), checked before the cut.  A call whose record
 * count is odd: SFQ_E_FORMAT; n_pairs == 0 or a window past the end: SFQ_E_ARG.  There is no device-pointer variant: a caller with
 * device buffers composes sfq_decode_block_range and sfq_split_pairs_range. */
int sfq_decode_pair_range_host(sfq_ctx* ctx, const sfq_params* params, const sfq_block_info* h_blocks, uint32_t n_blocks,
                               const uint8_t* h_first_hdrs, uint64_t first_hdr_bytes,
                               const uint8_t* h_streams, uint64_t streams_bytes, const uint64_t stream_offset[SFQ_NSTREAMS],
                               uint64_t first_pair, uint64_t n_pairs,
                               uint8_t* h_out, uint64_t out_cap, uint64_t* out_bytes, uint64_t* split, sfq_result* result);

/* ---- picked lines ---------------------------------------------------------------------------------------------------------
 * What a consumer of a decoded FASTQ often reads is part of it: FASTA, the read names, the base lines or the quality lines.  The
 * pass (pick.hip) picks those lines on the device, text to text like the paired files' passes, behind a decode's assembly; no
 * stream, coder or block format knows of it.  A line is the bytes up to and including a '\n'; a text without a final '\n' ends in
 * a line all the same, whose piece then lacks the '\n' and so does the result.  A record is four lines; '\r' is a byte like any
 * other.  Every record contributes ONE contiguous piece of the text, and the result is the pieces in record order with nothing
 * between them.  Every piece holds at least one byte, so the result is never larger than the text: out_cap = n always suffices. */
#define SFQ_PICK_FASTA 1   /* lines 1 and 2 of every record; the first byte of line 1 becomes '>' */
#define SFQ_PICK_NAMES 2   /* line 1 without its first byte (the '@') */
#define SFQ_PICK_BASES 3   /* line 2 */
#define SFQ_PICK_QUALS 4   /* line 4 */
/* Records [first_record, first_record + n_records) of d_text, picked; n_records = UINT64_MAX: to the text's last record.
 * *out_bytes = the bytes of the result (on SFQ_E_OVERFLOW: the size needed), *n_picked (may be NULL) = records picked.
 * SFQ_E_ARG: a null pointer, n == 0, an unknown selection, n_records == 0, a range that ends behind the last record (with UINT64_MAX:
 * a first_record that is no record of the text).  SFQ_E_FORMAT: a text whose lines are no multiple of four; under SFQ_PICK_FASTA and
 * SFQ_PICK_NAMES a record IN THE RANGE whose first byte is not '@' (sfq_last_error names the smallest such record and its byte
 * offset; SFQ_PICK_BASES and SFQ_PICK_QUALS do not look at that byte).  SFQ_E_OVERFLOW: a result larger than out_cap.
 * SFQ_E_UNSUPPORTED: a record whose piece holds 4 GiB or more.  Every refusal is decided on the device before the copy: a refused call
 * writes nothing to d_out.  A call that succeeds writes d_out[0, *out_bytes) and nothing else: the bytes behind the result stay as
 * they were, inside out_cap too.  d_out must not overlap d_text.  The call runs on the context's stream and synchronises once.
 * Like sfq_crc32 it may read the whole aligned 16-byte units of the text's first and last byte. */
int sfq_pick_lines(sfq_ctx* ctx, const uint8_t* d_text, uint64_t n, int what, uint64_t first_record, uint64_t n_records,
                   uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes, uint64_t* n_picked);
/* what != 0: sfq_decode_blocks_host, sfq_decode_block_range_host and sfq_decode_pair_range_host hand back the picked lines of
 * the text they decoded instead of the text; 0: off (default).  SFQ_E_ARG for an unknown selection (the setting stays).
 * The pick is the call's last pass: behind the checksum pass (the CRCs, installed ones included, stay those of the decoded FASTQ
 * text) and behind the pair split or the pair window's cut-and-split, where either runs.  A split layout is picked as one text --
 * first mates, then second mates, both whole records -- and the boundary that sfq_get_pair_split and sfq_decode_pair_range_host's
 * *split report is then the boundary IN THE PICKED RESULT.  out_cap keeps sizing the DECODED text; only the picked bytes cross
 * the link, and *out_bytes is their count.  Costs one more device buffer of the text's size, held while the switch is on.  The
 * device-pointer decode entries are not affected: call sfq_pick_lines on their output.  Default off: nothing is launched,
 * allocated or copied that is not today. */
int sfq_ctx_set_pick(sfq_ctx* ctx, int what);
/* 1: the last decode call picked; *what, *text_bytes (the decoded text's size before the pick), *n_records; 0: it did not (all zeroed) */
int sfq_get_pick(const sfq_ctx* ctx, int* what, uint64_t* text_bytes, uint64_t* n_records);

/* ---- selected records -------------------------------------------------------------------------------------------------------
 * A subset of a decoded FASTQ chosen by CONTENT, while the text is on the device: the records of a range that pass a filter and a
 * reproducible sample, whole and in order (sel.hip).  Text to text like the picked lines, whose copy the pass uses; no stream, coder
 * or block format knows of it.
 * Lines and records: they are sfq_pick_lines' own.  A line ends at '\n'; a text without a final '\n' still ends in a line; '\r' is a
 *   byte like any other.  Line lengths exclude the '\n'.
 * Content verdict: the AND of the terms that are on; if invert is set, the result is negated.
 *   Length: min_len <= L2 <= max_len, where L2 is the length of line 2.
 *   N: the count of 'N' and 'n' bytes in line 2 is <= max_n.
 *   Quality: with S the sum of line 4's bytes and L its length, the term holds when 100 * (S - qual_base * L) >= min_mean_q_x100 * L.
 *     The arithmetic is signed 64-bit.  An empty quality line passes (min_len is what catches empty lines).  Sums are 64-bit: a line
 *     may hold close to 4 GiB.
 *   Motif: the motif occurs as a substring of line 2, compared without regard to letter case.  With motif_rc, its reverse complement
 *     counts as an occurrence too.  Only line 2 counts: an occurrence in a header, in a '+' line that repeats the header, or in a
 *     quality line (ACGT are legal quality bytes) is no occurrence.  An occurrence never runs across a line end.
 * Pairs: a pair's content verdict is the AND (SFQ_SELECT_BOTH) or the OR (SFQ_SELECT_EITHER) of its mates' content verdicts, taken
 *   after invert.
 * Sampling: works on the index i = index_base + record number; with pairs, i is shifted right by one, so that mates share it.
 *     h = sample_seed + (i + 1) * 0x9E3779B97F4A7C15
 *     h ^= h >> 30; h *= 0xBF58476D1CE4E5B9
 *     h ^= h >> 27; h *= 0x94D049BB133111EB
 *     h ^= h >> 31                                        (all arithmetic mod 2^64)
 *   The record is kept where (h >> 32) < sample.  invert does not touch the range or the sample.
 * Kept records: a record is kept when it is in the range, it is sampled, and its content verdict holds.  The result is the kept
 *   records, whole (four lines each), in order, with nothing between them. */
#define SFQ_SELECT_BOTH 1
#define SFQ_SELECT_EITHER 2
typedef struct sfq_select {
    uint64_t first_record, n_records;   /* the range the selection looks at; n_records = UINT64_MAX: to the last record. Records outside are dropped */
    uint32_t min_len, max_len;          /* bytes of line 2 without its '\n'; 0 / UINT32_MAX = off */
    uint32_t max_n;                     /* bytes 'N' or 'n' in line 2; UINT32_MAX = off */
    uint32_t min_mean_q_x100;           /* 0 = off */
    uint32_t qual_base;                 /* subtracted from every quality byte (33 for Phred+33); <= 126 */
    uint32_t motif_len;                 /* 0 = off, at most 32 */
    uint8_t  motif[32];                 /* 'A' 'C' 'G' 'T' only */
    uint32_t motif_rc;                  /* != 0: the reverse complement counts as an occurrence too */
    uint32_t invert;                    /* != 0: the CONTENT verdict is negated (grep -v) */
    uint32_t pairs;                     /* 0: records stand alone; SFQ_SELECT_BOTH / SFQ_SELECT_EITHER: records 2k, 2k+1 are kept or dropped together */
    uint32_t sample;                    /* 0 = off; else keep where (h >> 32) < sample */
    uint64_t sample_seed, index_base;
} sfq_select;
typedef struct sfq_select_report {
    uint64_t n_in_range, n_kept, text_bytes, kept_bytes;
    uint64_t n_fail[4];                 /* records in range that fail the length / N / quality / motif term (before invert); 0 for a term that is off */
} sfq_select_report;
/* host only, no GPU: SFQ_OK, or SFQ_E_ARG for a null pointer, a motif byte outside ACGT, motif_len > 32, min_len > max_len,
 * qual_base > 126, pairs > 2, n_records == 0, or, with pairs, an odd first_record or index_base */
int sfq_select_check(const sfq_select* sel);
/* host only, no GPU: a rule from the CLI's -k SPEC, a comma-separated list of the terms minlen=N, maxlen=N, maxn=N, meanq=Q (a decimal
 * with up to two fraction digits; Phred+33), seq=MOTIF (upper or lower case, stored upper case), rc, invert, either and sample=F[:SEED]
 * (0 < F < 1, sample = floor(F * 2^32), seed 0 if absent).  *sel: the rule, every term that is not named off, the range (0, UINT64_MAX),
 * pairs = 0; *either (may be NULL) = 1 where the list names `either` -- whether records are pairs is the caller's to know.
 * SFQ_E_ARG for an unknown term, a bad number, a motif with a byte outside ACGTacgt or longer than 32; err (may be NULL) then says which. */
int sfq_select_parse(const char* spec, sfq_select* sel, int* either, char* err, uint64_t err_cap);
/* The selection of d_text[0, n) into d_out; *out_bytes = the bytes of the result (on SFQ_E_OVERFLOW: the size needed).
 * SFQ_E_ARG: a null pointer (report may be NULL), n == 0, a struct that sfq_select_check refuses, a range that ends behind the last
 * record.  SFQ_E_FORMAT: lines that are no multiple of four; with pairs, an odd record count in the range (n_records odd, or odd to
 * the end).  SFQ_E_UNSUPPORTED: a record of 4 GiB or more.  SFQ_E_OVERFLOW: a result larger than out_cap.
 * No record kept is not an error: SFQ_OK with *out_bytes = 0 and nothing written.  Every refusal is decided on the device before the
 * copy: a refused call writes nothing.  A call that succeeds writes d_out[0, *out_bytes) and nothing else.  d_out must not overlap
 * the text.  The call runs on the context's stream and synchronises once.  Like the other side passes, it may read the whole aligned
 * 16-byte units that hold the text's first and last byte. */
int sfq_select_records(sfq_ctx* ctx, const uint8_t* d_text, uint64_t n, const sfq_select* sel,
                       uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes, sfq_select_report* report);
/* sel != NULL: sfq_decode_blocks_host, sfq_decode_block_range_host and sfq_decode_pair_range_host hand back the selection of the text
 * they decoded (the struct is copied; SFQ_E_ARG, and the setting stays, where sfq_select_check refuses it); NULL: off (default).
 * The selection is the first pass behind the checksum pass: the CRCs, installed ones included, stay those of the decoded text.  It
 * runs in front of the pair split and in front of the pick, which then run unchanged on the selected text.  Because the range is part
 * of the struct, a caller can cut a window of blocks down to records without a host pass.  While the pair split is on, a selection
 * with pairs == 0 is refused with SFQ_E_ARG: the mates would fall out of step.  sfq_decode_pair_range_host supplies the range
 * itself, the window's pairs: the selection runs first, on the decoded blocks, with that range, and the cut-and-split then runs as a
 * plain split of the whole selected text; the struct's own range must be (0, UINT64_MAX) and pairs must not be 0 (SFQ_E_ARG;
 * likewise a window whose first pair is an odd record of the blocks that hold it -- blocks of an odd record count).
 * out_cap keeps sizing the DECODED text.  With nothing kept the _host entries return SFQ_OK and 0 bytes; the split and the pick are
 * skipped and their get_* calls answer 0.  Costs one more device buffer of the text's size, held while the switch is on.  The
 * device-pointer decode entries are not affected.  Default off: nothing is launched, allocated or copied that is not today. */
int sfq_ctx_set_select(sfq_ctx* ctx, const sfq_select* sel);
/* 1: the last decode call selected, *out = what it found; 0: it did not (*out zeroed) */
int sfq_get_select(const sfq_ctx* ctx, sfq_select_report* out);

/* ---- trimmed records ----------------------------------------------------------------------------------------------------------
 * What a consumer of FASTQ does first is trim: crop fixed ends, cut low-quality ends, clip the read-through adapter.  The pass
 * (trim.hip) does it while the text is on the device, text to text like the selected records, whose line starts and copy it uses; no
 * stream, coder or block format knows of it.  It is the first pass that changes a record's inside: NO RECORD IS EVER DROPPED, a record
 * cut to nothing keeps its four lines, two of them empty (sfq_select's min_len is what drops it).
 * Lines and records: they are sfq_pick_lines' own.  A line ends at '\n'; a text without a final '\n' still ends in a line; '\r' is a
 *   byte like any other.  Lengths exclude the '\n'.
 * The rule, for one record: L = the length of line 2, which line 4 must share; q(p) = line4[p] - qual_base, signed.  Every term is a
 * function of the ORIGINAL record alone, so the terms have no order, and the cut is their intersection:
 *   a_head  = min(head, L)                                   b_tail  = L - min(tail, L)
 *   a_lead  = lead_q  ? smallest p with q(p) >= lead_q  (L if none)      : 0
 *   b_trail = trail_q ? 1 + largest p with q(p) >= trail_q (0 if none)   : L
 *   b_win   = win_len ? smallest p in [0, L - win_len] with
 *                       100 * sum_{j<win_len} q(p+j) < win_q_x100 * win_len   (signed 64-bit; L if none, L if L < win_len) : L
 *   b_ad    = adapter_len ? smallest p in [0, L) at which the adapter matches (L if none) : L
 *   s = max(a_head, a_lead);  e = min(b_tail, b_trail, b_win, b_ad);  if e < s: e = s
 *   if max_len != UINT32_MAX: e = min(e, s + max_len)
 * The adapter matches at p when k = min(adapter_len, L - p) is at least adapter_min (a partial overlap at the 3' end) and the number
 *   of j < k with upper(line2[p+j]) != adapter[j] is at most adapter_mm * k / adapter_len (integer division).  A byte that is none of
 *   ACGTacgt mismatches every adapter byte: an N in the read is a mismatch.  An occurrence never runs across a line end, and only
 *   line 2 is compared (ACGT are legal quality and header bytes).
 * The output record is line 1, bytes [s, e) of line 2, line 3, bytes [s, e) of line 4, each with the '\n' it had (the last line of a
 *   text without a final '\n' still lacks it; where THAT line is cut to nothing the result ends in an empty line without a line end,
 *   which no reader can tell from no line -- the texts of a decode end in '\n').  Records stay in step, so the pair split, the pair window and the pick run unchanged on
 *   a trimmed text.  The result is never larger than the text: out_cap = n always suffices.  With every term off it is the text. */
typedef struct sfq_trim {
    uint32_t head, tail;          /* 0 = off */
    uint32_t max_len;             /* UINT32_MAX = off; 0 is legal (every base line empty) */
    uint32_t lead_q, trail_q;     /* 0 = off */
    uint32_t win_len;             /* 0 = off, at most 32 */
    uint32_t win_q_x100;
    uint32_t qual_base;           /* <= 126 */
    uint32_t adapter_len;         /* 0 = off, at most 32 */
    uint8_t  adapter[32];         /* 'A' 'C' 'G' 'T' only */
    uint32_t adapter_mm;          /* <= adapter_len */
    uint32_t adapter_min;         /* with an adapter: 1 .. adapter_len */
} sfq_trim;
typedef struct sfq_trim_report {
    uint64_t n_records, n_changed, n_emptied;      /* changed: (s, e) != (0, L); emptied: L > 0 and s == e */
    uint64_t text_bytes, out_bytes, bases_in, bases_out;
    uint64_t n_cut[4];            /* records where lead_q / trail_q / the window / the adapter ALONE cuts a base (a_lead > 0, b_trail < L, b_win < L, b_ad < L); 0 for a term that is off */
} sfq_trim_report;
/* host only, no GPU: SFQ_OK, or SFQ_E_ARG for a null pointer, win_len or adapter_len over 32, an adapter byte outside ACGT,
 * adapter_mm > adapter_len, adapter_min outside 1 .. adapter_len while an adapter is on, or qual_base > 126 */
int sfq_trim_check(const sfq_trim* trim);
/* host only, no GPU: a rule from the CLI's -c SPEC, a comma-separated list of the terms head=N, tail=N, maxlen=N, q5=Q, q3=Q (lead_q,
 * trail_q: integers), win=W:Q (Q a decimal with up to two fraction digits), adapter=SEQ (either case, stored upper case), mm=N and
 * overlap=N (adapter_mm, adapter_min).  *trim: the rule, every term that is not named off, qual_base = 33, mm = 0,
 * overlap = min(3, adapter_len).  SFQ_E_ARG for an unknown term, a bad number, mm or overlap without an adapter, or a rule that
 * sfq_trim_check refuses; err (may be NULL) then says which term. */
int sfq_trim_parse(const char* spec, sfq_trim* trim, char* err, uint64_t err_cap);
/* The records of d_text[0, n), trimmed, into d_out; *out_bytes = the bytes of the result (on SFQ_E_OVERFLOW: the size needed).
 * SFQ_E_ARG: a null pointer (report may be NULL), n == 0, a struct that sfq_trim_check refuses.  SFQ_E_FORMAT: lines that are no
 * multiple of four, or a record whose lines 2 and 4 differ in length -- a trim has no meaning there; sfq_last_error names the smallest
 * such record and its byte offset.  SFQ_E_UNSUPPORTED: a line of 4 GiB or more (or a record whose lines together hold as much).
 * SFQ_E_OVERFLOW: a result larger than out_cap.  Every refusal is decided on the device before the copy: a refused call writes
 * nothing.  A call that succeeds writes d_out[0, *out_bytes) and nothing else.  d_out must not overlap the text.  The call runs on
 * the context's stream and synchronises once.  Like the other side passes, it may read the whole aligned 16-byte units that hold the
 * text's first and last byte. */
int sfq_trim_records(sfq_ctx* ctx, const uint8_t* d_text, uint64_t n, const sfq_trim* trim,
                     uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes, sfq_trim_report* report);
/* trim != NULL: sfq_decode_blocks_host, sfq_decode_block_range_host and sfq_decode_pair_range_host trim the text they decoded (the
 * struct is copied; SFQ_E_ARG, and the setting stays, where sfq_trim_check refuses it); NULL: off (default).  The trim is the FIRST
 * pass behind the checksum pass: the CRCs, installed ones included, stay those of the decoded text.  It runs in front of the selection,
 * of the pair split or the pair window's cut, and of the pick: all of them see an ordinary FASTQ text whose record numbering is
 * unchanged, and a selection's min_len judges the trimmed length.  out_cap keeps sizing the DECODED text.  Costs one more device
 * buffer of the text's size, held while the switch is on.  The device-pointer decode entries are not affected.  Default off: nothing
 * is launched, allocated or copied that is not today. */
int sfq_ctx_set_trim(sfq_ctx* ctx, const sfq_trim* trim);
/* 1: the last decode call trimmed, *out = what it found; 0: it did not (*out zeroed) */
int sfq_get_trim(const sfq_ctx* ctx, sfq_trim_report* out);

/* ---- overlapping mates --------------------------------------------------------------------------------------------------------
 * Adapter removal for pairs WITHOUT knowing the adapter: where the sequenced fragment is shorter than the reads, both mates run
 * through into adapter, read 1 and the reverse complement of read 2 agree over the whole insert, and what lies behind it is
 * read-through.  The pass (ovl.hip) finds that overlap for every pair of an interleaved text while it is on the device, reports the
 * insert sizes, and cuts the read-through.  Text to text like the trimmed records, whose line starts, piece layout and copy it uses.
 * Lines and records: they are sfq_pick_lines' own.  A line ends at '\n'; a text without a final '\n' still ends in a line; '\r' is a
 *   byte like any other.  Lengths exclude the '\n'.
 * For one pair, record X is the first mate and record Y the second: a = line 2 of X, of length La; b = line 2 of Y, of length Lb;
 *   b' = the reverse complement of b: b'[j] = comp(b[Lb-1-j]), A <-> T and C <-> G.  Bases are compared without regard to letter case;
 *   a byte that is none of ACGTacgt, on either side, mismatches everything (the trim pass's convention).
 * Offsets: for an offset d in [-(Lb-1), La-1], position p of a lies against position p-d of b'.
 *   lo = max(0, d), hi = min(La, d + Lb), ov(d) = hi - lo; mm(d) = the number of p in [lo, hi) that mismatch.
 * Acceptance: d is accepted when ov(d) >= min_overlap, mm(d) <= max_mm and 100 * mm(d) <= max_mm_pct * ov(d) (integers).
 * Winner: the accepted d with the largest ov; among those the largest d.  The order is total: the result does not depend on the
 *   order of the search.
 * Insert and cut: the insert is I = d + Lb, 1 <= I <= La + Lb - min_overlap.  With cut set, lines 2 and 4 of X keep their first
 *   min(La, I) bytes and lines 2 and 4 of Y their first min(Lb, I) bytes: what is behind the insert in either read is read-through.
 *   Lines 1 and 3 and every '\n' stay.  NO RECORD IS EVER DROPPED, records stay in step; a pair without an accepted offset is unchanged.
 * Pairs that are not searched: a pair with La or Lb above SFQ_OVERLAP_MAX_LEN passes unchanged and is counted in n_skipped.
 * Range: the pairs are records (first_record + 2k, first_record + 2k + 1) inside [first_record, first_record + n_records);
 *   n_records = UINT64_MAX: to the last record.  Records outside the range are copied unchanged. */
#define SFQ_OVERLAP_MAX_LEN 512
typedef struct sfq_overlap {
    uint64_t first_record, n_records;
    uint32_t min_overlap;    /* 1 .. SFQ_OVERLAP_MAX_LEN */
    uint32_t max_mm;
    uint32_t max_mm_pct;     /* 0 .. 100 */
    uint32_t cut;            /* 0: the text is not changed, the report alone */
} sfq_overlap;
typedef struct sfq_overlap_report {
    uint64_t n_pairs, n_skipped, n_overlap, n_cut;   /* the range's pairs; n_overlap: with an accepted offset; n_cut: pairs that lost a base (with cut == 0: that would) */
    uint64_t text_bytes, out_bytes, bases_in, bases_out, mismatches;  /* bases_*: of the range's records; mismatches: sum of mm(d) of the winners */
    uint64_t insert_hist[2 * SFQ_OVERLAP_MAX_LEN + 1]; /* [I]: searched pairs whose insert is I; [0]: searched, none accepted */
} sfq_overlap_report;
/* host only, no GPU: SFQ_OK, or SFQ_E_ARG for a null pointer, min_overlap outside 1 .. SFQ_OVERLAP_MAX_LEN, max_mm_pct above 100,
 * n_records == 0 */
int sfq_overlap_check(const sfq_overlap* rule);
/* host only, no GPU: a rule from the CLI's -o SPEC, a comma-separated list of the terms min=N (min_overlap, default 30), mm=N (max_mm,
 * default 5), pct=N (max_mm_pct, default 20) and nocut (cut = 0, default 1), or the single word `default`.  *rule: the rule, the range
 * (0, UINT64_MAX).  SFQ_E_ARG for an unknown term, a bad number, an empty list or a rule that sfq_overlap_check refuses; err (may be
 * NULL) then says which. */
int sfq_overlap_parse(const char* spec, sfq_overlap* rule, char* err, uint64_t err_cap);
/* The pairs of d_text[0, n), searched, and with rule->cut the text with the read-through cut into d_out; *out_bytes = the bytes of the
 * result (on SFQ_E_OVERFLOW: the size needed).  With cut == 0 d_out may be NULL, nothing is written and *out_bytes = n.
 * SFQ_E_ARG: a null pointer (report may be NULL), n == 0, a struct that sfq_overlap_check refuses, a range that ends behind the last
 * record.  SFQ_E_FORMAT: lines that are no multiple of four, an odd number of records in the range, or a record of the range whose
 * lines 2 and 4 differ in length; sfq_last_error names the smallest such record and its byte offset.  SFQ_E_UNSUPPORTED: a line of
 * 4 GiB or more.  SFQ_E_OVERFLOW: a result larger than out_cap (never with out_cap >= n).  Every refusal is decided on the device
 * before the copy: a refused call writes nothing.  A call that succeeds writes d_out[0, *out_bytes) and nothing else.  d_out must not
 * overlap the text.  The call runs on the context's stream and synchronises once.  Like the other side passes, it may read the whole
 * aligned 16-byte units that hold the text's first and last byte. */
int sfq_overlap_pairs(sfq_ctx* ctx, const uint8_t* d_text, uint64_t n, const sfq_overlap* rule,
                      uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes, sfq_overlap_report* report);
/* rule != NULL: sfq_decode_blocks_host, sfq_decode_block_range_host and sfq_decode_pair_range_host search the pairs of the text they
 * decoded (the struct is copied; SFQ_E_ARG, and the setting stays, where sfq_overlap_check refuses it); NULL: off (default).  The pass
 * runs BEHIND the trim and IN FRONT OF the selection: a selection's min_len judges the cut length; the split, the pair window's cut and
 * the pick then run unchanged.  sfq_decode_pair_range_host supplies the range itself, the window's pairs; the struct's own range must
 * then be (0, UINT64_MAX), else SFQ_E_ARG.  The CRCs stay those of the decoded text.  With cut == 0 no buffer is reserved and no copy
 * is made; with cut != 0 the pass costs one more device buffer of the text's size, held while the switch is on.  The device-pointer
 * decode entries are not affected.  Default off: nothing is launched, allocated or copied that is not today. */
int sfq_ctx_set_overlap(sfq_ctx* ctx, const sfq_overlap* rule);
/* 1: the last decode call searched its pairs, *out = what it found; 0: it did not (*out zeroed) */
int sfq_get_overlap(const sfq_ctx* ctx, sfq_overlap_report* out);

/* ---- merged mates ---------------------------------------------------------------------------------------------------------------
 * What users of short-insert paired data do next: a pair whose mates overlap becomes ONE read, the fragment itself (fastp --merge,
 * PEAR, FLASH, BBMerge).  The pass (mrg.hip) runs the search of "overlapping mates" above and writes, for every pair that has an
 * accepted offset, one merged record; the other pairs follow whole.  Lines, records, pairs, a, b, b', offsets, acceptance and the
 * winner d are exactly those of "overlapping mates"; SFQ_OVERLAP_MAX_LEN applies as well.
 * Which pairs merge: a pair of the range merges if and only if it is searched and has an accepted offset.  Every other pair of the
 *   range is unmerged, pairs that are not searched (a mate above SFQ_OVERLAP_MAX_LEN) included.
 * The merged record of a pair (X, Y) with winner d, I = d + Lb: line 1 of X with its '\n'; I merged bases and a '\n'; line 3 of X with
 *   its '\n'; I merged quality bytes and a '\n'.  It always ends in '\n', even where the text does not, and is never longer than
 *   its pair: out_cap = n always suffices.
 * The merged position p in [0, I), j = p - d: p lies in a when p < La, in b' when 0 <= j < Lb; at least one holds.
 *   x = a[p], qx = line4X[p]; yb = b[Lb-1-j], qy = line4Y[Lb-1-j]; y = the upper-case complement of yb where yb is one of ACGTacgt
 *   ("valid"), else y = yb unchanged.
 *     in a only                             x (as it is, case included)   qx
 *     in b' only                            y                             qy
 *     both valid, upper(x) == y             x                             max(qx, qy)
 *     both valid, they differ, qx >= qy     x                             qual_base + min(max(|qx - qy|, 2), 126 - qual_base)
 *     both valid, they differ, qx <  qy     y                             the same
 *     only x valid                          x                             qx
 *     only yb valid                         y                             qy
 *     neither valid                         x                             qx
 *   The differ formula takes byte values as integers; it never yields '\n', because qual_base >= 33.
 * The result is two parts in one buffer: d_out[0, *merged_bytes) holds the merged records in pair order, d_out[*merged_bytes,
 *   *out_bytes) the unmerged pairs of the range, both records whole and unchanged, in order: an ordinary interleaved text.
 * Range: as sfq_overlap's -- but records outside the range are DROPPED, where sfq_overlap_pairs copies them: copied, an odd
 *   first_record would leave a lone record in front of the pairs of the second part. */
typedef struct sfq_merge {
    uint64_t first_record, n_records;   /* as sfq_overlap's; n_records = UINT64_MAX: to the last record */
    uint32_t min_overlap, max_mm, max_mm_pct;   /* as sfq_overlap's */
    uint32_t qual_base;                 /* 33 .. 124 */
} sfq_merge;
typedef struct sfq_merge_report {
    uint64_t n_pairs, n_skipped, n_merged;   /* the range's pairs; not searched; merged */
    uint64_t text_bytes, out_bytes, merged_bytes;
    uint64_t bases_in, bases_merged;         /* line-2 bytes of the range's records; the sum of I over merged pairs */
    uint64_t mismatches;                     /* sum of mm(d) of the winners, as sfq_overlap_report's */
    uint64_t n_x_wins, n_y_wins;             /* merged positions of the two "differ" rows of the table above */
    uint64_t insert_hist[2 * SFQ_OVERLAP_MAX_LEN + 1];   /* as sfq_overlap_report's */
} sfq_merge_report;
/* host only, no GPU: sfq_overlap_check's refusals, plus qual_base outside 33 .. 124 */
int sfq_merge_check(const sfq_merge* rule);
/* The pairs of d_text[0, n) merged into d_out as described above; *out_bytes = the bytes of the result (on SFQ_E_OVERFLOW: the size
 * needed), *merged_bytes = those of its first part.  Refusals as sfq_overlap_pairs' with cut set, the messages begin "merged mates:".
 * SFQ_E_ARG: a null pointer (report may be NULL), n == 0, a rule that sfq_merge_check refuses, a range that ends behind the last
 * record.  SFQ_E_FORMAT: lines that are no multiple of four, an odd number of records in the range, or a record of the range whose
 * lines 2 and 4 differ in length; sfq_last_error names the smallest such record and its byte offset.  SFQ_E_UNSUPPORTED: a line of
 * 4 GiB or more.  SFQ_E_OVERFLOW: a result larger than out_cap (never with out_cap >= n).  Every refusal is decided on the device
 * before anything is written: a refused call writes nothing.  A call that succeeds writes d_out[0, *out_bytes) and nothing else; the
 * text is never written.  d_out must not overlap the text.  The call runs on the context's stream and synchronises once.  Like the
 * other side passes, it may read the whole aligned 16-byte units that hold the text's first and last byte. */
int sfq_merge_pairs(sfq_ctx* ctx, const uint8_t* d_text, uint64_t n, const sfq_merge* rule, uint8_t* d_out, uint64_t out_cap,
                    uint64_t* out_bytes, uint64_t* merged_bytes, sfq_merge_report* report);
/* rule != NULL: sfq_decode_blocks_host, sfq_decode_block_range_host and sfq_decode_pair_range_host merge the pairs of the text they
 * decoded (the struct is copied; SFQ_E_ARG, and the setting stays, where sfq_merge_check refuses it); NULL: off (default).  Order:
 * the trim, the selection, THE MERGE, the pair split of the unmerged part, the pick.  The selection judges the mates, not the merged
 * read.  The CRCs stay those of the decoded text.  What comes back is [merged part | rest]: *out_bytes is the total, sfq_get_merge
 * gives the merged part's size in the result as handed back; sfq_get_pair_split's *first_bytes and sfq_decode_pair_range_host's *split
 * are offsets into the result as handed back and lie behind the merged part.  The split runs on the rest alone, when the pair-split
 * switch is on or the entry is the pair window; the pick runs on the merged part and on the rest separately, into one buffer, and all
 * boundaries reported are those in the picked result.  An empty part is skipped by the split and by the pick; a call with nothing left
 * returns SFQ_OK and 0 bytes.  sfq_decode_pair_range_host supplies the range itself, the window's pairs; the struct's own range must
 * then be (0, UINT64_MAX), else SFQ_E_ARG.  SFQ_E_ARG at the decode call too where the overlap switch is on as well, or a selection
 * whose pairs is 0.  Costs one more device buffer of the text's size, held while the switch is on.  The device-pointer decode entries
 * are not affected.  Default off: nothing is launched, allocated or copied that is not today. */
int sfq_ctx_set_merge(sfq_ctx* ctx, const sfq_merge* rule);
/* 1: the last decode call merged, *out = what it found, *merged_bytes (may be NULL) = the merged part's bytes in the result as
 * handed back; 0: it did not (both zeroed) */
int sfq_get_merge(const sfq_ctx* ctx, sfq_merge_report* out, uint64_t* merged_bytes);

/* ---- distinct records ---------------------------------------------------------------------------------------------------------
 * The one step of read preparation in which a record's verdict depends on every other record: duplicates dropped, while the text
 * is on the device (dd.hip).  Text to text like the selected records, whose line starts and copy the pass uses; no stream, coder or
 * block format knows of it.  A lock-free hash set in device memory finds the candidates; the keys themselves decide.
 * Lines and records: they are sfq_pick_lines' own.  A line ends at '\n'; a text without a final '\n' still ends in a line; '\r' is a
 *   byte like any other.  Line lengths exclude the '\n'.
 * Key of a record: the bytes of line 2 with 'a'..'z' replaced by 'A'..'Z'.  Every other byte stands as it is ('N', '.', '\r'); an
 *   empty line 2 is a key like any other.  Names and qualities play no part.
 * Units: with pairs == 0 a unit is a record.  With pairs != 0 a unit is the pair (record first_record + 2k, record first_record +
 *   2k + 1) and its key the ORDERED pair (key X, key Y): two pair keys are equal only if X equals X and Y equals Y, lengths included
 *   -- ("AC","G") is not ("A","CG"), and (X,Y) is not (Y,X).
 * Duplicate: a unit of the range is a duplicate if an earlier unit of the same call's range (a smaller record number) has an equal
 *   key, or, with use_set, a unit KEPT by an earlier successful call since the set was created or cleared has an equal key.
 * Equality is byte equality of the keys, decided by comparing the keys, never by a hash alone: a distinct read is never dropped.
 * Result: the units of the range that are no duplicates, whole (four lines a record), in order, with nothing between them.  Records
 *   outside the range are dropped and never enter the set.  The FIRST occurrence is kept, whatever its qualities.  The result is
 *   never larger than the text: out_cap = n always suffices.  Without a set a range always keeps something; with a set that knows
 *   every key nothing is kept: SFQ_OK with *out_bytes = 0 and nothing written.
 * Determinism: the result is a function of the text, the rule and the set's contents, not of scheduling. */
typedef struct sfq_dedup {
    uint64_t first_record, n_records;   /* n_records = UINT64_MAX: to the last record */
    uint32_t pairs;                     /* 0: records stand alone; 1: records first_record + 2k, + 2k + 1 are one unit */
    uint32_t use_set;                   /* != 0: the context's set counts too, and takes the keys of the units kept */
} sfq_dedup;
typedef struct sfq_dedup_report {
    uint64_t n_in_range, n_units, n_kept;   /* n_in_range counts records; n_units and n_kept count units */
    uint64_t n_dup_set;                     /* units whose key an earlier call left in the set */
    uint64_t n_dup_call;                    /* the other duplicates; n_kept + n_dup_set + n_dup_call == n_units */
    uint64_t text_bytes, kept_bytes;
    uint64_t set_keys, set_key_bytes;       /* set contents after the call (0 without a set) */
} sfq_dedup_report;
/* host only, no GPU: SFQ_OK, or SFQ_E_ARG for a null pointer, n_records == 0, pairs > 1, or an odd first_record with pairs */
int sfq_dedup_check(const sfq_dedup* rule);
/* The distinct units of d_text[0, n) into d_out; *out_bytes = the bytes of the result (on SFQ_E_OVERFLOW: the size needed).
 * SFQ_E_ARG: a null pointer (report may be NULL), n == 0, a rule that sfq_dedup_check refuses, a range that ends behind the last
 * record, use_set without a set, or a set whose pairs differs from the rule's.  SFQ_E_FORMAT: lines that are no multiple of four;
 * with pairs, an odd record count in the range.  SFQ_E_UNSUPPORTED: a record of 4 GiB or more, or with pairs a pair whose two keys hold as
 * much together (decided before such a key is read).  SFQ_E_OVERFLOW: a result larger than
 * out_cap.  SFQ_E_NOMEM: with use_set, the new keys do not fit the set's room; sfq_last_error names keys and bytes, needed and free.
 * Every refusal is decided on the device before the copy and before the set is written: a refused call writes nothing and leaves
 * the set exactly as it was.  A call that succeeds writes d_out[0, *out_bytes) and nothing else; the text is never written.  d_out
 * must not overlap the text.  The call runs on the context's stream and synchronises once.  Like the other side passes, it may read
 * the whole aligned 16-byte units that hold the text's first and last byte.  Working memory: like the other side passes the call
 * lays its arrays out BEFORE the records are counted, for one record per 64 bytes of text (or the most records an earlier call on
 * the context met; a text with more runs twice): about 97 bytes of arrays and 16 to 32 bytes of the call's own hash table per such
 * record, which is 1.8 to 2.0 times the text's size in the context's working buffer (the selection's pass takes 1.3 times), kept
 * until the context goes.  The kernels' grids are laid over those arrays; what lies behind the range's units returns at once. */
int sfq_dedup_records(sfq_ctx* ctx, const uint8_t* d_text, uint64_t n, const sfq_dedup* rule,
                      uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes, sfq_dedup_report* report);
/* The ONE set a context holds: room for max_keys keys whose bytes sum to at most max_key_bytes (a pair key's bytes are both mates'),
 * fixed for its life: a slot table of the power of two of at least 2 max_keys 8-byte slots, 8 bytes (pairs: 12) a key and the key
 * bytes, all in device memory.  pairs: the kind of rule that may use it.  SFQ_E_ARG if a set exists already, a capacity is 0,
 * max_keys is 2^39 or more, max_key_bytes 2^46 (64 TiB) or more, or pairs > 1; SFQ_E_NOMEM from the allocator (no set then). */
int sfq_dedup_set_create(sfq_ctx* ctx, uint64_t max_keys, uint64_t max_key_bytes, uint32_t pairs);
/* empties the set and keeps its memory; SFQ_E_ARG without a set */
int sfq_dedup_set_clear(sfq_ctx* ctx);
/* destroys the set (SFQ_OK without one); sfq_ctx_destroy does it too */
int sfq_dedup_set_destroy(sfq_ctx* ctx);
/* 1 and the set's contents and capacities (every pointer may be NULL), or 0 where there is no set (all zeroed) */
int sfq_dedup_set_info(const sfq_ctx* ctx, uint64_t* keys, uint64_t* key_bytes, uint64_t* max_keys, uint64_t* max_key_bytes);
/* rule != NULL: sfq_decode_blocks_host, sfq_decode_block_range_host and sfq_decode_pair_range_host hand back the distinct units of
 * the text they decoded (the struct is copied; SFQ_E_ARG, and the setting stays, where sfq_dedup_check refuses it); NULL: off
 * (default).  Order: the trim, the overlap, the selection, THE DEDUP, the merge, the pair split or the window's cut, the pick.  The
 * dedup judges what the selection kept, at its trimmed or cut length; the merge and the split then see an ordinary text.  The CRCs
 * stay those of the decoded text.  out_cap keeps sizing the DECODED text.  Costs one more device buffer of the text's size, held
 * while the switch is on, and sfq_dedup_records' working memory (above) in the buffer the passes share.  With use_set the calls share the context's set: duplicates are found across calls (segments).
 * SFQ_E_ARG at the decode call while the pair split, the merge or a pair window is on and pairs == 0: the mates would fall out of
 * step.  sfq_decode_pair_range_host supplies the range itself, the window's pairs, exactly as it does for the merge; the rule's own
 * range must then be (0, UINT64_MAX), else SFQ_E_ARG.  Where a selection ran in front, it has cut the range already.  With
 * nothing kept (only with a set) the _host entries return SFQ_OK and 0 bytes, and the passes behind are skipped.  The
 * device-pointer decode entries are not affected.  Default off: nothing is launched, allocated or copied that is not today. */
int sfq_ctx_set_dedup(sfq_ctx* ctx, const sfq_dedup* rule);
/* 1: the last decode call dropped duplicates, *out = what it found; 0: it did not (*out zeroed) */
int sfq_get_dedup(const sfq_ctx* ctx, sfq_dedup_report* out);

/* ---- screened records ---------------------------------------------------------------------------------------------------------
 * Reads screened against reference sequences while the text is on the device (scr.hip): the reads that share k-mers with phiX, an
 * adapter, rRNA or a host genome dropped -- or, the other way round, only the reads that hit a bait kept.  Text to text like the
 * distinct records, whose line starts and copy the pass uses; no stream, coder or block format knows of it.
 * Lines and records: they are sfq_pick_lines' own.  A line ends at '\n'; a text without a final '\n' still ends in a line; '\r' is a
 *   byte like any other.
 * Codes: 'A' 'a' 0, 'C' 'c' 1, 'G' 'g' 2, 'T' 't' 3.  Every other byte is a BREAK: 'N', '.', '\r', '\n', '>', and so on.
 * Window: k consecutive bytes of one sequence, none of them a break, 4 <= k <= 31.  Its forward value is the sum of
 *   code(b[j]) * 4^(k-1-j); its reverse-complement value that of the reversed window with the codes 3 - c; its CANONICAL value the
 *   smaller of the two.  A palindromic window has both equal: it is one window and one k-mer.
 * Sequence text (what a reference is to the library): any bytes.  Its windows are all runs of k bytes without a break; a '\n' or any
 *   other break separates sequences.  Nothing else is parsed (sfq_fasta_sequences makes one of a FASTA file).
 * Set: the canonical values of all windows of all sequence texts added since it was created or cleared.  It is a set: a k-mer added
 *   twice is in it once.  Membership is exact: the whole value is stored, no fingerprint, and there are no false positives.
 * Read: for a record, W is the number of windows of line 2 and H the number of them whose canonical value is in the set.  H counts by
 *   position: a k-mer of the set that occurs three times in the read counts three.  Headers, '+' lines and qualities play no part; a
 *   window never crosses a line end.
 * Matched: a record is matched when H >= min_hits AND 100 * H >= min_pct * W, in 64-bit arithmetic.  min_hits >= 1: a read without a
 *   window is never matched.
 * Units: pairs == 0: a unit is a record, matched when the record is.  pairs == 1: a unit is the records first_record + 2k and
 *   + 2k + 1 together, matched when EITHER mate is; pairs == 2: the same two records, matched when BOTH mates are.
 * Kept: a unit of the range is kept when (matched) == (keep_matched != 0): keep_matched = 0 decontaminates, 1 baits.
 * Result: the kept units whole (four lines a record), in order, with nothing between them; records outside the range are dropped.
 *   The result is never larger than the text: out_cap = n always suffices.  With nothing kept: SFQ_OK, *out_bytes = 0, nothing written.
 * Determinism: the result is a function of the text, the rule and the set's contents AS A SET, never of scheduling or slot order. */
typedef struct sfq_screen {
    uint64_t first_record, n_records;   /* n_records = UINT64_MAX: to the last record */
    uint32_t pairs;                     /* 0, 1 (either mate), 2 (both mates) */
    uint32_t min_hits;                  /* >= 1 */
    uint32_t min_pct;                   /* 0 .. 100 */
    uint32_t keep_matched;              /* 0: drop the matched units; else keep only them */
} sfq_screen;
typedef struct sfq_screen_report {
    uint64_t n_in_range, n_units, n_kept;   /* n_in_range counts records; n_units and n_kept count units */
    uint64_t n_matched_records;             /* the range's records that are matched, each by itself whatever pairs says */
    uint64_t n_windows, n_hits;             /* the sums of W and H over the range's records */
    uint64_t text_bytes, kept_bytes, set_kmers;
} sfq_screen_report;
/* host only, no GPU: SFQ_OK, or SFQ_E_ARG for a null pointer, n_records == 0, pairs > 2, an odd first_record with pairs, min_hits == 0
 * or min_pct > 100 */
int sfq_screen_check(const sfq_screen* rule);
/* host only: a rule and k from the terms of the CLI's -G: "k=N" (4 .. 31, default 27), "hits=N" (default 1), "pct=N" (0 .. 100, default
 * 0), "keep" (keep_matched = 1), "both" (pairs = 2), "either" (pairs = 1), separated by commas; a term "ref=..." is the CLI's own and is
 * skipped.  Without "both" and "either" pairs stays 0: the caller knows whether records are pairs.  The range is (0, UINT64_MAX).
 * SFQ_OK, or SFQ_E_ARG with a message in err[0, err_cap) (err may be NULL). */
int sfq_screen_parse(const char* spec, sfq_screen* rule, uint32_t* k, char* err, uint64_t err_cap);
/* host only: a FASTA file's bytes as a sequence text.  A line whose first byte is '>' becomes a single '\n', the break between two
 * records; every other line is copied without its '\n' and without a '\r' in front of it, so that k-mers run across the wrapped lines
 * of one record and never across two records.  Returns the size of the result, never larger than n; out == NULL: the size only;
 * SFQ_E_OVERFLOW where it is larger than cap (nothing is written then), SFQ_E_ARG for fasta == NULL with n != 0. */
int64_t sfq_fasta_sequences(const uint8_t* fasta, uint64_t n, uint8_t* out, uint64_t cap);
/* The ONE set of k-mers a context holds: a table of the power of two of at least 2 max_kmers 8-byte slots in device memory, fixed for
 * its life.  A slot is 0 or 2^63 | the canonical value; a k-mer's home slot is (canonical * 0x9E3779B97F4A7C15 mod 2^64) >> (64 -
 * log2(slots)), probing is linear.  SFQ_E_ARG if a set exists already, k is outside 4 .. 31, max_kmers is 0 or 2^39 or more;
 * SFQ_E_NOMEM from the allocator (no set then). */
int sfq_screen_set_create(sfq_ctx* ctx, uint32_t k, uint64_t max_kmers);
/* Adds the windows of the sequence text h_seq[0, n), HOST bytes.  The library copies them up in pieces of 4 MiB that overlap by k - 1
 * bytes: the windows are those of the whole text however it is cut.  Windows never span two CALLS: a call's text ends in a break.
 * SFQ_E_ARG: no set, h_seq == NULL, n == 0.  SFQ_E_NOMEM: the set would hold more than max_kmers k-mers (or a probe found no slot);
 * the library then CLEARS the set: a refused add leaves the set EMPTY, not half-filled. */
int sfq_screen_set_add(sfq_ctx* ctx, const uint8_t* h_seq, uint64_t n);
/* empties the set and keeps its memory; SFQ_E_ARG without a set */
int sfq_screen_set_clear(sfq_ctx* ctx);
/* destroys the set (SFQ_OK without one); sfq_ctx_destroy does it too */
int sfq_screen_set_destroy(sfq_ctx* ctx);
/* 1 and the set's k, contents and capacity (every pointer may be NULL), or 0 where there is no set (all zeroed) */
int sfq_screen_set_info(const sfq_ctx* ctx, uint32_t* k, uint64_t* kmers, uint64_t* max_kmers);
/* The kept units of d_text[0, n) into d_out; *out_bytes = the bytes of the result (on SFQ_E_OVERFLOW: the size needed).
 * SFQ_E_ARG: a null pointer (report may be NULL), n == 0, a rule that sfq_screen_check refuses, a range that ends behind the last
 * record, no set.  SFQ_E_FORMAT: lines that are no multiple of four; with pairs, an odd record count in the range.
 * SFQ_E_UNSUPPORTED: a record of 4 GiB or more (decided before its line is walked).  SFQ_E_OVERFLOW: a result larger than out_cap.
 * Every refusal is decided on the device before the copy: a refused call writes nothing.  A call that succeeds writes
 * d_out[0, *out_bytes) and nothing else; the text is never written and the set is never written by a screening call.  d_out must not
 * overlap the text.  The call runs on the context's stream and synchronises once.  Like the other side passes, it may read the whole
 * aligned 16-byte units that hold the text's first and last byte.  Working memory: like the other side passes the call lays its arrays
 * out BEFORE the records are counted, for one record per 64 bytes of text (or the most records an earlier call on the context met; a
 * text with more runs twice): 76 bytes of arrays per such record, which with the line counts' scratch is 1.2 to 1.3 times the text's size in the context's
 * working buffer (the selection's pass takes 1.3 times), kept until the context goes.  The kernels' grids are laid over those arrays; what lies behind
 * the range's records returns at once. */
int sfq_screen_records(sfq_ctx* ctx, const uint8_t* d_text, uint64_t n, const sfq_screen* rule,
                       uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes, sfq_screen_report* report);
/* rule != NULL: sfq_decode_blocks_host, sfq_decode_block_range_host and sfq_decode_pair_range_host hand back the kept units of the text
 * they decoded (the struct is copied; SFQ_E_ARG, and the setting stays, where sfq_screen_check refuses it); NULL: off (default).
 * Order: the trim, the overlap, the selection, THE SCREEN, the dedup, the merge, the pair split or the window's cut, the pick.  The
 * screen judges what the selection kept, at its trimmed or cut length; a contaminant never enters the dedup's set.  The CRCs stay
 * those of the decoded text.  out_cap keeps sizing the DECODED text.  Costs one more device buffer of the text's size, held while the
 * switch is on, and sfq_screen_records' working memory (above) in the buffer the passes share.  SFQ_E_ARG at the decode call where the
 * context holds no set, and while the pair split, the merge or a pair window is on and pairs == 0: the mates would fall out of step.
 * sfq_decode_pair_range_host supplies the range itself, the window's pairs; the rule's own range must then be (0, UINT64_MAX), else
 * SFQ_E_ARG.  Where a selection ran in front, it has cut the range already.  With nothing kept the _host entries return SFQ_OK and 0
 * bytes, and the passes behind are skipped.  The device-pointer decode entries are not affected.  Default off: nothing is launched,
 * allocated or copied that is not today. */
int sfq_ctx_set_screen(sfq_ctx* ctx, const sfq_screen* rule);
/* 1: the last decode call screened, *out = what it found; 0: it did not (*out zeroed) */
int sfq_get_screen(const sfq_ctx* ctx, sfq_screen_report* out);

/* ---- demultiplexed records ----------------------------------------------------------------------------------------------------
 * The first step of read preparation: a lane's reads split by SAMPLE, while the text is on the device (dmx.hip).  A unit carries a
 * barcode in the index field of its header ("... 1:N:0:ATCACG", "...:ATCACG+TTAGGC") or inline at the start of its bases; the unit goes
 * to the sample whose barcode is nearest, within a mismatch allowance.  Text to text like the distinct records, whose line starts and
 * copy the pass uses; no stream, coder or block format knows of it.  Unlike every other pass it does not keep or drop records in
 * place: it is a stable multi-way partition.
 * Lines and records: they are sfq_pick_lines' own.  A line ends at '\n'; '\r' is a byte like any other.  Line lengths exclude the '\n'.
 * Units: with pairs == 0 a unit is a record.  With pairs == 1 a unit is (record first_record + 2k, record first_record + 2k + 1),
 *   mate 0 and mate 1.  The range is (first_record, n_records), n_records = UINT64_MAX: to the last record.  Records outside the
 *   range are dropped.
 * Barcode parts: a sample's barcode has one or two parts, part 0 then part 1, of len0 + len1 = B bases, 1 <= B <= 32, len0 >= 1;
 *   part 1 is ABSENT where its len is 0 (its other fields are then not looked at).  A part says where its observed bytes come from:
 *   SFQ_DEMUX_HEADER: of line 1 of the unit's record `mate`.  F = the bytes of line 1 behind its LAST ':'.  Subfield 0 = F up to its
 *     first '+', or all of F without one; subfield 1 = what lies behind that '+'.  The observed bytes are subfield[sub][pos, pos + len);
 *     what lies behind them is ignored.  The part is SHORT when line 1 holds no ':', when sub == 1 and F holds no '+', or when the
 *     subfield has fewer than pos + len bytes.
 *   SFQ_DEMUX_BASES: the observed bytes are line2[pos, pos + len) of the unit's record `mate`; the part is SHORT where line 2 is
 *     shorter than pos + len.  sub must be 0.
 * Distance: the comparison ignores letter case; an observed byte that is none of ACGTacgt mismatches every barcode base (the trim's
 *   convention).  d(s) = the mismatching positions among all B positions of sample s (part 0's, then part 1's).
 * Verdict of a unit, in this order: SHORT: some part is short.  Otherwise m = min over s of d(s).  FAR: m > max_mm.  AMBIGUOUS:
 *   m <= max_mm and two or more samples attain m.  ASSIGNED to s: exactly one s attains m <= max_mm; PERFECT: assigned with m == 0.
 *   Every unit that is not assigned goes to the UNASSIGNED part.
 * Clip (clip != 0): of an ASSIGNED unit, record R loses the first c_R bytes of its lines 2 and 4, c_R = the largest pos + len among
 *   the SFQ_DEMUX_BASES parts read from R (0 where there is none).  Lines 1 and 3 and every '\n' stay.  Unassigned units are never
 *   clipped.  With clip a record of the range whose lines 2 and 4 differ in length is SFQ_E_FORMAT (sfq_last_error names the
 *   smallest such record and its byte offset, as the trim does).  bases_clipped = the bytes that the lines 2 lost.
 * Result: ONE buffer of NP parts back to back with nothing between them.  Without split_mates NP = n_samples + 1: part s < n_samples
 *   holds sample s's units, part n_samples the unassigned ones.  With pairs and split_mates NP = 2 (n_samples + 1): part 2 s holds the
 *   first mates and part 2 s + 1 the second mates of what part s would be.  Inside every part the records are whole (but for the
 *   clip) and in their original order.  part_off[0 .. NP] are the boundaries, part_off[0] = 0, part_off[NP] = *out_bytes;
 *   part_units[0 .. n_samples] the units of every sample, the unassigned last.  The result is never larger than the text: out_cap = n
 *   always suffices.
 * Final line end: a text that does not end in '\n' is SFQ_E_FORMAT -- its last record may land in the middle of the result (as
 *   sfq_interleave refuses an A that does not end in one).  A decode's texts end in '\n'.
 * Order of the refusals: the lines' count, the final '\n', the range, an odd count under pairs, a record of 4 GiB, the clip's unequal
 *   lines, the output's room.
 * Determinism: the result is a function of the text, the rule and the barcodes, never of scheduling: no atomic decides a place. */
#define SFQ_DEMUX_HEADER 1
#define SFQ_DEMUX_BASES  2
#define SFQ_DEMUX_MAX_SAMPLES 4096
typedef struct sfq_demux_part { uint32_t src, mate, sub, pos, len; } sfq_demux_part;
/* src: SFQ_DEMUX_HEADER | SFQ_DEMUX_BASES; mate: 0 / 1, which record of the unit (0 without pairs) */
typedef struct sfq_demux {
    uint64_t first_record, n_records;   /* n_records = UINT64_MAX: to the last record */
    uint32_t pairs, split_mates, max_mm, clip;
    sfq_demux_part part[2];
    uint32_t n_samples, reserved;       /* 1 .. SFQ_DEMUX_MAX_SAMPLES */
} sfq_demux;
typedef struct sfq_demux_report {
    uint64_t n_in_range, n_units, n_assigned, n_perfect, n_short, n_far, n_ambiguous;   /* assigned + short + far + ambiguous == units */
    uint64_t text_bytes, out_bytes, bases_clipped;
} sfq_demux_report;
/* host only, no GPU.  h_barcodes: n_samples rows of B = part[0].len + part[1].len bytes, part 0's bases then part 1's.  SFQ_OK, or
 * SFQ_E_ARG for a null pointer, n_records == 0, pairs > 1, an odd first_record with pairs, split_mates without pairs, a mate != 0
 * without pairs or > 1, a sub > 1 or != 0 on a SFQ_DEMUX_BASES part, an unknown src, pos + len beyond 32 bits, part[0].len == 0, B
 * outside 1 .. 32, max_mm > B, n_samples outside 1 .. SFQ_DEMUX_MAX_SAMPLES, a barcode byte outside ACGT (upper case), two equal rows. */
int sfq_demux_check(const sfq_demux* rule, const uint8_t* h_barcodes);
/* host only: the terms of the CLI's -X into *rule: "SHEET[,term...]".  The FIRST term is the sample sheet's path and is skipped, as are
 * the file terms out=PREFIX and counts=FILE.  mm=N: max_mm (default 1); hdr (the default): part 0 from header subfield 0, part 1
 * from header subfield 1; inline[=POS]: part 0 from mate 0's bases at POS (default 0); inline2[=POS]: with inline, part 1 from mate
 * 1's bases; hdr2: with inline, part 1 from header subfield 0; clip.  The parts' lengths are left 0: they are the sheet's; the range
 * is (0, UINT64_MAX), pairs, split_mates and n_samples 0.  SFQ_E_ARG for a null pointer, an unknown term, a bad number, hdr with inline,
 * inline2 or hdr2 without inline, or both; err (may be NULL) then says which. */
int sfq_demux_parse(const char* spec, sfq_demux* rule, char* err, uint64_t err_cap);
/* host only: a sample sheet text[0, n).  Lines end at '\n' (a '\r' in front of it is dropped); empty lines and lines that begin with
 * '#' are skipped.  A data line is name<TAB>BARCODE, name<TAB>BARCODE0+BARCODE1 or name<TAB>BARCODE0<TAB>BARCODE1; barcodes in
 * either case of ACGT, stored upper case.  All rows have the same len0 >= 1 and len1 (0: one part), len0 + len1 <= 32.  Names are 1 ..
 * 64 bytes of [A-Za-z0-9._-], unique, none equal to "unassigned".  names_out: max_samples rows of 65 bytes, NUL-terminated;
 * barcodes_out: max_samples rows of 32 bytes' room, of which the first n_samples * (len0 + len1) are written: row s at s * (len0 +
 * len1), what sfq_demux_check and sfq_demux_records take.  SFQ_E_ARG for a null pointer (err may be NULL), max_samples == 0, a sheet
 * without data lines or with more than min(max_samples, SFQ_DEMUX_MAX_SAMPLES), a malformed line, a bad name, unequal lengths, a
 * duplicate name or barcode; err then names the line, counted from 1. */
int sfq_demux_sheet(const char* text, uint64_t n, uint32_t max_samples, char* names_out, uint8_t* barcodes_out,
                    uint32_t* n_samples, uint32_t* len0, uint32_t* len1, char* err, uint64_t err_cap);
/* The units of d_text[0, n) by sample into d_out; *out_bytes = the bytes of the result (on SFQ_E_OVERFLOW: the size needed).
 * part_off: host, NP + 1 entries; part_units: host, n_samples + 1 entries, may be NULL; report may be NULL.
 * SFQ_E_ARG: a null pointer, n == 0, what sfq_demux_check refuses, a range that ends behind the last record.  SFQ_E_FORMAT: lines
 * that are no multiple of four, a text without a final '\n', with pairs an odd record count in the range, with clip a record whose
 * lines 2 and 4 differ in length.  SFQ_E_UNSUPPORTED: a record of 4 GiB or more.  SFQ_E_OVERFLOW: a result larger than out_cap.
 * Every refusal is decided on the device before the copy: a refused call writes nothing to d_out.  A call that succeeds writes
 * d_out[0, *out_bytes) and nothing else; the text is never written.  d_out must not overlap the text; both may lie at any byte
 * alignment.  The call runs on the context's stream and synchronises once.  Like the other side passes, it may read the whole aligned
 * 16-byte units that hold the text's first and last byte.  All offsets are 64-bit.  Working memory: like the other side passes the
 * call lays its arrays out BEFORE the records are counted, for one record per 64 bytes of text (or the most records an earlier call on
 * the context met; a text with more runs twice): about 75 bytes per such record, with clip 127 -- 1.2 and 2.0 times the text's size in
 * the context's working buffer, whatever n_samples is: the partition sorts by digits of the class and keeps 256 counters per 1024
 * records, not a counter per tile and class. */
int sfq_demux_records(sfq_ctx* ctx, const uint8_t* d_text, uint64_t n, const sfq_demux* rule, const uint8_t* h_barcodes,
                      uint8_t* d_out, uint64_t out_cap, uint64_t* out_bytes, uint64_t* part_off, uint64_t* part_units,
                      sfq_demux_report* report);
/* rule != NULL: sfq_decode_blocks_host and sfq_decode_block_range_host hand back the PARTITIONED text of what they decoded (rule and
 * barcodes are copied; SFQ_E_ARG, and the setting stays, where sfq_demux_check refuses them); NULL: off (default).  Order: the trim,
 * the overlap, the selection, the screen, the dedup, THE DEMUX: it is the call's last pass.  The CRCs stay those of the decoded text.
 * out_cap keeps sizing the DECODED text.  Costs one more device buffer of the text's size, held while the switch is on, and
 * sfq_demux_records' working memory (above) in the buffer the passes share.  SFQ_E_ARG at the decode call while the merge, the pick
 * or the pair split is on, and from sfq_decode_pair_range_host (split_mates is the split; the others are not combined with the
 * demux); SFQ_E_ARG too where a selection, a screen or a dedup in front has pairs == 0 and the demux pairs == 1, or the other way
 * round: the mates would fall out of step.  With nothing left by a pass in front the _host entries return SFQ_OK and 0 bytes as
 * they do today, and sfq_get_demux answers 0.  The device-pointer decode entries are not affected.  Default off: nothing is
 * launched, allocated or copied that is not today. */
int sfq_ctx_set_demux(sfq_ctx* ctx, const sfq_demux* rule, const uint8_t* h_barcodes);
/* 1: the last decode call demultiplexed: *report (may be NULL) = what it found, part_off[0 .. NP] and part_units[0 .. n_samples] (either
 * may be NULL) as sfq_demux_records gives them, where cap_entries >= NP + 1; 0: it did not (*report zeroed).  SFQ_E_ARG for a null context
 * and for a cap_entries below NP + 1 with either array given: the context is const here as for the sibling getters, so this refusal
 * leaves no message and sfq_last_error keeps what it said before. */
int sfq_get_demux(const sfq_ctx* ctx, sfq_demux_report* report, uint64_t* part_off, uint64_t* part_units, uint64_t cap_entries);

/* ---- BGZF: blocked gzip, deflated on the GPU (bgz.hip) --------------------------
 * A text in device memory as BGZF (the SAM specification's blocked gzip, what bgzip writes): a plain concatenation of gzip members,
 * which every gzip reader reads.  The text is given in parts, as sfq_crc32 takes its ranges; every part is cut into pieces of
 * SFQ_BGZF_PIECE bytes (the last may be shorter), a piece is one member, and no member crosses a part's bound -- the result can be cut
 * where the parts meet.  A part of zero bytes has no member.  A member is 18 header bytes (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6,
 * 'B' 'C' 02 00, BSIZE = the member's size - 1), one raw deflate stream -- one dynamic-Huffman block over an LZ77 parse of the piece, or
 * one stored block where that would be larger than the piece + 5 bytes -- the piece's CRC-32 and its size.  The same piece gives the
 * same member whatever else the call holds and wherever the piece lies in memory.  The pass writes no end-of-file block: a file ends
 * with sfq_bgzf_eof's 28 bytes, written once by whoever closes it. */
#define SFQ_BGZF_PIECE 65280
typedef struct sfq_bgzf_report {
    uint64_t text_bytes;       /* the text's */
    uint64_t out_bytes;        /* the result's; on SFQ_E_OVERFLOW the size needed */
    uint64_t members;
    uint64_t stored_members;   /* of them, those that hold a stored block */
} sfq_bgzf_report;
/* what the members of n bytes of text in n_parts parts hold at most: n + 31 * (n / 65280 + n_parts) */
uint64_t sfq_bgzf_bound(uint64_t n, uint32_t n_parts);
/* the specification's empty member, which ends a file; returns 28 */
int sfq_bgzf_eof(uint8_t out[28]);
/* Part i of the text is d_text[h_bounds[i], h_bounds[i + 1]), i < n_parts; part i of the result is d_out[h_part_off[i],
 * h_part_off[i + 1]).  The contract is sfq_pick_lines': any alignment of d_text and d_out; SFQ_E_ARG for a null pointer, n_parts == 0
 * or decreasing bounds; SFQ_E_OVERFLOW with the size needed in report->out_bytes where the result exceeds out_cap, decided before
 * anything is written to d_out; a successful call writes d_out[0, report->out_bytes) and nothing else; d_out must not overlap the
 * text; one synchronise; reads may extend to the aligned 16-byte units of the text's ends.  A text of zero bytes is fine: no member,
 * every offset 0.  report may be NULL. */
int sfq_bgzf_deflate(sfq_ctx* ctx, const uint8_t* d_text, const uint64_t* h_bounds, uint32_t n_parts, uint8_t* d_out, uint64_t out_cap,
                     uint64_t* h_part_off /* n_parts + 1 */, sfq_bgzf_report* report);
/* on != 0: sfq_decode_blocks_host, sfq_decode_block_range_host and sfq_decode_pair_range_host hand back BGZF bytes instead of text.
 * It is the call's last pass, behind everything, the pick and the demultiplexing included, and its parts are what that exit has: one
 * text; first mates | second mates; merged | rest (the rest's mates split: three parts); the demultiplexing's parts.  Every byte
 * offset into the returned buffer -- *split, sfq_get_pair_split's first_bytes, sfq_get_demux's part_off, sfq_get_merge's merged_bytes --
 * becomes an offset into the compressed result; record and unit counts do not change, and checksums stay those of the decoded text.
 * out_cap keeps sizing the decoded text; a result larger than out_cap (text that does not compress) is SFQ_E_OVERFLOW with the size
 * needed in *out_bytes.  A call whose passes keep nothing returns 0 bytes, as without the switch.  While it is on the context holds a
 * device buffer of 65536 bytes per member (1.004 bytes per byte of text) and the tokens' buffer (four bytes per byte of the pieces in
 * flight, 134 MB on a 256-CU device whatever the text's size).  The device-pointer decode entries are not affected.  Default off:
 * nothing is launched, allocated or copied that is not today. */
int sfq_ctx_set_bgzf(sfq_ctx* ctx, int on);
/* 1: the last decode call deflated: *report (may be NULL), part_off[0 .. NP] = the parts' offsets in the returned bytes and
 * text_part_bytes[0 .. NP) = the text-side sizes of the same parts (either may be NULL), where cap >= NP + 1; 0: it did not (*report
 * zeroed).  SFQ_E_ARG for a null context and for a cap below NP + 1 with either array given. */
int sfq_get_bgzf(const sfq_ctx* ctx, sfq_bgzf_report* report, uint64_t* part_off, uint64_t* text_part_bytes, uint64_t cap);

/* ---- the ".sfq" container (host only) ----------------------------------------------------------
 * Replaces FilerSave + the info page (filer.cpp:217-242, config.cpp:334-347) for hosts that assemble an archive
 * themselves: info_text is the info page ("key=value\n" lines), then n_streams named byte streams (names of at most
 * 8 bytes: filer.cpp:42-47).  A block-format archive of several calls' results: sfq_archive_write_segments below. */
int sfq_archive_write(const char* path, const char* info_text, uint32_t n_streams,
                      const char* const* names, const uint8_t* const* data, const uint64_t* sizes);
/* The "blk.idx" stream of a block-format archive from a block index; returns its size (out == NULL: size only). */
int64_t sfq_pack_block_index(const sfq_block_info* blocks, uint32_t n, uint8_t* out, uint64_t cap);

/* One encode call's results, as they are to be stored: ONE SEGMENT of a block-format archive.
 * Every pointer may be NULL where its size is 0. */
typedef struct sfq_segment {
    const uint8_t* streams[SFQ_NSTREAMS];  /* the call's part of every stream (sfq_result.stream_offset / stream_bytes) */
    uint64_t stream_bytes[SFQ_NSTREAMS];
    const sfq_block_info* blocks;          /* sfq_get_block_index */
    uint32_t n_blocks, reserved;
    const uint8_t* first_hdrs;  uint64_t first_hdr_bytes;       /* sfq_get_first_headers */
    const uint8_t* qlt_prior;   uint64_t qlt_prior_bytes;       /* sfq_get_qlt_prior ("qlt.pri") */
    const uint8_t* chain_index; uint64_t chain_index_bytes;     /* sfq_get_chain_index ("chn.idx") */
    const uint8_t* rec_prior;   uint64_t rec_prior_bytes;       /* sfq_get_rec_prior ("rec.pri") */
    uint64_t raw_bytes;                    /* bytes of FASTQ text the call coded */
} sfq_segment;
/* A block-format archive of n segments, in order (the writer rank of a multi-GPU job: one segment per slab of every rank);
 * the layout, info keys and index streams the CLI writes.  tables: SFQ_TABLES_FROZEN or SFQ_TABLES_ADAPTIVE, as the calls
 * coded; shared_prior != 0: a segment without priors of its own decodes from the previous segment's (info key
 * "seg.shared_prior").  Segments without blocks are left out; SFQ_E_ARG if none is left, or if a segment's stream bytes
 * are not what its blocks say. */
int sfq_archive_write_segments(const char* path, const char* orig_name, int level, uint32_t tables, int shared_prior,
                               uint32_t n, const sfq_segment* segs);

/* ---- utilities (host only, no GPU) ----------------------------------------------------------- */
/* Deterministic synthetic FASTQ. kind 0 = 150 bp-style Illumina reads of
 * read_len bases; kind 1 = long reads, lengths log-uniform in [10000, 50000] (read_len ignored);
 * kind 2 = kind 0 with NovaSeq-style 4-level binned qualities; kind 3 = kind 0 with the bases sampled (either
 * strand, 0.5 % substitutions) from a seeded random 10 Mbp genome: 30x coverage at 2 M reads of 150 bp.
 * Returns bytes written, or the required size when h_out == NULL, or <0. */
int64_t sfq_synth_fastq(uint64_t first_read, uint64_t n_reads, uint32_t read_len, uint64_t seed, int kind,
                        uint8_t* h_out, uint64_t cap);
int sfq_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SLIMFASTQ_AMD_H */

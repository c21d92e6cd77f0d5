"""ctypes binding of libslimfastq_amd.so (include/slimfastq_amd.h).  No fallback of any kind."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libslimfastq_amd.so")

NSTREAMS = 14
STREAM_NAMES = ["rec", "gen", "qlt", "gen.Ns", "gen.Nn", "rec.x", "usr.x", "usr.x.q", "usr.pfg", "usr.pfq",
                "gen.lc", "usr.lrec", "usr.lgen", "usr.lqlt"]
M_REC, M_GEN, M_QLT, M_USR, M_ALL = 1, 2, 4, 8, 15
T_FRAME, T_QLT, T_GEN, T_REC, T_USR, T_PACK, T_TOTAL = range(7)
PRIOR_AUTO = 0xFFFFFFFF
PRIOR_GIVEN = 0xFFFFFFFE
PRIOR_COUNTS = 0xFFFFFFFD
BLOCK_AUTO = 0xFFFFFFFF
TABLES_ADAPTIVE, TABLES_FROZEN, TABLES_AUTO = 0, 1, 2
LDS_ROWS_NONE = 0xFFFFFFFF
QMAP_ILLUMINA8, QMAP_NOVASEQ4 = 1, 2
QMAP_PRESETS = {"illumina8": QMAP_ILLUMINA8, "novaseq4": QMAP_NOVASEQ4}
PICK_FASTA, PICK_NAMES, PICK_BASES, PICK_QUALS = 1, 2, 3, 4
PICKS = {"fasta": PICK_FASTA, "names": PICK_NAMES, "bases": PICK_BASES, "quals": PICK_QUALS}
PICK_TO_END = 0xFFFFFFFFFFFFFFFF
SELECT_BOTH, SELECT_EITHER = 1, 2
SELECT_TO_END = 0xFFFFFFFFFFFFFFFF

EXPORTS = [
    "sfq_stream_name", "sfq_ctx_create", "sfq_ctx_destroy", "sfq_last_error", "sfq_ctx_set_table_budget",
    "sfq_ctx_stream", "sfq_ctx_synchronize", "sfq_encode_bound", "sfq_encode_blocks", "sfq_encode_qlt_blocks",
    "sfq_encode_blocks_host", "sfq_get_block_index", "sfq_get_first_headers", "sfq_decode_blocks",
    "sfq_decode_blocks_host", "sfq_synth_fastq", "sfq_abi_version", "sfq_get_qlt_prior", "sfq_set_qlt_prior",
    "sfq_archive_write", "sfq_pack_block_index", "sfq_ctx_device_memory", "sfq_get_chain_index", "sfq_set_chain_index", "sfq_get_rec_prior", "sfq_set_rec_prior", "sfq_build_priors",
    "sfq_host_alloc", "sfq_host_free", "sfq_count_priors", "sfq_prior_counts_words", "sfq_get_prior_counts", "sfq_set_prior_counts",
    "sfq_archive_write_segments", "sfq_crc32", "sfq_crc32_combine", "sfq_ctx_set_checksums", "sfq_get_checksums",
    "sfq_set_block_checksums", "sfq_decode_block_range", "sfq_decode_block_range_host",
    "sfq_ctx_set_stats", "sfq_get_text_stats", "sfq_text_stats_merge", "sfq_pack_text_stats", "sfq_unpack_text_stats",
    "sfq_quality_map_preset", "sfq_quality_map_check", "sfq_map_qualities", "sfq_ctx_set_quality_map", "sfq_get_quality_map_changed",
    "sfq_interleave", "sfq_split_pairs", "sfq_encode_pairs_host", "sfq_ctx_set_pair_split", "sfq_get_pair_split",
    "sfq_split_pairs_range", "sfq_check_mates", "sfq_ctx_set_mate_check", "sfq_get_mate_report", "sfq_pair_window_blocks",
    "sfq_decode_pair_range_host", "sfq_pick_lines", "sfq_ctx_set_pick", "sfq_get_pick",
    "sfq_select_check", "sfq_select_parse", "sfq_select_records", "sfq_ctx_set_select", "sfq_get_select",
    "sfq_trim_check", "sfq_trim_parse", "sfq_trim_records", "sfq_ctx_set_trim", "sfq_get_trim",
    "sfq_overlap_check", "sfq_overlap_parse", "sfq_overlap_pairs", "sfq_ctx_set_overlap", "sfq_get_overlap",
    "sfq_merge_check", "sfq_merge_pairs", "sfq_ctx_set_merge", "sfq_get_merge",
    "sfq_dedup_check", "sfq_dedup_records", "sfq_dedup_set_create", "sfq_dedup_set_clear", "sfq_dedup_set_destroy", "sfq_dedup_set_info",
    "sfq_ctx_set_dedup", "sfq_get_dedup",
    "sfq_screen_check", "sfq_screen_parse", "sfq_fasta_sequences", "sfq_screen_set_create", "sfq_screen_set_add", "sfq_screen_set_clear",
    "sfq_screen_set_destroy", "sfq_screen_set_info", "sfq_screen_records", "sfq_ctx_set_screen", "sfq_get_screen",
    "sfq_demux_check", "sfq_demux_parse", "sfq_demux_sheet", "sfq_demux_records", "sfq_ctx_set_demux", "sfq_get_demux",
    "sfq_bgzf_bound", "sfq_bgzf_eof", "sfq_bgzf_deflate", "sfq_ctx_set_bgzf", "sfq_get_bgzf",
]


class Params(C.Structure):
    _fields_ = [("level", C.c_int32), ("block_reads", C.c_uint32), ("gen_bits", C.c_int32), ("models", C.c_uint32),
                ("kernel", C.c_uint32), ("version", C.c_uint32), ("prior_step", C.c_uint32), ("tables", C.c_uint32),
                ("chain_reads", C.c_uint32), ("lds_rows", C.c_uint32)]


class BlockInfo(C.Structure):
    _fields_ = [("first_record", C.c_uint64), ("n_records", C.c_uint32), ("llen", C.c_uint32),
                ("solid", C.c_uint8), ("two_id", C.c_uint8), ("n_byte", C.c_uint8), ("gen_bits", C.c_uint8),
                ("extra_hi", C.c_uint32), ("first_hdr_len", C.c_uint32), ("first_hdr_off", C.c_uint64),
                ("size", C.c_uint64 * NSTREAMS), ("status", C.c_uint32), ("hdr_bytes", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_blocks", C.c_uint32), ("abi_version", C.c_uint32),
                ("stream_bytes", C.c_uint64 * NSTREAMS), ("stream_offset", C.c_uint64 * NSTREAMS),
                ("total_bytes", C.c_uint64), ("first_hdr_bytes", C.c_uint64), ("n_chains", C.c_uint32), ("reserved", C.c_uint32),
                ("kernel_ms", C.c_double * 8), ("coder_ms", C.c_double * 4)]


class Segment(C.Structure):
    _fields_ = [("streams", C.c_void_p * NSTREAMS), ("stream_bytes", C.c_uint64 * NSTREAMS),
                ("blocks", C.POINTER(BlockInfo)), ("n_blocks", C.c_uint32), ("reserved", C.c_uint32),
                ("first_hdrs", C.c_void_p), ("first_hdr_bytes", C.c_uint64), ("qlt_prior", C.c_void_p), ("qlt_prior_bytes", C.c_uint64),
                ("chain_index", C.c_void_p), ("chain_index_bytes", C.c_uint64), ("rec_prior", C.c_void_p), ("rec_prior_bytes", C.c_uint64),
                ("raw_bytes", C.c_uint64)]


STATS_CYCLES = 512


class TextStats(C.Structure):
    """sfq_text_stats: the statistics of a FASTQ text (stats.hip).  Compares by value."""
    _fields_ = [("n_records", C.c_uint64), ("hdr_bytes", C.c_uint64), ("seq_bytes", C.c_uint64), ("plus_bytes", C.c_uint64),
                ("qlt_bytes", C.c_uint64), ("seq_len_min", C.c_uint32), ("seq_len_max", C.c_uint32),
                ("seq_hist", C.c_uint64 * 256), ("qlt_hist", C.c_uint64 * 256),
                ("cyc_n", C.c_uint64 * (STATS_CYCLES + 1)), ("cyc_qsum", C.c_uint64 * (STATS_CYCLES + 1))]

    def __eq__(self, other):
        return isinstance(other, TextStats) and bytes(self) == bytes(other)

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    def copy(self):
        t = TextStats()
        C.memmove(C.byref(t), C.byref(self), C.sizeof(TextStats))
        return t


class MateReport(C.Structure):
    """sfq_mate_report: what the name pass found (pair.hip k_pair_names)."""
    _fields_ = [("n_pairs", C.c_uint64), ("n_mismatch", C.c_uint64), ("first_mismatch", C.c_uint64),
                ("first_off_a", C.c_uint64), ("first_off_b", C.c_uint64)]


class Select(C.Structure):
    """sfq_select: the rule of a selection (sel.hip).  Select() is the rule that keeps every record: every term off."""
    _fields_ = [("first_record", C.c_uint64), ("n_records", C.c_uint64), ("min_len", C.c_uint32), ("max_len", C.c_uint32),
                ("max_n", C.c_uint32), ("min_mean_q_x100", C.c_uint32), ("qual_base", C.c_uint32), ("motif_len", C.c_uint32),
                ("motif", C.c_uint8 * 32), ("motif_rc", C.c_uint32), ("invert", C.c_uint32), ("pairs", C.c_uint32), ("sample", C.c_uint32),
                ("sample_seed", C.c_uint64), ("index_base", C.c_uint64)]

    def __init__(self, first_record=0, n_records=None, min_len=0, max_len=0xFFFFFFFF, max_n=0xFFFFFFFF, min_mean_q_x100=0, qual_base=33,
                 motif=b"", motif_rc=False, invert=False, pairs=0, sample=0, sample_seed=0, index_base=0, motif_len=None):
        super().__init__()
        self.first_record, self.n_records = first_record, SELECT_TO_END if n_records is None else n_records
        self.min_len, self.max_len, self.max_n = min_len, max_len, max_n
        self.min_mean_q_x100, self.qual_base = min_mean_q_x100, qual_base
        self.motif_len = len(motif) if motif_len is None else motif_len
        for i, b in enumerate(bytes(motif)[:32]):
            self.motif[i] = b
        self.motif_rc, self.invert, self.pairs = int(motif_rc), int(invert), pairs
        self.sample, self.sample_seed, self.index_base = sample, sample_seed, index_base


class SelectReport(C.Structure):
    """sfq_select_report: what a selection found."""
    _fields_ = [("n_in_range", C.c_uint64), ("n_kept", C.c_uint64), ("text_bytes", C.c_uint64), ("kept_bytes", C.c_uint64),
                ("n_fail", C.c_uint64 * 4)]


def select_check(sel) -> int:
    """sfq_select_check (no GPU): 0, or E_ARG for a rule the library refuses."""
    return int(lib().sfq_select_check(C.byref(sel)))


def select_parse(spec: str):
    """sfq_select_parse (no GPU): (Select, either) of the CLI's -k SPEC; ValueError with the library's words where it refuses."""
    sel, either, err = Select(), C.c_int(), C.create_string_buffer(256)
    if lib().sfq_select_parse(spec.encode(), C.byref(sel), C.byref(either), err, 256):
        raise ValueError(err.value.decode("latin1"))
    return sel, bool(either.value)


class Dedup(C.Structure):
    """sfq_dedup: the rule of a dedup (dd.hip).  Dedup() judges every record of the text by itself, without the context's set."""
    _fields_ = [("first_record", C.c_uint64), ("n_records", C.c_uint64), ("pairs", C.c_uint32), ("use_set", C.c_uint32)]

    def __init__(self, first_record=0, n_records=None, pairs=0, use_set=False):
        super().__init__()
        self.first_record, self.n_records = first_record, SELECT_TO_END if n_records is None else n_records
        self.pairs, self.use_set = int(pairs), int(use_set)


class DedupReport(C.Structure):
    """sfq_dedup_report: what a dedup found."""
    _fields_ = [("n_in_range", C.c_uint64), ("n_units", C.c_uint64), ("n_kept", C.c_uint64), ("n_dup_set", C.c_uint64),
                ("n_dup_call", C.c_uint64), ("text_bytes", C.c_uint64), ("kept_bytes", C.c_uint64), ("set_keys", C.c_uint64),
                ("set_key_bytes", C.c_uint64)]


def dedup_check(rule) -> int:
    """sfq_dedup_check (no GPU): 0, or E_ARG for a rule the library refuses."""
    return int(lib().sfq_dedup_check(C.byref(rule)))


class Screen(C.Structure):
    """sfq_screen: the rule of a screen (scr.hip).  Screen() drops every record of the text that shares one k-mer with the context's set."""
    _fields_ = [("first_record", C.c_uint64), ("n_records", C.c_uint64), ("pairs", C.c_uint32), ("min_hits", C.c_uint32),
                ("min_pct", C.c_uint32), ("keep_matched", C.c_uint32)]

    def __init__(self, first_record=0, n_records=None, pairs=0, min_hits=1, min_pct=0, keep_matched=False):
        super().__init__()
        self.first_record, self.n_records = first_record, SELECT_TO_END if n_records is None else n_records
        self.pairs, self.min_hits, self.min_pct, self.keep_matched = int(pairs), int(min_hits), int(min_pct), int(keep_matched)


class ScreenReport(C.Structure):
    """sfq_screen_report: what a screen found."""
    _fields_ = [("n_in_range", C.c_uint64), ("n_units", C.c_uint64), ("n_kept", C.c_uint64), ("n_matched_records", C.c_uint64),
                ("n_windows", C.c_uint64), ("n_hits", C.c_uint64), ("text_bytes", C.c_uint64), ("kept_bytes", C.c_uint64),
                ("set_kmers", C.c_uint64)]


def screen_check(rule) -> int:
    """sfq_screen_check (no GPU): 0, or E_ARG for a rule the library refuses."""
    return int(lib().sfq_screen_check(C.byref(rule)))


def screen_parse(spec: str):
    """sfq_screen_parse (no GPU): (Screen, k) of the terms of the CLI's -G; a ValueError carries the library's message."""
    rule, k, err = Screen(), C.c_uint32(), C.create_string_buffer(256)
    if lib().sfq_screen_parse(spec.encode(), C.byref(rule), C.byref(k), err, len(err)):
        raise ValueError(err.value.decode())
    return rule, int(k.value)


DEMUX_HEADER, DEMUX_BASES, DEMUX_MAX_SAMPLES = 1, 2, 4096


class DemuxPart(C.Structure):
    """sfq_demux_part: where a barcode part's observed bytes come from.  len 0: the part is absent."""
    _fields_ = [("src", C.c_uint32), ("mate", C.c_uint32), ("sub", C.c_uint32), ("pos", C.c_uint32), ("len", C.c_uint32)]

    def __init__(self, src=0, mate=0, sub=0, pos=0, len=0):
        super().__init__(int(src), int(mate), int(sub), int(pos), int(len))


class Demux(C.Structure):
    """sfq_demux: the rule of a demultiplexing (dmx.hip).  parts: one or two DemuxPart."""
    _fields_ = [("first_record", C.c_uint64), ("n_records", C.c_uint64), ("pairs", C.c_uint32), ("split_mates", C.c_uint32),
                ("max_mm", C.c_uint32), ("clip", C.c_uint32), ("part", DemuxPart * 2), ("n_samples", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, parts=(), n_samples=0, max_mm=1, pairs=0, split_mates=0, clip=0, first_record=0, n_records=None):
        super().__init__()
        self.first_record, self.n_records = first_record, SELECT_TO_END if n_records is None else n_records
        self.pairs, self.split_mates, self.max_mm, self.clip, self.n_samples = int(pairs), int(split_mates), int(max_mm), int(clip), int(n_samples)
        for i, p in enumerate(parts):
            self.part[i] = p

    @property
    def n_parts(self):
        """NP: the parts of the result."""
        return (2 if self.split_mates else 1) * (self.n_samples + 1)


class DemuxReport(C.Structure):
    """sfq_demux_report: what a demultiplexing found."""
    _fields_ = [("n_in_range", C.c_uint64), ("n_units", C.c_uint64), ("n_assigned", C.c_uint64), ("n_perfect", C.c_uint64),
                ("n_short", C.c_uint64), ("n_far", C.c_uint64), ("n_ambiguous", C.c_uint64), ("text_bytes", C.c_uint64),
                ("out_bytes", C.c_uint64), ("bases_clipped", C.c_uint64)]


BGZF_PIECE = 65280


class BgzfReport(C.Structure):
    """sfq_bgzf_report: what a BGZF pass wrote."""
    _fields_ = [("text_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("members", C.c_uint64), ("stored_members", C.c_uint64)]


def bgzf_bound(n, n_parts=1) -> int:
    """sfq_bgzf_bound (no GPU): what the members of n bytes of text in n_parts parts hold at most."""
    return int(lib().sfq_bgzf_bound(int(n), int(n_parts)))


def bgzf_eof() -> bytes:
    """sfq_bgzf_eof (no GPU): the 28 bytes that end a BGZF file."""
    buf = C.create_string_buffer(28)
    if lib().sfq_bgzf_eof(buf) != 28:
        raise SfqError(E_ARG, "sfq_bgzf_eof")
    return buf.raw


def _barcode_rows(barcodes, rule=None) -> bytes:
    """the rows as the library takes them; with a rule, a ValueError unless they are its n_samples rows of B bytes (the library reads that many)"""
    rows = bytes(barcodes) if isinstance(barcodes, (bytes, bytearray)) else b"".join(barcodes)
    if rule is not None:
        want = rule.n_samples * (rule.part[0].len + rule.part[1].len)
        if len(rows) != want:
            raise ValueError("barcodes: %d bytes, the rule's %d samples of %d bases are %d" % (len(rows), rule.n_samples, rule.part[0].len + rule.part[1].len, want))
    return rows


def demux_check(rule, barcodes) -> int:
    """sfq_demux_check (no GPU): 0, or E_ARG for a rule or barcodes the library refuses.  barcodes: the rows, a list of bytes or
    one bytes object of n_samples * B bytes; None: a null pointer."""
    try:
        rows = None if barcodes is None else _barcode_rows(barcodes, rule)
    except ValueError:
        return -1                                                       # rows that are not the rule's: E_ARG, and the library is not shown them
    return int(lib().sfq_demux_check(None if rule is None else C.byref(rule), rows))


def demux_parse(spec: str):
    """sfq_demux_parse (no GPU): the Demux of the terms of the CLI's -X (lengths and samples are the sheet's); a ValueError
    carries the library's message."""
    rule, err = Demux(), C.create_string_buffer(256)
    if lib().sfq_demux_parse(spec.encode(), C.byref(rule), err, len(err)):
        raise ValueError(err.value.decode())
    return rule


def demux_sheet(text: bytes, max_samples=DEMUX_MAX_SAMPLES):
    """sfq_demux_sheet (no GPU): (names, barcodes, len0, len1) of a sample sheet's bytes, barcodes a list of bytes rows (part 0's
    bases, then part 1's); a ValueError carries the library's message, which names the line."""
    names, codes = C.create_string_buffer(65 * max_samples), C.create_string_buffer(32 * max_samples)
    n, l0, l1, err = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.create_string_buffer(256)
    if lib().sfq_demux_sheet(text, len(text), int(max_samples), names, codes, C.byref(n), C.byref(l0), C.byref(l1), err, len(err)):
        raise ValueError(err.value.decode())
    B = l0.value + l1.value
    return ([names.raw[65 * s:65 * s + 65].split(b"\0", 1)[0].decode() for s in range(n.value)],
            [codes.raw[B * s:B * s + B] for s in range(n.value)], int(l0.value), int(l1.value))


def fasta_sequences(fasta: bytes, cap=None, size_only=False):
    """sfq_fasta_sequences (no GPU): a FASTA file's bytes as a sequence text; cap: the room given (default: what it needs);
    size_only: the result's size alone, an int.  An SfqError of code E_OVERFLOW where cap is too small."""
    n = int(lib().sfq_fasta_sequences(fasta, len(fasta), None, 0))
    if n < 0:
        raise SfqError(n, "sfq_fasta_sequences")
    if size_only:
        return n
    room = n if cap is None else int(cap)
    out = C.create_string_buffer(room + 1)
    m = int(lib().sfq_fasta_sequences(fasta, len(fasta), C.cast(out, C.c_void_p), room))
    if m < 0:
        raise SfqError(m, "sfq_fasta_sequences: the result needs %d bytes" % n)
    return out.raw[:m]


class Trim(C.Structure):
    """sfq_trim: the rule of a trim (trim.hip).  Trim() is the rule that changes nothing: every term off."""
    _fields_ = [("head", C.c_uint32), ("tail", C.c_uint32), ("max_len", C.c_uint32), ("lead_q", C.c_uint32), ("trail_q", C.c_uint32),
                ("win_len", C.c_uint32), ("win_q_x100", C.c_uint32), ("qual_base", C.c_uint32), ("adapter_len", C.c_uint32),
                ("adapter", C.c_uint8 * 32), ("adapter_mm", C.c_uint32), ("adapter_min", C.c_uint32)]

    def __init__(self, head=0, tail=0, max_len=0xFFFFFFFF, lead_q=0, trail_q=0, win_len=0, win_q_x100=0, qual_base=33, adapter=b"",
                 adapter_mm=0, adapter_min=None, adapter_len=None):
        super().__init__()
        self.head, self.tail, self.max_len, self.lead_q, self.trail_q = head, tail, max_len, lead_q, trail_q
        self.win_len, self.win_q_x100, self.qual_base = win_len, win_q_x100, qual_base
        self.adapter_len = len(adapter) if adapter_len is None else adapter_len
        for i, b in enumerate(bytes(adapter)[:32]):
            self.adapter[i] = b
        self.adapter_mm = adapter_mm
        self.adapter_min = min(3, len(adapter)) if adapter_min is None else adapter_min


class TrimReport(C.Structure):
    """sfq_trim_report: what a trim found."""
    _fields_ = [("n_records", C.c_uint64), ("n_changed", C.c_uint64), ("n_emptied", C.c_uint64), ("text_bytes", C.c_uint64),
                ("out_bytes", C.c_uint64), ("bases_in", C.c_uint64), ("bases_out", C.c_uint64), ("n_cut", C.c_uint64 * 4)]


def trim_check(trim) -> int:
    """sfq_trim_check (no GPU): 0, or E_ARG for a rule the library refuses."""
    return int(lib().sfq_trim_check(C.byref(trim)))


def trim_parse(spec: str):
    """sfq_trim_parse (no GPU): the Trim of the CLI's -c SPEC; ValueError with the library's words where it refuses."""
    trim, err = Trim(), C.create_string_buffer(256)
    if lib().sfq_trim_parse(spec.encode(), C.byref(trim), err, 256):
        raise ValueError(err.value.decode("latin1"))
    return trim


OVERLAP_MAX_LEN = 512


class Overlap(C.Structure):
    """sfq_overlap: the rule of the mates' overlap search (ovl.hip).  Overlap() is the CLI's `default`: 30 bases, 5 mismatches, 20 %, cut."""
    _fields_ = [("first_record", C.c_uint64), ("n_records", C.c_uint64), ("min_overlap", C.c_uint32), ("max_mm", C.c_uint32),
                ("max_mm_pct", C.c_uint32), ("cut", C.c_uint32)]

    def __init__(self, first_record=0, n_records=None, min_overlap=30, max_mm=5, max_mm_pct=20, cut=1):
        super().__init__()
        self.first_record, self.n_records = first_record, SELECT_TO_END if n_records is None else n_records
        self.min_overlap, self.max_mm, self.max_mm_pct, self.cut = min_overlap, max_mm, max_mm_pct, int(cut)


class OverlapReport(C.Structure):
    """sfq_overlap_report: what the overlap search found."""
    _fields_ = [("n_pairs", C.c_uint64), ("n_skipped", C.c_uint64), ("n_overlap", C.c_uint64), ("n_cut", C.c_uint64),
                ("text_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("bases_in", C.c_uint64), ("bases_out", C.c_uint64),
                ("mismatches", C.c_uint64), ("insert_hist", C.c_uint64 * (2 * OVERLAP_MAX_LEN + 1))]


def overlap_check(rule) -> int:
    """sfq_overlap_check (no GPU): 0, or E_ARG for a rule the library refuses."""
    return int(lib().sfq_overlap_check(C.byref(rule)))


def overlap_parse(spec: str):
    """sfq_overlap_parse (no GPU): the Overlap of the CLI's -o SPEC; ValueError with the library's words where it refuses."""
    rule, err = Overlap(), C.create_string_buffer(256)
    if lib().sfq_overlap_parse(spec.encode(), C.byref(rule), err, 256):
        raise ValueError(err.value.decode("latin1"))
    return rule


class Merge(C.Structure):
    """sfq_merge: the rule of the mates' merge (mrg.hip).  Merge() is the CLI's `default,merge=PATH`: Overlap()'s search, qualities from 33."""
    _fields_ = [("first_record", C.c_uint64), ("n_records", C.c_uint64), ("min_overlap", C.c_uint32), ("max_mm", C.c_uint32),
                ("max_mm_pct", C.c_uint32), ("qual_base", C.c_uint32)]

    def __init__(self, first_record=0, n_records=None, min_overlap=30, max_mm=5, max_mm_pct=20, qual_base=33):
        super().__init__()
        self.first_record, self.n_records = first_record, SELECT_TO_END if n_records is None else n_records
        self.min_overlap, self.max_mm, self.max_mm_pct, self.qual_base = min_overlap, max_mm, max_mm_pct, qual_base


class MergeReport(C.Structure):
    """sfq_merge_report: what the merge found."""
    _fields_ = [("n_pairs", C.c_uint64), ("n_skipped", C.c_uint64), ("n_merged", C.c_uint64),
                ("text_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("merged_bytes", C.c_uint64),
                ("bases_in", C.c_uint64), ("bases_merged", C.c_uint64), ("mismatches", C.c_uint64),
                ("n_x_wins", C.c_uint64), ("n_y_wins", C.c_uint64), ("insert_hist", C.c_uint64 * (2 * OVERLAP_MAX_LEN + 1))]


def merge_check(rule) -> int:
    """sfq_merge_check (no GPU): 0, or E_ARG for a rule the library refuses."""
    return int(lib().sfq_merge_check(C.byref(rule)))


class SfqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("slimfastq_amd error %d: %s" % (code, msg))
        self.code = code


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process: PyTorch wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7).  If this library pulled in /opt/rocm's copy first, a later `import torch` would
    load a second runtime and see no GPU.  Pre-loading torch's copy makes the dynamic linker bind our
    DT_NEEDED libamdhip64.so.7 to it.  Set SFQ_HIP_RUNTIME=system to skip (e.g. torch-free processes
    that must use /opt/rocm)."""
    if os.environ.get("SFQ_HIP_RUNTIME") == "system":
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except Exception:
        spec = None
    if spec and spec.origin:
        p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: run `python -m slimfastq_amd.build` (there is no CPU fallback)" % LIB_PATH)
        _share_hip_runtime_with_torch()
        L = C.CDLL(LIB_PATH)
        vp, u64, u8p = C.c_void_p, C.c_uint64, C.c_void_p
        L.sfq_stream_name.restype = C.c_char_p
        L.sfq_ctx_create.argtypes = [C.POINTER(vp), C.c_int]
        L.sfq_ctx_destroy.argtypes = [vp]
        L.sfq_ctx_destroy.restype = None
        L.sfq_last_error.argtypes = [vp]
        L.sfq_last_error.restype = C.c_char_p
        L.sfq_ctx_set_table_budget.argtypes = [vp, u64]
        L.sfq_ctx_device_memory.argtypes = [vp]
        L.sfq_ctx_device_memory.restype = u64
        L.sfq_ctx_stream.argtypes = [vp]
        L.sfq_ctx_stream.restype = vp
        L.sfq_ctx_synchronize.argtypes = [vp]
        L.sfq_host_alloc.argtypes = [vp, C.c_uint64]; L.sfq_host_alloc.restype = C.c_void_p
        L.sfq_host_free.argtypes = [vp, C.c_void_p]; L.sfq_host_free.restype = None
        L.sfq_encode_bound.argtypes = [u64]
        L.sfq_encode_bound.restype = u64
        for f in (L.sfq_encode_blocks, L.sfq_encode_qlt_blocks, L.sfq_encode_blocks_host):
            f.argtypes = [vp, u8p, u64, C.POINTER(Params), u8p, u64, C.POINTER(Result)]
        L.sfq_get_block_index.argtypes = [vp, C.POINTER(BlockInfo), C.c_uint32]
        L.sfq_get_first_headers.argtypes = [vp, u8p, u64]
        L.sfq_decode_blocks.argtypes = [vp, C.POINTER(Params), C.POINTER(BlockInfo), C.c_uint32, u8p, u64, u8p,
                                        C.POINTER(u64), u8p, u64, C.POINTER(u64), C.POINTER(Result)]
        L.sfq_decode_blocks_host.argtypes = [vp, C.POINTER(Params), C.POINTER(BlockInfo), C.c_uint32, u8p, u64, u8p, u64,
                                             C.POINTER(u64), u8p, u64, C.POINTER(u64), C.POINTER(Result)]
        L.sfq_decode_block_range.argtypes = [vp, C.POINTER(Params), C.POINTER(BlockInfo), C.c_uint32, u8p, u64, u8p,
                                             C.POINTER(u64), C.c_uint32, C.c_uint32, u8p, u64, C.POINTER(u64), C.POINTER(Result)]
        L.sfq_decode_block_range_host.argtypes = [vp, C.POINTER(Params), C.POINTER(BlockInfo), C.c_uint32, u8p, u64, u8p, u64,
                                                  C.POINTER(u64), C.c_uint32, C.c_uint32, u8p, u64, C.POINTER(u64), C.POINTER(Result)]
        L.sfq_get_qlt_prior.argtypes = [vp, u8p, u64]
        L.sfq_get_qlt_prior.restype = C.c_int64
        L.sfq_set_qlt_prior.argtypes = [vp, u8p, u64]
        L.sfq_build_priors.argtypes = [vp, u8p, u64, C.POINTER(Params)]
        L.sfq_count_priors.argtypes = [vp, u8p, u64, C.POINTER(Params), C.c_uint32]
        L.sfq_prior_counts_words.argtypes = [C.c_int, C.POINTER(u64), C.POINTER(u64)]
        L.sfq_prior_counts_words.restype = None
        L.sfq_get_prior_counts.argtypes = [vp, C.c_int, u8p, u8p]
        L.sfq_set_prior_counts.argtypes = [vp, C.c_int, u8p, u8p]
        L.sfq_get_rec_prior.argtypes = [vp, u8p, u64]
        L.sfq_get_rec_prior.restype = C.c_int64
        L.sfq_set_rec_prior.argtypes = [vp, u8p, u64]
        L.sfq_get_chain_index.argtypes = [vp, u8p, u64]
        L.sfq_get_chain_index.restype = C.c_int64
        L.sfq_set_chain_index.argtypes = [vp, u8p, u64]
        L.sfq_synth_fastq.argtypes = [u64, u64, C.c_uint32, u64, C.c_int, u8p, u64]
        L.sfq_synth_fastq.restype = C.c_int64
        L.sfq_archive_write.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(u64)]
        L.sfq_pack_block_index.argtypes = [C.POINTER(BlockInfo), C.c_uint32, u8p, u64]
        L.sfq_pack_block_index.restype = C.c_int64
        L.sfq_archive_write_segments.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(Segment)]
        u32p = C.POINTER(C.c_uint32)
        L.sfq_crc32.argtypes = [vp, u8p, C.POINTER(u64), C.c_uint32, u32p]
        L.sfq_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, u64]
        L.sfq_crc32_combine.restype = C.c_uint32
        L.sfq_ctx_set_checksums.argtypes = [vp, C.c_int]
        L.sfq_get_checksums.argtypes = [vp, u32p, C.c_uint32, u32p]
        L.sfq_set_block_checksums.argtypes = [vp, u32p, C.c_uint32]
        tsp = C.POINTER(TextStats)
        L.sfq_ctx_set_stats.argtypes = [vp, C.c_int]
        L.sfq_get_text_stats.argtypes = [vp, tsp]
        L.sfq_text_stats_merge.argtypes = [tsp, tsp]
        L.sfq_text_stats_merge.restype = None
        L.sfq_pack_text_stats.argtypes = [tsp, u8p, u64]
        L.sfq_pack_text_stats.restype = C.c_int64
        L.sfq_unpack_text_stats.argtypes = [u8p, u64, tsp]
        L.sfq_quality_map_preset.argtypes = [C.c_int, C.c_char_p]
        L.sfq_quality_map_check.argtypes = [C.c_char_p]
        L.sfq_map_qualities.argtypes = [vp, u8p, u64, C.c_char_p, C.POINTER(u64)]
        L.sfq_ctx_set_quality_map.argtypes = [vp, C.c_char_p]
        L.sfq_get_quality_map_changed.argtypes = [vp]
        L.sfq_get_quality_map_changed.restype = u64
        u64p = C.POINTER(u64)
        L.sfq_interleave.argtypes = [vp, vp, u64, vp, u64, vp, u64, u64p, u64p]
        L.sfq_split_pairs.argtypes = [vp, vp, u64, vp, u64, u64p, u64p]
        L.sfq_encode_pairs_host.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, vp]
        L.sfq_ctx_set_pair_split.argtypes = [vp, C.c_int]
        L.sfq_get_pair_split.argtypes = [vp, u64p, u64p]
        L.sfq_split_pairs_range.argtypes = [vp, vp, u64, u64, u64, vp, u64, u64p, u64p]
        L.sfq_check_mates.argtypes = [vp, vp, u64, vp, u64, C.POINTER(MateReport)]
        L.sfq_ctx_set_mate_check.argtypes = [vp, C.c_int]
        L.sfq_get_mate_report.argtypes = [vp, C.POINTER(MateReport)]
        L.sfq_pair_window_blocks.argtypes = [C.POINTER(BlockInfo), C.c_uint32, u64, u64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.sfq_decode_pair_range_host.argtypes = [vp, C.POINTER(Params), C.POINTER(BlockInfo), C.c_uint32, u8p, u64, u8p, u64, C.POINTER(u64),
                                                 u64, u64, u8p, u64, u64p, u64p, C.POINTER(Result)]
        L.sfq_pick_lines.argtypes = [vp, vp, u64, C.c_int, u64, u64, vp, u64, u64p, u64p]
        L.sfq_ctx_set_pick.argtypes = [vp, C.c_int]
        L.sfq_get_pick.argtypes = [vp, C.POINTER(C.c_int), u64p, u64p]
        L.sfq_select_check.argtypes = [C.POINTER(Select)]
        L.sfq_select_parse.argtypes = [C.c_char_p, C.POINTER(Select), C.POINTER(C.c_int), C.c_char_p, u64]
        L.sfq_select_records.argtypes = [vp, vp, u64, C.POINTER(Select), vp, u64, u64p, C.POINTER(SelectReport)]
        L.sfq_ctx_set_select.argtypes = [vp, C.POINTER(Select)]
        L.sfq_get_select.argtypes = [vp, C.POINTER(SelectReport)]
        L.sfq_trim_check.argtypes = [C.POINTER(Trim)]
        L.sfq_trim_parse.argtypes = [C.c_char_p, C.POINTER(Trim), C.c_char_p, u64]
        L.sfq_trim_records.argtypes = [vp, vp, u64, C.POINTER(Trim), vp, u64, u64p, C.POINTER(TrimReport)]
        L.sfq_ctx_set_trim.argtypes = [vp, C.POINTER(Trim)]
        L.sfq_get_trim.argtypes = [vp, C.POINTER(TrimReport)]
        L.sfq_overlap_check.argtypes = [C.POINTER(Overlap)]
        L.sfq_overlap_parse.argtypes = [C.c_char_p, C.POINTER(Overlap), C.c_char_p, u64]
        L.sfq_overlap_pairs.argtypes = [vp, vp, u64, C.POINTER(Overlap), vp, u64, u64p, C.POINTER(OverlapReport)]
        L.sfq_ctx_set_overlap.argtypes = [vp, C.POINTER(Overlap)]
        L.sfq_get_overlap.argtypes = [vp, C.POINTER(OverlapReport)]
        L.sfq_merge_check.argtypes = [C.POINTER(Merge)]
        L.sfq_merge_pairs.argtypes = [vp, vp, u64, C.POINTER(Merge), vp, u64, u64p, u64p, C.POINTER(MergeReport)]
        L.sfq_ctx_set_merge.argtypes = [vp, C.POINTER(Merge)]
        L.sfq_get_merge.argtypes = [vp, C.POINTER(MergeReport), u64p]
        L.sfq_dedup_check.argtypes = [C.POINTER(Dedup)]
        L.sfq_dedup_records.argtypes = [vp, vp, u64, C.POINTER(Dedup), vp, u64, u64p, C.POINTER(DedupReport)]
        L.sfq_dedup_set_create.argtypes = [vp, u64, u64, C.c_uint32]
        L.sfq_dedup_set_clear.argtypes = [vp]
        L.sfq_dedup_set_destroy.argtypes = [vp]
        L.sfq_dedup_set_info.argtypes = [vp, u64p, u64p, u64p, u64p]
        L.sfq_ctx_set_dedup.argtypes = [vp, C.POINTER(Dedup)]
        L.sfq_get_dedup.argtypes = [vp, C.POINTER(DedupReport)]
        L.sfq_screen_check.argtypes = [C.POINTER(Screen)]
        L.sfq_screen_parse.argtypes = [C.c_char_p, C.POINTER(Screen), C.POINTER(C.c_uint32), C.c_char_p, u64]
        L.sfq_fasta_sequences.argtypes = [C.c_char_p, u64, vp, u64]
        L.sfq_fasta_sequences.restype = C.c_int64
        L.sfq_screen_set_create.argtypes = [vp, C.c_uint32, u64]
        L.sfq_screen_set_add.argtypes = [vp, C.c_char_p, u64]
        L.sfq_screen_set_clear.argtypes = [vp]
        L.sfq_screen_set_destroy.argtypes = [vp]
        L.sfq_screen_set_info.argtypes = [vp, C.POINTER(C.c_uint32), u64p, u64p]
        L.sfq_screen_records.argtypes = [vp, vp, u64, C.POINTER(Screen), vp, u64, u64p, C.POINTER(ScreenReport)]
        L.sfq_ctx_set_screen.argtypes = [vp, C.POINTER(Screen)]
        L.sfq_get_screen.argtypes = [vp, C.POINTER(ScreenReport)]
        L.sfq_demux_check.argtypes = [C.POINTER(Demux), C.c_char_p]
        L.sfq_demux_parse.argtypes = [C.c_char_p, C.POINTER(Demux), C.c_char_p, u64]
        L.sfq_demux_sheet.argtypes = [C.c_char_p, u64, C.c_uint32, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32), C.c_char_p, u64]
        L.sfq_demux_records.argtypes = [vp, vp, u64, C.POINTER(Demux), C.c_char_p, vp, u64, u64p, u64p, u64p, C.POINTER(DemuxReport)]
        L.sfq_ctx_set_demux.argtypes = [vp, C.POINTER(Demux), C.c_char_p]
        L.sfq_get_demux.argtypes = [vp, C.POINTER(DemuxReport), u64p, u64p, u64]
        L.sfq_bgzf_bound.restype = C.c_uint64
        L.sfq_bgzf_bound.argtypes = [u64, C.c_uint32]
        L.sfq_bgzf_eof.argtypes = [C.c_char_p]
        L.sfq_bgzf_deflate.argtypes = [vp, vp, u64p, C.c_uint32, vp, u64, u64p, C.POINTER(BgzfReport)]
        L.sfq_ctx_set_bgzf.argtypes = [vp, C.c_int]
        L.sfq_get_bgzf.argtypes = [vp, C.POINTER(BgzfReport), u64p, u64p, u64]
        _lib = L
    return _lib


def synth_fastq(n_reads, read_len=150, seed=1, kind=0, first_read=0) -> bytes:
    """Deterministic synthetic FASTQ (host-side generator inside the library)."""
    L = lib()
    need = L.sfq_synth_fastq(first_read, n_reads, read_len, seed, kind, None, 0)
    if need < 0:
        raise SfqError(need, "synth")
    buf = np.empty(need, np.uint8)
    got = L.sfq_synth_fastq(first_read, n_reads, read_len, seed, kind, buf.ctypes.data_as(C.c_void_p), need)
    if got != need:
        raise SfqError(got, "synth")
    return buf.tobytes()


def archive_write_segments(path: str, parts, level: int, orig_name: str, tables=TABLES_FROZEN, shared_prior=False):
    """One block-format archive, a segment per part, in order (sfq_archive_write_segments).  parts: dicts of one encode call's
    results: streams=[bytes] * NSTREAMS, blocks=[BlockInfo], first=bytes, prior=bytes, chains=bytes, rec_prior=bytes, raw=int."""
    keep = []

    def ptr(b):
        if not len(b):
            return None
        keep.append(np.frombuffer(b, np.uint8))                      # (no copy: the bytes stay where they are)
        return keep[-1].ctypes.data
    segs = (Segment * len(parts))()
    for g, p in zip(segs, parts):
        for s in range(NSTREAMS):
            g.streams[s] = ptr(p["streams"][s]); g.stream_bytes[s] = len(p["streams"][s])
        keep.append((BlockInfo * len(p["blocks"]))(*p["blocks"]))
        g.blocks = C.cast(keep[-1], C.POINTER(BlockInfo)); g.n_blocks = len(p["blocks"])
        g.first_hdrs = ptr(p["first"]); g.first_hdr_bytes = len(p["first"])
        g.qlt_prior = ptr(p["prior"]); g.qlt_prior_bytes = len(p["prior"])
        g.chain_index = ptr(p["chains"]); g.chain_index_bytes = len(p["chains"])
        g.rec_prior = ptr(p["rec_prior"]); g.rec_prior_bytes = len(p["rec_prior"])
        g.raw_bytes = p["raw"]
    rc = lib().sfq_archive_write_segments(path.encode(), orig_name.encode(), level, tables, int(shared_prior), len(parts), segs)
    if rc:
        raise SfqError(rc, "cannot write " + path)


def crc32_combine(crc_a, crc_b, len_b):
    """zlib's crc32_combine: the CRC-32 of A followed by B from crc(A), crc(B) and len(B) (host only)."""
    return int(lib().sfq_crc32_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, int(len_b)))


def quality_map_preset(name_or_id) -> bytes:
    """The 256-byte table of a quality binning preset ("illumina8" / "novaseq4", or QMAP_*); host only."""
    pid = QMAP_PRESETS.get(name_or_id, name_or_id) if isinstance(name_or_id, str) else int(name_or_id)
    buf = C.create_string_buffer(256)
    rc = lib().sfq_quality_map_preset(pid if isinstance(pid, int) else -1, buf)
    if rc:
        raise SfqError(rc, "no quality map preset %r" % (name_or_id,))
    return buf.raw


def quality_map_check(lut: bytes) -> int:
    """SFQ_OK (0) for a table a quality map may use, SFQ_E_ARG (-1) otherwise; host only."""
    if len(lut) != 256:
        return -1
    return int(lib().sfq_quality_map_check(bytes(lut)))


def _lut_arg(lut):
    lut = bytes(lut)
    if len(lut) != 256:
        raise SfqError(-1, "a quality map is a table of 256 bytes")
    return lut


def stats_merge(into: TextStats, add: TextStats) -> TextStats:
    """The statistics of two texts into those of both, in place (sfq_text_stats_merge); returns into."""
    lib().sfq_text_stats_merge(C.byref(into), C.byref(add))
    return into


def pack_text_stats(stats: TextStats) -> bytes:
    """The "txt.stat" stream of these statistics."""
    L = lib()
    n = L.sfq_pack_text_stats(C.byref(stats), None, 0)
    if n < 0:
        raise SfqError(n, "sfq_pack_text_stats")
    buf = C.create_string_buffer(max(n, 1))
    got = L.sfq_pack_text_stats(C.byref(stats), buf, n)
    if got != n:
        raise SfqError(got, "sfq_pack_text_stats")
    return buf.raw[:n]


def unpack_text_stats(blob: bytes) -> TextStats:
    """"txt.stat" -> TextStats; SfqError (code -6) where the stream is damaged."""
    t = TextStats()
    rc = lib().sfq_unpack_text_stats(blob if len(blob) else None, len(blob), C.byref(t))
    if rc:
        raise SfqError(rc, "damaged txt.stat")
    return t


class Encoded:
    """Host copy of one sfq_encode_blocks result.  crcs / text_crc: the CRC-32 of every block's text and of the whole text,
    where the context had checksums on (else None); stats: the text's statistics (TextStats), where it had them on (else None)."""

    def __init__(self, res, blocks, first_hdrs, data, prior=b"", chains=b"", rec_prior=b"", crcs=None, text_crc=None, stats=None):
        self.res, self.blocks, self.first_hdrs, self.data, self.prior, self.chains = res, blocks, first_hdrs, data, prior, chains
        self.rec_prior = rec_prior
        self.crcs, self.text_crc = crcs, text_crc
        self.stats = stats

    def clone(self):
        """A deep copy (the tests damage copies)."""
        blocks = (BlockInfo * len(self.blocks))()
        C.memmove(blocks, self.blocks, C.sizeof(blocks))
        res = Result()
        C.memmove(C.byref(res), C.byref(self.res), C.sizeof(Result))
        data = self.data.copy() if isinstance(self.data, np.ndarray) else bytes(self.data)
        return Encoded(res, blocks, bytes(self.first_hdrs), data, bytes(self.prior), bytes(self.chains), bytes(self.rec_prior),
                       None if self.crcs is None else list(self.crcs), self.text_crc, None if self.stats is None else self.stats.copy())

    def stream(self, s, block=None) -> bytes:
        """Bytes of stream s (an id or a name): the whole concatenation, or one block's part."""
        if isinstance(s, str):
            s = STREAM_NAMES.index(s)
        off = self.res.stream_offset[s]
        if block is None:
            return bytes(self.data[off:off + self.res.stream_bytes[s]])
        for b in range(block):
            off += self.blocks[b].size[s]
        return bytes(self.data[off:off + self.blocks[block].size[s]])

    @property
    def payload_bytes(self):
        return int(self.res.total_bytes)

    @property
    def archive_bytes(self):
        """Everything a decoder needs: streams + first headers + quality prior + ~the block index."""
        return int(self.res.total_bytes) + len(self.first_hdrs) + len(self.prior) + len(self.chains) + len(self.rec_prior) + 14 * len(self.blocks)


class Context:
    def __init__(self, device=0, table_budget=None):
        self._h = C.c_void_p()
        rc = lib().sfq_ctx_create(C.byref(self._h), device)
        if rc != 0:
            raise SfqError(rc, "sfq_ctx_create failed (a HIP device is required; there is no CPU path)")
        if table_budget:
            lib().sfq_ctx_set_table_budget(self._h, int(table_budget))

    def close(self):
        if self._h:
            lib().sfq_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise SfqError(rc, lib().sfq_last_error(self._h).decode("latin1"))

    @property
    def handle(self):
        return self._h

    def set_checksums(self, on=True):
        """Checksums on: every call computes the CRC-32 of each block's text and of the whole text (checksums())."""
        self._check(lib().sfq_ctx_set_checksums(self._h, 1 if on else 0))

    def checksums(self):
        """(per-block CRCs, CRC of the whole text) of the last call; ([], 0) where it computed none."""
        L = lib()
        text = C.c_uint32()
        n = L.sfq_get_checksums(self._h, None, 0, C.byref(text))
        if n < 0:
            self._check(n)
        buf = (C.c_uint32 * max(n, 1))()
        L.sfq_get_checksums(self._h, buf, n, None)
        return list(buf)[:n], text.value

    def set_stats(self, on=True):
        """Text statistics on: every encode call counts them of its text on the GPU (text_stats())."""
        self._check(lib().sfq_ctx_set_stats(self._h, 1 if on else 0))

    def text_stats(self):
        """The last encode call's TextStats; None where it computed none."""
        t = TextStats()
        rc = lib().sfq_get_text_stats(self._h, C.byref(t))
        if rc < 0:
            self._check(rc)
        return t if rc == 1 else None

    def map_qualities(self, d_ptr, nbytes, lut) -> int:
        """Every quality byte of the FASTQ text in the device buffer at d_ptr through the 256-byte table, in place; returns the
        number of bytes whose value changed."""
        changed = C.c_uint64()
        self._check(lib().sfq_map_qualities(self._h, C.c_void_p(d_ptr), int(nbytes), _lut_arg(lut), C.byref(changed)))
        return int(changed.value)

    def set_quality_map(self, lut):
        """A 256-byte table: encode_host maps the qualities of its text through it before it codes them (LOSSY).  None: off."""
        self._check(lib().sfq_ctx_set_quality_map(self._h, None if lut is None else _lut_arg(lut)))

    def quality_map_changed(self) -> int:
        """Bytes changed by the last encode call's quality map (0 where none ran)."""
        return int(lib().sfq_get_quality_map_changed(self._h))

    def interleave(self, d_a, na, d_b, nb, d_out, out_cap):
        """The FASTQ texts in the device buffers at d_a and d_b record by record into the one at d_out (A0 B0 A1 B1 ...); returns
        (bytes written, pairs).  An SfqError of code E_OVERFLOW carries the size needed as .needed."""
        n, pairs = C.c_uint64(), C.c_uint64()
        rc = lib().sfq_interleave(self._h, C.c_void_p(d_a), int(na), C.c_void_p(d_b), int(nb), C.c_void_p(d_out), int(out_cap),
                                  C.byref(n), C.byref(pairs))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return int(n.value), int(pairs.value)

    def split_pairs(self, d_text, nbytes, d_out, out_cap):
        """The interleaved FASTQ text in the device buffer at d_text into the one at d_out: its even records, then its odd ones;
        returns (where the odd ones begin, pairs)."""
        split, pairs = C.c_uint64(), C.c_uint64()
        self._check(lib().sfq_split_pairs(self._h, C.c_void_p(d_text), int(nbytes), C.c_void_p(d_out), int(out_cap),
                                          C.byref(split), C.byref(pairs)))
        return int(split.value), int(pairs.value)

    def split_pairs_range(self, d_text, nbytes, first_record, n_records, d_out, out_cap):
        """Records [first_record, first_record + n_records) of the FASTQ text in the device buffer at d_text into the one at d_out:
        the window's even records, then its odd ones (sfq_split_pairs_range); returns (where the odd ones begin, bytes written).  An
        SfqError of code E_OVERFLOW carries the size needed as .needed."""
        split, n = C.c_uint64(), C.c_uint64()
        rc = lib().sfq_split_pairs_range(self._h, C.c_void_p(d_text), int(nbytes), int(first_record), int(n_records),
                                         C.c_void_p(d_out), int(out_cap), C.byref(split), C.byref(n))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return int(split.value), int(n.value)

    def check_mates(self, d_a, na, d_b=None, nb=0) -> MateReport:
        """The names of record i of the device text at d_a against those of record i of the one at d_b; d_b None: d_a is an interleaved
        text, record 2k against record 2k + 1 (sfq_check_mates).  Mismatches are reported, not raised."""
        r = MateReport()
        self._check(lib().sfq_check_mates(self._h, C.c_void_p(d_a), int(na), C.c_void_p(d_b) if d_b is not None else None, int(nb), C.byref(r)))
        return r

    def set_mate_check(self, on=True):
        """On: encode_pairs_host compares the mates' names before it codes and raises an SfqError of code E_FORMAT where a pair differs."""
        self._check(lib().sfq_ctx_set_mate_check(self._h, 1 if on else 0))

    def mate_report(self):
        """What the last encode_pairs_host's name check found (a MateReport); None where it did not run."""
        r = MateReport()
        rc = lib().sfq_get_mate_report(self._h, C.byref(r))
        if rc < 0:
            self._check(rc)
        return r if rc == 1 else None

    def set_pair_split(self, on=True):
        """On: decode_host returns the first mates followed by the second mates (pair_split() says where) instead of the
        interleaved text."""
        self._check(lib().sfq_ctx_set_pair_split(self._h, 1 if on else 0))

    def pair_split(self):
        """(where the second mates begin, pairs) of the last decode call; None where it did not split its text."""
        first, pairs = C.c_uint64(), C.c_uint64()
        rc = lib().sfq_get_pair_split(self._h, C.byref(first), C.byref(pairs))
        if rc < 0:
            self._check(rc)
        return (int(first.value), int(pairs.value)) if rc == 1 else None

    def pick_lines(self, d_text, nbytes, what, d_out, out_cap, first_record=0, n_records=None):
        """Of records [first_record, first_record + n_records) (None: to the last) of the FASTQ text in the device buffer at d_text
        the lines `what` selects (PICK_*), one behind the other into the one at d_out (sfq_pick_lines); returns (bytes written,
        records picked).  An SfqError of code E_OVERFLOW carries the size needed as .needed."""
        n, recs = C.c_uint64(), C.c_uint64()
        rc = lib().sfq_pick_lines(self._h, C.c_void_p(d_text), int(nbytes), int(what), int(first_record),
                                  PICK_TO_END if n_records is None else int(n_records), C.c_void_p(d_out), int(out_cap), C.byref(n), C.byref(recs))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return int(n.value), int(recs.value)

    def set_pick(self, what=0):
        """PICK_*: decode_host, decode_range_host and decode_pair_range_host return the picked lines of the text they decoded instead
        of the text (get_pick() says of what); 0: off."""
        self._check(lib().sfq_ctx_set_pick(self._h, int(what)))

    def get_pick(self):
        """(selection, the decoded text's bytes, records) of the last decode call; None where it did not pick."""
        what, n, recs = C.c_int(), C.c_uint64(), C.c_uint64()
        rc = lib().sfq_get_pick(self._h, C.byref(what), C.byref(n), C.byref(recs))
        if rc < 0:
            self._check(rc)
        return (int(what.value), int(n.value), int(recs.value)) if rc == 1 else None

    def select_records(self, d_text, nbytes, sel, d_out, out_cap):
        """The records of the FASTQ text in the device buffer at d_text that the Select keeps, whole and in order, into the one at
        d_out (sfq_select_records); returns (bytes written, SelectReport).  An SfqError of code E_OVERFLOW carries the size needed
        as .needed."""
        n, rep = C.c_uint64(), SelectReport()
        rc = lib().sfq_select_records(self._h, C.c_void_p(d_text), int(nbytes), C.byref(sel), C.c_void_p(d_out), int(out_cap),
                                      C.byref(n), C.byref(rep))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return int(n.value), rep

    def set_select(self, sel=None):
        """A Select: decode_host, decode_range_host and decode_pair_range_host return the selection of the text they decoded instead
        of the text (get_select() says what it kept); None: off."""
        self._check(lib().sfq_ctx_set_select(self._h, None if sel is None else C.byref(sel)))

    def get_select(self):
        """The SelectReport of the last decode call; None where it did not select."""
        rep = SelectReport()
        rc = lib().sfq_get_select(self._h, C.byref(rep))
        if rc < 0:
            self._check(rc)
        return rep if rc == 1 else None

    def trim_records(self, d_text, nbytes, trim, d_out, out_cap):
        """The records of the FASTQ text in the device buffer at d_text, trimmed by the Trim, into the one at d_out
        (sfq_trim_records); returns (bytes written, TrimReport).  An SfqError of code E_OVERFLOW carries the size needed as .needed."""
        n, rep = C.c_uint64(), TrimReport()
        rc = lib().sfq_trim_records(self._h, C.c_void_p(d_text), int(nbytes), C.byref(trim), C.c_void_p(d_out), int(out_cap),
                                    C.byref(n), C.byref(rep))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return int(n.value), rep

    def set_trim(self, trim=None):
        """A Trim: decode_host, decode_range_host and decode_pair_range_host trim the text they decoded before every other pass
        (get_trim() says what was cut); None: off."""
        self._check(lib().sfq_ctx_set_trim(self._h, None if trim is None else C.byref(trim)))

    def get_trim(self):
        """The TrimReport of the last decode call; None where it did not trim."""
        rep = TrimReport()
        rc = lib().sfq_get_trim(self._h, C.byref(rep))
        if rc < 0:
            self._check(rc)
        return rep if rc == 1 else None

    def overlap_pairs(self, d_text, nbytes, rule, d_out, out_cap):
        """The pairs of the interleaved FASTQ text in the device buffer at d_text, searched for the mates' overlap by the Overlap, and
        with rule.cut the text without the read-through into the one at d_out (sfq_overlap_pairs; d_out may be None where cut is 0);
        returns (bytes of the result, OverlapReport).  An SfqError of code E_OVERFLOW carries the size needed as .needed."""
        n, rep = C.c_uint64(), OverlapReport()
        rc = lib().sfq_overlap_pairs(self._h, C.c_void_p(d_text), int(nbytes), C.byref(rule), C.c_void_p(d_out), int(out_cap),
                                     C.byref(n), C.byref(rep))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return int(n.value), rep

    def set_overlap(self, rule=None):
        """An Overlap: decode_host, decode_range_host and decode_pair_range_host search the pairs of the text they decoded, behind the
        trim and in front of the selection, and with rule.cut cut the read-through (get_overlap() says what was found); None: off."""
        self._check(lib().sfq_ctx_set_overlap(self._h, None if rule is None else C.byref(rule)))

    def get_overlap(self):
        """The OverlapReport of the last decode call; None where it did not search."""
        rep = OverlapReport()
        rc = lib().sfq_get_overlap(self._h, C.byref(rep))
        if rc < 0:
            self._check(rc)
        return rep if rc == 1 else None

    def merge_pairs(self, d_text, nbytes, rule, d_out, out_cap):
        """The pairs of the interleaved FASTQ text in the device buffer at d_text, merged by the Merge into the one at d_out: the merged
        records, then the pairs that do not merge (sfq_merge_pairs); returns (bytes of the result, bytes of its merged part,
        MergeReport).  An SfqError of code E_OVERFLOW carries the size needed as .needed."""
        n, m, rep = C.c_uint64(), C.c_uint64(), MergeReport()
        rc = lib().sfq_merge_pairs(self._h, C.c_void_p(d_text), int(nbytes), C.byref(rule), C.c_void_p(d_out), int(out_cap),
                                   C.byref(n), C.byref(m), C.byref(rep))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return int(n.value), int(m.value), rep

    def set_merge(self, rule=None):
        """A Merge: decode_host, decode_range_host and decode_pair_range_host merge the pairs of the text they decoded, behind the trim
        and the selection and in front of the split and the pick; the result is [merged part | rest] (get_merge() says what was found
        and where the rest begins); None: off."""
        self._check(lib().sfq_ctx_set_merge(self._h, None if rule is None else C.byref(rule)))

    def get_merge(self):
        """(MergeReport, bytes of the merged part in the result as handed back) of the last decode call; None where it did not merge."""
        rep, m = MergeReport(), C.c_uint64()
        rc = lib().sfq_get_merge(self._h, C.byref(rep), C.byref(m))
        if rc < 0:
            self._check(rc)
        return (rep, int(m.value)) if rc == 1 else None

    def dedup_records(self, d_text, nbytes, rule, d_out, out_cap):
        """The units (records, or pairs) of the FASTQ text in the device buffer at d_text whose base lines no earlier unit has --
        nor, with rule.use_set, a unit an earlier call kept --, whole and in order, into the one at d_out (sfq_dedup_records);
        returns (bytes written, DedupReport).  An SfqError of code E_OVERFLOW carries the size needed as .needed."""
        n, rep = C.c_uint64(), DedupReport()
        rc = lib().sfq_dedup_records(self._h, C.c_void_p(d_text), int(nbytes), C.byref(rule), C.c_void_p(d_out), int(out_cap),
                                     C.byref(n), C.byref(rep))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return int(n.value), rep

    def dedup_set_create(self, max_keys, max_key_bytes, pairs=0):
        """The context's one set of keys, of fixed capacity, that calls with use_set share (sfq_dedup_set_create)."""
        self._check(lib().sfq_dedup_set_create(self._h, int(max_keys), int(max_key_bytes), int(pairs)))

    def dedup_set_clear(self):
        """Empties the set and keeps its memory."""
        self._check(lib().sfq_dedup_set_clear(self._h))

    def dedup_set_destroy(self):
        """Destroys the set; nothing to do where there is none."""
        self._check(lib().sfq_dedup_set_destroy(self._h))

    def dedup_set_info(self):
        """(keys, key bytes, max_keys, max_key_bytes) of the set; None where there is none."""
        v = [C.c_uint64() for _ in range(4)]
        rc = lib().sfq_dedup_set_info(self._h, *[C.byref(x) for x in v])
        if rc < 0:
            self._check(rc)
        return tuple(int(x.value) for x in v) if rc == 1 else None

    def set_dedup(self, rule=None):
        """A Dedup: decode_host, decode_range_host and decode_pair_range_host return the distinct units of the text they decoded,
        behind the selection and in front of the merge, the split and the pick (get_dedup() says what was found); None: off."""
        self._check(lib().sfq_ctx_set_dedup(self._h, None if rule is None else C.byref(rule)))

    def get_dedup(self):
        """The DedupReport of the last decode call; None where it dropped no duplicates."""
        rep = DedupReport()
        rc = lib().sfq_get_dedup(self._h, C.byref(rep))
        if rc < 0:
            self._check(rc)
        return rep if rc == 1 else None

    def demux_records(self, d_text, nbytes, rule, barcodes, d_out, out_cap):
        """The units (records, or pairs) of the FASTQ text in the device buffer at d_text sorted by the sample whose barcode they
        carry, every sample's in their original order, the unassigned last, into the one at d_out (sfq_demux_records); returns
        (bytes written, part offsets [NP + 1], units per sample [n_samples + 1], DemuxReport).  An SfqError of code E_OVERFLOW
        carries the size needed as .needed."""
        n, rep = C.c_uint64(), DemuxReport()
        off, units = (C.c_uint64 * (rule.n_parts + 1))(), (C.c_uint64 * (rule.n_samples + 1))()
        rc = lib().sfq_demux_records(self._h, C.c_void_p(d_text), int(nbytes), C.byref(rule), _barcode_rows(barcodes, rule), C.c_void_p(d_out),
                                     int(out_cap), C.byref(n), off, units, C.byref(rep))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return int(n.value), list(off), list(units), rep

    def set_demux(self, rule=None, barcodes=None):
        """A Demux and its barcode rows: decode_host and decode_range_host return the text they decoded partitioned by sample,
        behind the dedup, as the call's last pass (get_demux() says where the parts lie); None: off."""
        self._check(lib().sfq_ctx_set_demux(self._h, None if rule is None else C.byref(rule),
                                            None if barcodes is None else _barcode_rows(barcodes, rule)))
        self._demux_entries = 0 if rule is None else rule.n_parts + 1
        self._demux_samples = 0 if rule is None else rule.n_samples

    def get_demux(self):
        """(DemuxReport, part offsets, units per sample) of the last decode call; None where it did not demultiplex."""
        rep, cap = DemuxReport(), max(getattr(self, "_demux_entries", 0), 1)
        off, units = (C.c_uint64 * cap)(), (C.c_uint64 * cap)()
        rc = lib().sfq_get_demux(self._h, C.byref(rep), off, units, cap)
        if rc < 0:
            self._check(rc)
        if rc != 1:
            return None
        return rep, list(off), list(units)[:getattr(self, "_demux_samples", 0) + 1]

    def screen_records(self, d_text, nbytes, rule, d_out, out_cap):
        """The units (records, or pairs) of the FASTQ text in the device buffer at d_text that the rule keeps -- those whose base
        lines share too few k-mers with the context's set, or with rule.keep_matched only the others --, whole and in order, into
        the one at d_out (sfq_screen_records); returns (bytes written, ScreenReport).  An SfqError of code E_OVERFLOW carries the
        size needed as .needed."""
        n, rep = C.c_uint64(), ScreenReport()
        rc = lib().sfq_screen_records(self._h, C.c_void_p(d_text), int(nbytes), C.byref(rule), C.c_void_p(d_out), int(out_cap),
                                      C.byref(n), C.byref(rep))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return int(n.value), rep

    def screen_set_create(self, k, max_kmers):
        """The context's one set of reference k-mers, of fixed capacity (sfq_screen_set_create)."""
        self._check(lib().sfq_screen_set_create(self._h, int(k), int(max_kmers)))

    def screen_set_add(self, seq: bytes):
        """The k-mers of a sequence text (host bytes; any byte but ACGTacgt separates sequences) into the set; E_NOMEM where they do
        not fit, and the set is empty then."""
        self._check(lib().sfq_screen_set_add(self._h, seq, len(seq)))

    def screen_set_clear(self):
        """Empties the set and keeps its memory."""
        self._check(lib().sfq_screen_set_clear(self._h))

    def screen_set_destroy(self):
        """Destroys the set; nothing to do where there is none."""
        self._check(lib().sfq_screen_set_destroy(self._h))

    def screen_set_info(self):
        """(k, k-mers, max_kmers) of the set; None where there is none."""
        k, v = C.c_uint32(), [C.c_uint64() for _ in range(2)]
        rc = lib().sfq_screen_set_info(self._h, C.byref(k), *[C.byref(x) for x in v])
        if rc < 0:
            self._check(rc)
        return (int(k.value),) + tuple(int(x.value) for x in v) if rc == 1 else None

    def set_screen(self, rule=None):
        """A Screen: decode_host, decode_range_host and decode_pair_range_host return the units of the text they decoded that the
        rule keeps, behind the selection and in front of the dedup, the merge, the split and the pick (get_screen() says what was
        found); None: off."""
        self._check(lib().sfq_ctx_set_screen(self._h, None if rule is None else C.byref(rule)))

    def get_screen(self):
        """The ScreenReport of the last decode call; None where it did not screen."""
        rep = ScreenReport()
        rc = lib().sfq_get_screen(self._h, C.byref(rep))
        if rc < 0:
            self._check(rc)
        return rep if rc == 1 else None

    def bgzf_deflate(self, d_text, bounds, d_out, out_cap):
        """The parts [bounds[i], bounds[i + 1]) of the device buffer at d_text as BGZF members into the one at d_out
        (sfq_bgzf_deflate); returns (part offsets [n_parts + 1], BgzfReport).  bounds: at least two non-decreasing integers, a
        ValueError otherwise.  An SfqError of code E_OVERFLOW carries the size needed as .needed."""
        bounds = [int(x) for x in bounds]
        if len(bounds) < 2:
            raise ValueError("bounds: %d entries, a part has two" % len(bounds))
        if any(b < 0 for b in bounds) or any(b < a for a, b in zip(bounds, bounds[1:])):
            raise ValueError("bounds: negative or decreasing")
        n = len(bounds) - 1
        b = (C.c_uint64 * (n + 1))(*bounds)
        off, rep = (C.c_uint64 * (n + 1))(), BgzfReport()
        rc = lib().sfq_bgzf_deflate(self._h, C.c_void_p(d_text), b, n, C.c_void_p(d_out), int(out_cap), off, C.byref(rep))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(rep.out_bytes)
            raise
        return list(off), rep

    def set_bgzf(self, on=True):
        """decode_host, decode_range_host and decode_pair_range_host return BGZF bytes instead of text, as the call's last pass
        (get_bgzf() says where the parts lie); False: off."""
        self._check(lib().sfq_ctx_set_bgzf(self._h, int(bool(on))))

    def get_bgzf(self, max_parts=8200):
        """(BgzfReport, part offsets [NP + 1], text bytes per part [NP]) of the last decode call; None where it did not deflate."""
        rep, cap = BgzfReport(), int(max_parts) + 1
        off, text = (C.c_uint64 * cap)(), (C.c_uint64 * cap)()
        for i in range(cap):
            off[i] = 0xFFFFFFFFFFFFFFFF
        rc = lib().sfq_get_bgzf(self._h, C.byref(rep), off, text, cap)
        if rc < 0:
            self._check(rc)
        if rc != 1:
            return None
        np_ = next((i for i in range(cap) if off[i] == 0xFFFFFFFFFFFFFFFF), cap) - 1
        return rep, list(off)[:np_ + 1], list(text)[:np_]

    def set_block_checksums(self, crcs):
        """The expected CRCs of the next decode call's blocks (consumed by it)."""
        arr = (C.c_uint32 * max(len(crcs), 1))(*[c & 0xFFFFFFFF for c in crcs])
        self._check(lib().sfq_set_block_checksums(self._h, arr, len(crcs)))

    def crc32(self, d_ptr, bounds):
        """zlib.crc32 of every range [bounds[i], bounds[i+1]) of the device buffer at d_ptr."""
        n = len(bounds) - 1
        if n <= 0:
            return []
        b = (C.c_uint64 * len(bounds))(*[int(x) for x in bounds])
        out = (C.c_uint32 * n)()
        self._check(lib().sfq_crc32(self._h, C.c_void_p(d_ptr), b, n, out))
        return list(out)

    def index(self, n_blocks):
        blocks = (BlockInfo * n_blocks)()
        got = lib().sfq_get_block_index(self._h, blocks, n_blocks)
        if got < 0:
            self._check(got)
        return blocks

    def first_headers(self, nbytes):
        buf = C.create_string_buffer(max(int(nbytes), 1))
        self._check(lib().sfq_get_first_headers(self._h, buf, nbytes))
        return buf.raw[:nbytes]

    def prior(self) -> bytes:
        n = lib().sfq_get_qlt_prior(self._h, None, 0)
        if n <= 0:
            return b""
        buf = C.create_string_buffer(n)
        lib().sfq_get_qlt_prior(self._h, buf, n)
        return buf.raw[:n]

    def rec_prior(self) -> bytes:
        n = lib().sfq_get_rec_prior(self._h, None, 0)
        if n <= 0:
            return b""
        buf = C.create_string_buffer(n)
        lib().sfq_get_rec_prior(self._h, buf, n)
        return buf.raw[:n]

    def build_priors(self, d_ptr, nbytes, level=3, block_reads=BLOCK_AUTO, prior_step=PRIOR_AUTO, tables=1):
        """Priors of a device-resident text (quality prior, header prior); install elsewhere with set_priors()."""
        p = Params(level, block_reads, 0, 0, 0, 0, prior_step, tables, 0, 0)
        self._check(lib().sfq_build_priors(self._h, C.c_void_p(d_ptr), nbytes, C.byref(p)))
        return self.prior(), self.rec_prior()

    def count_priors(self, d_ptr, nbytes, level=3, block_reads=BLOCK_AUTO, prior_step=PRIOR_AUTO, tables=1, sample_scale=1):
        """The sample COUNTS of a device-resident text (every sample_scale-th record of the automatic sample): for several
        ranks that add their counts up (dist.allreduce_prior_counts) and code with prior_step = PRIOR_COUNTS."""
        p = Params(level, block_reads, 0, 0, 0, 0, prior_step, tables, 0, 0)
        self._check(lib().sfq_count_priors(self._h, C.c_void_p(d_ptr), nbytes, C.byref(p), sample_scale))

    @staticmethod
    def prior_counts_words(level=3):
        nq, nr = C.c_uint64(), C.c_uint64()
        lib().sfq_prior_counts_words(level, C.byref(nq), C.byref(nr))
        return nq.value, nr.value

    def get_prior_counts(self, level, d_qlt, d_rec):
        self._check(lib().sfq_get_prior_counts(self._h, level, C.c_void_p(d_qlt), C.c_void_p(d_rec)))

    def set_prior_counts(self, level, d_qlt, d_rec):
        self._check(lib().sfq_set_prior_counts(self._h, level, C.c_void_p(d_qlt), C.c_void_p(d_rec)))

    def set_priors(self, prior: bytes, rec_prior: bytes = b""):
        L = lib()
        self._check(L.sfq_set_qlt_prior(self._h, prior if prior else None, len(prior)))
        self._check(L.sfq_set_rec_prior(self._h, rec_prior if rec_prior else None, len(rec_prior)))

    def chains(self) -> bytes:
        n = lib().sfq_get_chain_index(self._h, None, 0)
        if n <= 0:
            return b""
        buf = C.create_string_buffer(n)
        lib().sfq_get_chain_index(self._h, buf, n)
        return buf.raw[:n]

    def encode_host(self, fastq: bytes, level=3, block_reads=0, gen_bits=0, models=0, kernel=0, prior_step=0, tables=0,
                    chain_reads=0, lds_rows=0) -> Encoded:
        L = lib()
        p = Params(level, block_reads, gen_bits, models, kernel, 0, prior_step, tables, chain_reads, lds_rows)
        res = Result()
        cap = L.sfq_encode_bound(len(fastq))
        out = np.empty(cap, np.uint8)
        src = np.frombuffer(fastq, np.uint8)
        self._check(L.sfq_encode_blocks_host(self._h, src.ctypes.data_as(C.c_void_p), len(fastq), C.byref(p),
                                             out.ctypes.data_as(C.c_void_p), cap, C.byref(res)))
        return self._encoded(res, out)

    def _encoded(self, res, out) -> Encoded:
        """What the last *_host encode call left in the context, with its streams in out."""
        blocks = self.index(res.n_blocks)
        crcs, text_crc = self.checksums()
        on = len(crcs) == res.n_blocks and res.n_blocks > 0
        return Encoded(res, blocks, self.first_headers(res.first_hdr_bytes), out[:res.total_bytes].copy(), self.prior(), self.chains(), self.rec_prior(),
                       crcs if on else None, text_crc if on else None, self.text_stats())

    def encode_pairs_host(self, fastq_a: bytes, fastq_b: bytes, level=3, block_reads=0, gen_bits=0, models=0, kernel=0, prior_step=0,
                          tables=0, chain_reads=0, lds_rows=0) -> Encoded:
        """encode_host of the two texts interleaved record by record on the device (sfq_encode_pairs_host)."""
        L = lib()
        p = Params(level, block_reads, gen_bits, models, kernel, 0, prior_step, tables, chain_reads, lds_rows)
        res = Result()
        cap = L.sfq_encode_bound(len(fastq_a) + len(fastq_b))
        out = np.empty(cap, np.uint8)
        a, b = np.frombuffer(fastq_a, np.uint8), np.frombuffer(fastq_b, np.uint8)
        self._check(L.sfq_encode_pairs_host(self._h, a.ctypes.data_as(C.c_void_p), len(fastq_a), b.ctypes.data_as(C.c_void_p), len(fastq_b),
                                            C.byref(p), out.ctypes.data_as(C.c_void_p), cap, C.byref(res)))
        return self._encoded(res, out)

    def encode_device(self, d_ptr, nbytes, d_out, out_cap, level=3, block_reads=0, gen_bits=0, models=0, kernel=0, qlt_only=False,
                      prior_step=0, tables=0, chain_reads=0, lds_rows=0):
        """Device-pointer entry point (ints from torch .data_ptr()). Returns the Result struct."""
        L = lib()
        p = Params(level, block_reads, gen_bits, models, kernel, 0, prior_step, tables, chain_reads, lds_rows)
        res = Result()
        f = L.sfq_encode_qlt_blocks if qlt_only else L.sfq_encode_blocks
        self._check(f(self._h, C.c_void_p(d_ptr), nbytes, C.byref(p), C.c_void_p(d_out), out_cap, C.byref(res)))
        return res

    def decode_device(self, blocks, first_hdrs: bytes, d_streams, stream_offset, d_out, out_cap, prior=b"", level=3, version=0,
                      chains=b"", lds_rows=0, rec_prior=b"", kernel=0):
        """Device-pointer decode (ints from torch .data_ptr()): returns (bytes written, Result)."""
        L = lib()
        self._check(L.sfq_set_qlt_prior(self._h, prior if prior else None, len(prior)))
        self._check(L.sfq_set_chain_index(self._h, chains if chains else None, len(chains)))
        self._check(L.sfq_set_rec_prior(self._h, rec_prior if rec_prior else None, len(rec_prior)))
        p = Params(level, 0, 0, 0, kernel, version, 0, 0, 0, lds_rows)
        res = Result()
        n = C.c_uint64()
        fb = np.frombuffer(first_hdrs if len(first_hdrs) else b"\0", np.uint8)
        soff = (C.c_uint64 * NSTREAMS)(*list(stream_offset))
        self._check(L.sfq_decode_blocks(self._h, C.byref(p), blocks, len(blocks), fb.ctypes.data_as(C.c_void_p), len(first_hdrs),
                                        C.c_void_p(d_streams), soff, C.c_void_p(d_out), out_cap, C.byref(n), C.byref(res)))
        return n.value, res

    def decode_host(self, enc_or_parts, level=3, version=0, out_cap=None, kernel=0, lds_rows=0) -> bytes:
        """Decode an Encoded (or a (blocks, first_hdrs, data, stream_offset) tuple) back to FASTQ text."""
        L = lib()
        prior = chains = rec_prior = b""
        crcs = None
        if isinstance(enc_or_parts, Encoded):
            blocks, first, data, prior, chains = enc_or_parts.blocks, enc_or_parts.first_hdrs, enc_or_parts.data, enc_or_parts.prior, enc_or_parts.chains
            rec_prior = enc_or_parts.rec_prior
            crcs = enc_or_parts.crcs
            soff = (C.c_uint64 * NSTREAMS)(*list(enc_or_parts.res.stream_offset))
        else:
            blocks, first, data, so = enc_or_parts[:4]
            if len(enc_or_parts) > 4:
                prior = enc_or_parts[4]
            if len(enc_or_parts) > 5:
                chains = enc_or_parts[5]
            if len(enc_or_parts) > 6:
                rec_prior = enc_or_parts[6]
            soff = (C.c_uint64 * NSTREAMS)(*so)
        self._check(L.sfq_set_qlt_prior(self._h, prior if prior else None, len(prior)))
        self._check(L.sfq_set_chain_index(self._h, chains if chains else None, len(chains)))
        self._check(L.sfq_set_rec_prior(self._h, rec_prior if rec_prior else None, len(rec_prior)))
        data = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8)) if not isinstance(data, np.ndarray) else data
        p = Params(level, 0, 0, 0, kernel, version, 0, 0, 0, lds_rows)
        res = Result()
        if crcs is not None:
            self.set_block_checksums(crcs)
        if out_cap is None:
            out_cap = 64 * len(data) + (1 << 20)
        out = np.empty(out_cap, np.uint8)
        n = C.c_uint64()
        fb = np.frombuffer(first if len(first) else b"\0", np.uint8)
        self._check(L.sfq_decode_blocks_host(self._h, C.byref(p), blocks, len(blocks), fb.ctypes.data_as(C.c_void_p), len(first),
                                             data.ctypes.data_as(C.c_void_p), len(data), soff,
                                             out.ctypes.data_as(C.c_void_p), out_cap, C.byref(n), C.byref(res)))
        return out[:n.value].tobytes()

    def decode_range_device(self, blocks, first_hdrs: bytes, d_streams, stream_offset, first_block, n_window, d_out, out_cap, prior=b"",
                            level=3, version=0, chains=b"", lds_rows=0, rec_prior=b"", kernel=0, crcs=None):
        """Device-pointer decode of blocks [first_block, first_block + n_window) of a call (sfq_decode_block_range): blocks, the first
        headers, stream_offset and the blobs are the whole call's; crcs: the window's expected CRCs.  Returns (bytes written, Result)."""
        L = lib()
        self._check(L.sfq_set_qlt_prior(self._h, prior if prior else None, len(prior)))
        self._check(L.sfq_set_chain_index(self._h, chains if chains else None, len(chains)))
        self._check(L.sfq_set_rec_prior(self._h, rec_prior if rec_prior else None, len(rec_prior)))
        if crcs is not None:
            self.set_block_checksums(crcs)
        p = Params(level, 0, 0, 0, kernel, version, 0, 0, 0, lds_rows)
        res = Result()
        n = C.c_uint64()
        fb = np.frombuffer(first_hdrs if len(first_hdrs) else b"\0", np.uint8)
        soff = (C.c_uint64 * NSTREAMS)(*list(stream_offset))
        self._check(L.sfq_decode_block_range(self._h, C.byref(p), blocks, len(blocks), fb.ctypes.data_as(C.c_void_p), len(first_hdrs),
                                             C.c_void_p(d_streams), soff, first_block, n_window, C.c_void_p(d_out), out_cap,
                                             C.byref(n), C.byref(res)))
        return n.value, res

    def decode_range_host(self, enc: Encoded, first_block, n_window, level=3, version=0, out_cap=None, kernel=0, lds_rows=0, crcs=None):
        """Blocks [first_block, first_block + n_window) of an Encoded back to FASTQ text (sfq_decode_block_range_host); crcs: the
        window's expected CRCs (default: the window's share of enc.crcs, where the encode computed them).  Returns (text, Result)."""
        L = lib()
        self._check(L.sfq_set_qlt_prior(self._h, enc.prior if enc.prior else None, len(enc.prior)))
        self._check(L.sfq_set_chain_index(self._h, enc.chains if enc.chains else None, len(enc.chains)))
        self._check(L.sfq_set_rec_prior(self._h, enc.rec_prior if enc.rec_prior else None, len(enc.rec_prior)))
        data = enc.data if isinstance(enc.data, np.ndarray) else np.ascontiguousarray(np.frombuffer(bytes(enc.data), np.uint8))
        if crcs is None and enc.crcs is not None:
            crcs = enc.crcs[first_block:first_block + n_window]
        if crcs is not None:
            self.set_block_checksums(crcs)
        p = Params(level, 0, 0, 0, kernel, version, 0, 0, 0, lds_rows)
        res = Result()
        if out_cap is None:
            out_cap = 64 * len(data) + (1 << 20)
        out = np.empty(out_cap, np.uint8)
        n = C.c_uint64()
        fb = np.frombuffer(enc.first_hdrs if len(enc.first_hdrs) else b"\0", np.uint8)
        soff = (C.c_uint64 * NSTREAMS)(*list(enc.res.stream_offset))
        self._check(L.sfq_decode_block_range_host(self._h, C.byref(p), enc.blocks, len(enc.blocks), fb.ctypes.data_as(C.c_void_p), len(enc.first_hdrs),
                                                  data.ctypes.data_as(C.c_void_p), len(data), soff, first_block, n_window,
                                                  out.ctypes.data_as(C.c_void_p), out_cap, C.byref(n), C.byref(res)))
        return out[:n.value].tobytes(), res

    def decode_pair_range_host(self, enc: Encoded, first_pair, n_pairs, level=3, version=0, out_cap=None, kernel=0, lds_rows=0, crcs=None):
        """Pairs [first_pair, first_pair + n_pairs) of an Encoded written from paired files (sfq_decode_pair_range_host); crcs: the
        expected CRCs of the blocks pair_window_blocks names (default: their share of enc.crcs, where the encode computed them).
        Returns (the first mates, the second mates, Result)."""
        L = lib()
        self._check(L.sfq_set_qlt_prior(self._h, enc.prior if enc.prior else None, len(enc.prior)))
        self._check(L.sfq_set_chain_index(self._h, enc.chains if enc.chains else None, len(enc.chains)))
        self._check(L.sfq_set_rec_prior(self._h, enc.rec_prior if enc.rec_prior else None, len(enc.rec_prior)))
        data = enc.data if isinstance(enc.data, np.ndarray) else np.ascontiguousarray(np.frombuffer(bytes(enc.data), np.uint8))
        if crcs is None and enc.crcs is not None:
            w = pair_window_blocks(enc.blocks, first_pair, n_pairs)
            crcs = enc.crcs[w[0]:w[0] + w[1]] if w is not None else None
        if crcs:                                               # (an empty list: none are installed)
            self.set_block_checksums(crcs)
        p = Params(level, 0, 0, 0, kernel, version, 0, 0, 0, lds_rows)
        res = Result()
        if out_cap is None:
            out_cap = 64 * len(data) + (1 << 20)
        out = np.empty(out_cap, np.uint8)
        n, split = C.c_uint64(), C.c_uint64()
        fb = np.frombuffer(enc.first_hdrs if len(enc.first_hdrs) else b"\0", np.uint8)
        soff = (C.c_uint64 * NSTREAMS)(*list(enc.res.stream_offset))
        rc = L.sfq_decode_pair_range_host(self._h, C.byref(p), enc.blocks, len(enc.blocks), fb.ctypes.data_as(C.c_void_p), len(enc.first_hdrs),
                                          data.ctypes.data_as(C.c_void_p), len(data), soff, int(first_pair), int(n_pairs),
                                          out.ctypes.data_as(C.c_void_p), out_cap, C.byref(n), C.byref(split), C.byref(res))
        try:
            self._check(rc)
        except SfqError as e:
            e.needed = int(n.value)
            raise
        return out[:split.value].tobytes(), out[split.value:n.value].tobytes(), res

    @staticmethod
    def pair_window_blocks(blocks, first_pair, n_pairs):
        return pair_window_blocks(blocks, first_pair, n_pairs)


def pair_window_blocks(blocks, first_pair, n_pairs):
    """(first block, blocks) that hold pairs [first_pair, first_pair + n_pairs) of a call's block index (sfq_pair_window_blocks, no
    GPU); None where there is no such window."""
    if not isinstance(blocks, C.Array):
        blocks = (BlockInfo * max(len(blocks), 1))(*blocks)
    b0, nw = C.c_uint32(), C.c_uint32()
    rc = lib().sfq_pair_window_blocks(blocks, len(blocks), int(first_pair), int(n_pairs), C.byref(b0), C.byref(nw))
    return (int(b0.value), int(nw.value)) if rc == 0 else None

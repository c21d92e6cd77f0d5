"""The device entries of the C ABI -- sfq_encode_blocks, sfq_encode_qlt_blocks, sfq_build_priors, sfq_count_priors, sfq_decode_blocks,
sfq_decode_block_range -- on texts, streams and outputs that lie ANYWHERE in the caller's device memory: at every kind of offset from a
sixteen-byte boundary and between guard bytes that would change the answer if a kernel ever used them (util.Placed: a piece of FASTQ that
goes on behind the text -- line ends, '@', '+', '!', N-like and lower-case bytes --, and 0xFF throughout).  Every other test of the coding
path hands in the context's own staging buffer or a fresh tensor: sixteen-byte aligned, with slack behind it.

Expected values come from the oracle, computed once per text and mode: the first placement's result -- the control, (0, 0) -- goes through
check_against_oracle / util.block_reference / O.compress, every other placement and fill must give the control's bytes, stream for stream and
blob for blob (same_encoded names the first stream and byte that differ).  After every call the guards and the input come back byte for byte.
The encoder's output buffer holds sfq_encode_bound(n) bytes exactly, the decoder's exactly the text.

  test_texts_are_what_the_gpu_tests_rely_on   CPU.  Every text below is built; lengths on the framing's borders, the last record's N over '!',
      the genome-like text's verdict ("on", by the oracle), and the oracle codes and decodes each of them in the modes it is used in.
  test_frozen_tables...   sfq_encode_blocks with frozen tables, lds_rows none and 64 (both quality kernels), then sfq_decode_blocks.
  test_adaptive_blocks... / test_format_6...   adaptive tables, blocks and one block, default and cross-check kernels, both ways.
  test_long_records_in_segments...   chains that are segments of a record.
  test_quality_entry...   sfq_encode_qlt_blocks.
  test_priors_entries...   sfq_build_priors; sfq_count_priors + SFQ_PRIOR_COUNTS on the same pointer (the one path through k_text_fingerprint).
  test_block_windows...   sfq_decode_block_range: a window in the middle and the last one.
"""
import functools
import os
import re

import numpy as np
import pytest

import util
from oracle import oracle as O
from slimfastq_amd import capi
from util import FILLS, PLACEMENTS, Placed, first_difference
from test_frozen_tables import (PRIOR_SYMBOLS, SEG, _exception_heavy_fastq, _folded_genome_reads, _long_reads, _odd_headers_fastq,
                                base_chains_oracle, check_against_oracle, gm_chain_reads, gm_table_bits, rec_sample)
from test_gpu_parity import KERNELS, _fuzz_fastq, _pad_to
assert KERNELS == (0, 1)
from test_pairs import reads, records

FROZEN, ADAPTIVE = capi.TABLES_FROZEN, capi.TABLES_ADAPTIVE


def frame_borders():
    """The sizes k_frame lays from the text's first byte: its 64-byte window, its sub-tile and its tile, read from frame.hip"""
    src = open(os.path.join(os.path.dirname(capi.__file__), "csrc", "frame.hip")).read()
    sub = int(re.search(r"^#define FRAME_SUB (\d+)u\s*$", src, re.M).group(1))
    win = int(re.search(r"^#define FRAME_WIN (\d+)\s*$", src, re.M).group(1))
    assert re.search(r"^#define FRAME_TILE \(FRAME_SUB \* FRAME_WIN\)\s*$", src, re.M) and re.search(r"^#define FRAME_NW \(FRAME_TILE / 64u\)", src, re.M)
    return 64, sub, sub * win


BORDERS = frame_borders()


# ---- the texts: each a function of its arguments ---------------------------------------------------------------------------------------------
def last_record(L, seed):
    """A record whose base and quality lines are L long and end in an N over a '!': the marks of the text's last bytes are live"""
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].copy(); seq[-1] = ord("N")
    qual = rng.integers(ord("5"), ord("J"), L, dtype=np.uint8); qual[-1] = ord("!")
    return b"@z%d\n" % L + seq.tobytes() + b"\n+\n" + qual.tobytes() + b"\n"


def text_of_length(total):
    """Ragged records, then last_record(20): `total` bytes exactly, the first headers padded as test_gpu_parity._pad_to does"""
    last = last_record(20, total)
    if total < 256:
        recs = [b"@r0\nACGT\n+\nI5I5\n", b"@r1\nNA\n+\n!I\n"]
        last = b"@z\nCN\n+\nI!\n"
    else:
        pool = records(reads(total // 60 + 8, 1, 120, seed=total))
        recs, size = [], 0
        for r in pool:
            if size + len(r) + len(last) > total:
                break
            recs.append(r); size += len(r)
    recs = _pad_to(recs + [last], len(recs) + 1, total, 1 << 30, 0)
    return b"".join(recs)


# name -> (text, level, block_reads, chain_reads): small blocks and chains, as the tests of the aligned path choose them
@functools.lru_cache(maxsize=None)
def text(name):
    fq, level, br, cr = _text(name)
    return fq, level, br, min(cr, fq.count(b"\n") // 4)                       # (a call's chains hold no more records than the text has)


def _text(name):
    kind, _, arg = name.partition(":")
    if kind == "one":
        return b"@a\nA\n+\nI\n", 3, 64, 7
    if kind == "tiny":                                                        # a text of 17 .. 40 bytes
        return b"@t 1\nACGNT\n+\nII!I5\n@t 2\nN\n+\n!\n", 3, 64, 7
    if kind == "last":                                                        # about 300 ragged records, the last of every length
        return reads(299, 1, 40, seed=int(arg)) + last_record(int(arg), 7), 3, 100, 13
    if kind == "border":                                                      # the text ends on, before and behind a border of the framing
        total = BORDERS["WST".index(arg[0])] + int(arg[1:] or 0)              # W: the window, S: the sub-tile, T: the tile
        return text_of_length(total), 3, (64 if total < 40000 else 200), (7 if total < 40000 else 33)
    if kind == "fuzz":                                                        # test_gpu_parity's structurally hostile texts
        return _fuzz_fastq(np.random.default_rng(1000 + int(arg)), 150), (1, 4)[int(arg) % 2], 97, 11
    if kind == "exc":
        return _exception_heavy_fastq(600, 33), 3, 150, 7
    if kind == "genome":                                                      # the suite's smallest text that the match model takes
        return _folded_genome_reads(), 3, 128, 32
    if kind == "oddhdr":                                                      # headers outside the fast header kernels' envelope
        return _odd_headers_fastq(300, 5), 3, 200, 50
    raise KeyError(name)


LAST = ["last:%d" % L for L in (1, 15, 16, 17, 63, 64, 65)]
BORDER = ["border:%s%s" % (b, d) for b in "WST" for d in ("-1", "", "+1")]
SMALL = ["one"] + LAST + BORDER + ["fuzz:0", "fuzz:1", "exc", "oddhdr"]
FROZEN_TEXTS = SMALL + ["genome"]
# format 6 is one wave (9 MB/s, 2.7 back) and refuses 'n' beside 'N' (gens.cpp:107-108): no exception-heavy text, one text past the tile's border
FORMAT6_TEXTS = [n for n in SMALL if n not in ("exc", "border:T-1", "border:T")]
# the cross-check kernels are one LANE a block: the texts of every kind, the smaller ones
THIN = ["one", "last:1", "last:17", "last:64", "border:W", "border:S+1", "fuzz:1"]
PRIOR_TEXTS = ["one", "tiny", "last:17", "border:S+1", "fuzz:1", "oddhdr"]
SEGMENTS = ((1000, 4, False), (700, 7, True), (4096, 3, False))               # test_long_records_are_cut_into_segments: seg, br, qdiff


def segment_text(seg, br, qdiff):
    return _long_reads(np.random.default_rng(seg + br), 8, 2500, 9000, qdiff)


def window_records(fq, br, first, count):
    return b"".join(util.split_records(fq, br)[first:first + count])


# ---- 4. the texts themselves (no GPU) ----------------------------------------------------------------------------------------------------------
def test_texts_are_what_the_gpu_tests_rely_on():
    assert BORDERS[0] == 64 and BORDERS[1] % 64 == 0 and BORDERS[2] % BORDERS[1] == 0 and BORDERS[2] > BORDERS[1]
    assert len(text("one")[0]) < 16 and 17 <= len(text("tiny")[0]) <= 40
    for i, L in enumerate((1, 15, 16, 17, 63, 64, 65)):
        fq = text(LAST[i])[0]
        lines = fq.split(b"\n")
        assert len(lines) == 4 * 300 + 1 and len(lines[-4]) == L and len(lines[-2]) == L
    want = [b + d for b in BORDERS for d in (-1, 0, 1)]
    assert [len(text(n)[0]) for n in BORDER] == want
    for n in LAST + BORDER + ["tiny"]:
        lines = text(n)[0].split(b"\n")
        assert lines[-1] == b"" and lines[-4].endswith(b"N") and lines[-2].endswith(b"!"), n
    fq = text("oddhdr")[0]
    hdrs = fq.split(b"\n")[0::4]
    assert max(len(h) for h in hdrs) > 128 and any(h.startswith(b"@hex.") for h in hdrs)
    assert len({text("fuzz:0")[0], text("fuzz:1")[0]}) == 2
    for n in FORMAT6_TEXTS:
        assert len(text(n)[0]) < 150_000, n                                   # (format 6 is one wave: 9 MB/s)
    # the oracle codes and decodes every text: under the block format's rules (lossless), and the reference's where format 6 is run
    for n in SMALL + ["tiny"]:
        fq, level, br, cr = text(n)
        assert fq == _text(n)[0]
        assert O.decompress(util.block_reference(fq, level).image) == fq, n
        if n in FORMAT6_TEXTS:
            back = O.decompress(O.compress(fq, level).image)                  # (lossy where the reference is: SURVEY H7)
            assert back.count(b"\n") == fq.count(b"\n"), n
    with pytest.raises(O.OracleError):
        O.compress(text("exc")[0], 3)
    for seg, br, qdiff in SEGMENTS:
        fq = segment_text(seg, br, qdiff)
        starts, lens = util.line_table(fq)
        assert int(O.seg_counts(lens[1::4], lens[3::4], seg).max()) >= 2 and len(fq) < 150_000
        assert O.decompress(util.block_reference(fq, 3).image) == fq
    # the genome-like text: the match model's verdict is "on", and its chains decode to the text's bases
    fq, level, br, cr = text("genome")
    starts, lens = util.line_table(fq)
    nrec = len(starts) // 4
    gcr, tb = gm_chain_reads(len(fq), nrec, br, cr), gm_table_bits(len(fq))
    streams, sizes, on = O.gm_encode_chains(fq, starts[1::4], lens[1::4], tb, br, gcr)
    assert on == 1
    code = np.zeros(256, np.uint8)
    for ch, v in zip("ACGT", range(4)):
        code[ord(ch)] = v
    a = np.frombuffer(fq, np.uint8)
    lines = fq.split(b"\n")[1::4]
    assert np.array_equal(O.gm_decode_chains(streams, sizes, lens[1::4], tb, br, gcr), code[np.frombuffer(b"".join(lines), np.uint8)])
    assert a[int(starts[1])] in b"ACGT"


# ---- the calls ---------------------------------------------------------------------------------------------------------------------------------
def where(entry, mode, place, fill):
    return "%s, %s, text/streams at +%d, output at +%d, guards '%s'" % (entry, mode, place[0], place[1], fill)


def block_fields(enc):
    return [(b.first_record, b.n_records, b.llen, b.solid, b.two_id, b.n_byte, b.gen_bits, b.extra_hi, b.first_hdr_len, b.first_hdr_off,
             tuple(b.size), b.status, b.hdr_bytes) for b in enc.blocks]


def same_encoded(got, want, what):
    """Every stream, the priors, the chain index, the first headers and the block index of two encode calls, byte for byte"""
    for name in capi.STREAM_NAMES:
        first_difference(got.stream(name), want.stream(name), "%s: stream %s" % (what, name))
    for blob in ("prior", "rec_prior", "chains", "first_hdrs"):
        first_difference(getattr(got, blob), getattr(want, blob), "%s: %s" % (what, blob))
    assert block_fields(got) == block_fields(want), what + ": the block index"
    assert (got.res.n_records, got.res.n_blocks, got.res.n_chains, got.res.total_bytes) == \
           (want.res.n_records, want.res.n_blocks, want.res.n_chains, want.res.total_bytes), what
    assert list(got.res.stream_offset) == list(want.res.stream_offset) and list(got.res.stream_bytes) == list(want.res.stream_bytes), what


def encode_placed(ctx, fq, place, fill, what, src=None, **kw):
    """sfq_encode_blocks (qlt_only: sfq_encode_qlt_blocks) of the text placed at place[0] into sfq_encode_bound(n) bytes placed at place[1]"""
    src = src or Placed(len(fq), place[0], fill, fq)
    cap = capi.lib().sfq_encode_bound(len(fq))
    dst = Placed(cap, place[1], fill)
    res = ctx.encode_device(src.ptr, len(fq), dst.ptr, cap, **kw)
    assert dst.guards_intact(), what + ": a byte outside [d_out, d_out + out_cap) was written"
    first_difference(src.back(what + ": the input"), fq, what + ": the input text")
    return ctx._encoded(res, np.frombuffer(dst.head(res.total_bytes), np.uint8))


def decode_placed(ctx, enc, want, place, fill, what, level, window=None, **kw):
    """sfq_decode_blocks (window = (first, count): sfq_decode_block_range) of the streams placed at place[0] into len(want) bytes at place[1]"""
    data = enc.data.tobytes()
    src = Placed(len(data), place[0], fill, data)
    dst = Placed(len(want), place[1], fill)
    args = (enc.blocks, enc.first_hdrs, src.ptr, list(enc.res.stream_offset))
    kw = dict(kw, prior=enc.prior, level=level, chains=enc.chains, rec_prior=enc.rec_prior)
    if window is None:
        n, _ = ctx.decode_device(*args, dst.ptr, len(want), **kw)
    else:
        n, res = ctx.decode_range_device(*args, window[0], window[1], dst.ptr, len(want), **kw)
        assert res.n_blocks == window[1], what
    got = dst.back(what + ": the output")
    first_difference(src.back(what + ": the streams"), data, what + ": the streams")
    assert n == len(want), "%s: %d bytes written, want %d" % (what, n, len(want))
    first_difference(got, want, what + ": the text")


def everywhere():
    return [(place, fill) for place in PLACEMENTS for fill in FILLS]


_checked = {}                                            # (text, mode) -> an Encoded that has passed the oracle (test_block_windows reuses them)


# ---- 3a. frozen tables -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", FROZEN_TEXTS)
def test_frozen_tables_at_every_placement(ctx, name):
    fq, level, br, cr = text(name)
    control = None
    for lds in (capi.LDS_ROWS_NONE, 64):                                      # k_qlt_encode_c / k_qlt_decode_c without and with rows in LDS
        mode = "frozen tables (%s, lds_rows %s)" % (name, "none" if lds == capi.LDS_ROWS_NONE else lds)
        for place, fill in everywhere():
            what = where("sfq_encode_blocks", mode, place, fill)
            enc = encode_placed(ctx, fq, place, fill, what, level=level, block_reads=br, prior_step=1, tables=FROZEN, chain_reads=cr, lds_rows=lds)
            if control is None:
                assert place == PLACEMENTS[0] == (0, 0)
                control = check_against_oracle(ctx, fq, level, br, cr, 1, what=what, enc=enc)
                if name == "genome":
                    assert util.unpack_chains(enc.chains)["flags"] & 32       # the match model is on
            else:
                same_encoded(enc, control, what)
            decode_placed(ctx, enc, fq, place, fill, where("sfq_decode_blocks", mode, place, fill), level, lds_rows=lds)
    _checked[name, "frozen"] = control


@pytest.mark.gpu
@pytest.mark.parametrize("seg,br,qdiff", SEGMENTS)
def test_long_records_in_segments_at_every_placement(ctx, seg, br, qdiff):
    fq = segment_text(seg, br, qdiff)
    mode = "frozen tables, segments of %d" % seg
    control = None
    for place, fill in everywhere():
        what = where("sfq_encode_blocks", mode, place, fill)
        enc = encode_placed(ctx, fq, place, fill, what, level=3, block_reads=br, prior_step=1, tables=FROZEN, chain_reads=SEG | seg)
        if control is None:                                                   # (as test_long_records_are_cut_into_segments checks it)
            starts, lens = util.line_table(fq)
            nblocks = -(-(len(starts) // 4) // br)
            ci = util.unpack_chains(enc.chains, nblocks)
            assert ci["flags"] & 8 and ci["seg_len"] == seg and ci["chain_reads"] == 1
            qoff, qlen, goff, glen = starts[3::4], lens[3::4], starts[1::4], lens[1::4]
            nseg = O.seg_counts(glen, qlen, seg)
            assert [int(nseg[b * br:(b + 1) * br].sum()) for b in range(nblocks)] == list(ci["seg_blocks"])
            rows66 = O.qlt_prior_rows(O.qlt_histogram(fq, qoff, np.minimum(qlen, PRIOR_SYMBOLS), 3, 0, 1))
            assert np.array_equal(util.unpack_prior(enc.prior, 65536), rows66), what
            want, sizes, extra = O.qlt_encode_segs(fq, qoff, qlen, glen, 3, seg, O.qlt_frozen_rows(rows66))
            assert list(ci["qlt"]) == list(sizes), what
            first_difference(enc.stream("qlt"), want, what + ": stream qlt")
            want, sizes, on = base_chains_oracle(fq, goff, glen, ci, br, 1, seg, qlen)
            assert list(ci["gen"]) == list(sizes), what
            first_difference(enc.stream("gen"), want, what + ": stream gen")
            control = enc
        else:
            same_encoded(enc, control, what)
        decode_placed(ctx, enc, fq, place, fill, where("sfq_decode_blocks", mode, place, fill), 3)


# ---- 3b. adaptive tables: blocks, and format 6 ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_references(name, gen_bits):
    fq, level, br, _ = text(name)
    return [util.block_reference(chunk, level, gen_bits=g).streams for chunk, g in zip(util.split_records(fq, br), gen_bits)]


@functools.lru_cache(maxsize=None)
def format_6_reference(name):
    fq, level, _, _ = text(name)
    ref = O.compress(fq, level)
    return ref.streams, O.decompress(ref.image)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kernel", [(n, 0) for n in SMALL] + [(n, 1) for n in THIN + ["exc"]])
def test_adaptive_blocks_at_every_placement(ctx, name, kernel):
    fq, level, br, _ = text(name)
    mode = "adaptive blocks (%s, kernel %d)" % (name, kernel)
    nblocks = len(util.split_records(fq, br))
    for place, fill in everywhere():
        what = where("sfq_encode_blocks", mode, place, fill)
        enc = encode_placed(ctx, fq, place, fill, what, level=level, block_reads=br, tables=ADAPTIVE, kernel=kernel)
        assert enc.res.n_blocks == nblocks and not enc.chains, what
        want = block_references(name, tuple(b.gen_bits for b in enc.blocks))
        for b in range(nblocks):
            for s in capi.STREAM_NAMES:
                first_difference(enc.stream(s, b), want[b].get(s, b""), "%s: block %d, stream %s" % (what, b, s))
        decode_placed(ctx, enc, fq, place, fill, where("sfq_decode_blocks", mode, place, fill), level, kernel=kernel)
    _checked[name, "adaptive"] = enc


@pytest.mark.gpu
@pytest.mark.parametrize("name,kernel", [(n, 0) for n in FORMAT6_TEXTS] + [(n, 1) for n in THIN])
def test_format_6_at_every_placement(ctx, name, kernel):
    fq, level, _, _ = text(name)
    mode = "format 6 (%s, kernel %d)" % (name, kernel)
    streams, back = format_6_reference(name)
    for place, fill in everywhere():
        what = where("sfq_encode_blocks", mode, place, fill)
        enc = encode_placed(ctx, fq, place, fill, what, level=level, block_reads=0, kernel=kernel)
        assert enc.res.n_blocks == 1, what
        for s in capi.STREAM_NAMES:
            first_difference(enc.stream(s), streams.get(s, b""), "%s: stream %s" % (what, s))
        decode_placed(ctx, enc, back, place, fill, where("sfq_decode_blocks", mode, place, fill), level, kernel=kernel)


# ---- 3c. the quality model alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "last:65", "border:S", "fuzz:1", "exc"])
def test_quality_entry_at_every_placement(ctx, name):
    fq, level, br, _ = text(name)
    mode = "adaptive blocks (%s)" % name
    want = b"".join(util.block_reference(c, level).streams.get("qlt", b"") for c in util.split_records(fq, br))
    q = capi.STREAM_NAMES.index("qlt")
    for place, fill in everywhere():
        what = where("sfq_encode_qlt_blocks", mode, place, fill)
        enc = encode_placed(ctx, fq, place, fill, what, level=level, block_reads=br, tables=ADAPTIVE, qlt_only=True)
        assert enc.res.total_bytes == enc.res.stream_bytes[q], what
        first_difference(enc.stream("qlt"), want, what + ": stream qlt")


# ---- 3d. the priors' entries -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", PRIOR_TEXTS)
def test_priors_entries_at_every_placement(ctx, name):
    fq, level, br, cr = text(name)
    step = 1 if len(fq) < 1000 else 2                                         # the sampling step: every record, every second one
    mode = "frozen tables (%s, prior_step %d)" % (name, step)
    starts, lens = util.line_table(fq)
    nrec = len(starts) // 4
    rows66 = O.qlt_prior_rows(O.qlt_histogram(fq, starts[3::4], np.minimum(lens[3::4], PRIOR_SYMBOLS), level, 0, step))
    hoff, hlen = starts[0::4] + 1, lens[0::4] - 1
    freqs = O.rec_prior_freqs(O.rec_count(fq, hoff, hlen, *rec_sample(nrec, int(hlen.max()))))
    control = None
    for place, fill in everywhere():
        what = where("sfq_build_priors", mode, place, fill)
        src = Placed(len(fq), place[0], fill, fq)
        prior, rec_prior = ctx.build_priors(src.ptr, len(fq), level=level, block_reads=br, prior_step=step, tables=FROZEN)
        first_difference(src.back(what + ": the input"), fq, what + ": the input text")
        assert np.array_equal(util.unpack_prior(prior, 4096 if level == 1 else 65536), rows66), what + ": qlt.pri"
        assert np.array_equal(util.unpack_rec_prior(rec_prior), freqs), what + ": rec.pri"
        # the counts alone, then the call that codes from them -- on the same pointer: it keeps the first call's line index, if the
        # text's fingerprint (k_text_fingerprint) says it is still the text that was framed
        what = where("sfq_count_priors + sfq_encode_blocks(SFQ_PRIOR_COUNTS)", mode, place, fill)
        ctx.count_priors(src.ptr, len(fq), level=level, block_reads=br, prior_step=step, tables=FROZEN, sample_scale=1)
        first_difference(src.back(what + ": the input"), fq, what + ": the input text")
        enc = encode_placed(ctx, fq, place, fill, what, src=src, level=level, block_reads=br, prior_step=capi.PRIOR_COUNTS, tables=FROZEN, chain_reads=cr)
        if control is None:
            control = check_against_oracle(ctx, fq, level, br, cr, step, what=what, enc=enc)
        else:
            same_encoded(enc, control, what)
    ctx.set_priors(b"", b"")


# ---- 3e. a window of the blocks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,tables", (("genome", "frozen"), ("exc", "frozen"), ("exc", "adaptive")))
def test_block_windows_at_every_placement(ctx, name, tables):
    fq, level, br, cr = text(name)
    enc = _checked.get((name, tables))
    if enc is None:                                                           # (run alone: the aligned call, checked here)
        if tables == "frozen":
            enc = check_against_oracle(ctx, fq, level, br, cr, 1, what=name)
        else:
            enc = ctx.encode_host(fq, level=level, block_reads=br, tables=ADAPTIVE)
            want = block_references(name, tuple(b.gen_bits for b in enc.blocks))
            for b in range(len(enc.blocks)):
                for s in capi.STREAM_NAMES:
                    first_difference(enc.stream(s, b), want[b].get(s, b""), "%s: block %d, stream %s" % (name, b, s))
    if name == "genome":                                                      # the one decoder that reads outside its window
        assert util.unpack_chains(enc.chains)["flags"] & 32
    nb = len(enc.blocks)
    assert nb >= 4
    mode = "%s tables (%s)" % (tables, name)
    for window in ((nb // 2 - 1, 2), (nb - 1, 1)):                            # one in the middle, and the last
        want = window_records(fq, br, *window)
        assert want and (window[0] + window[1] == nb) == fq.endswith(want)
        for place, fill in everywhere():
            decode_placed(ctx, enc, want, place, fill, where("sfq_decode_block_range", mode + ", blocks %d+%d" % window, place, fill), level, window=window)

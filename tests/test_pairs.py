"""Paired files on the GPU (pair.hip): sfq_interleave and sfq_split_pairs against three lines of Python over
fq.split(b"\\n"), on texts whose record starts fall on every border of the kernels, in buffers at every alignment and between guard
bytes; the refusals; sfq_encode_pairs_host against sfq_encode_blocks_host of the text interleaved in Python; the decode switch.
Every comparison is exact byte equality."""
import zlib

import numpy as np
import pytest

import util
from slimfastq_amd import capi
from test_text_stats import ref_stats, diff

pytestmark = pytest.mark.gpu
# pair.hip: a lane takes one aligned UNIT of the OUTPUT (of the texts in the counting passes), a wavefront a ROW of them at a time and a
# SPAN in all, a workgroup four spans (WG_TILE); a wavefront keeps the destinations of WINDOW pieces, one per lane; spans are laid
# from the aligned unit that holds the first byte.  SCAN_BLOCK: the entries one block of launch_scan_u32 takes.
UNIT, ROW, SPAN, WG_TILE, WINDOW, SCAN_BLOCK = 16, 1024, 16 << 10, 64 << 10, 64, 1024
GUARD = 64
E_ARG, E_FORMAT, E_OVERFLOW, E_CORRUPT, E_UNSUPPORTED = -1, -4, -5, -6, -7


# ---- the references ------------------------------------------------------------------------------------------------------------

def records(fq: bytes):
    """Records are groups of four lines; a text without a final '\\n' ends in a line all the same."""
    lines = fq.split(b"\n")
    lines = [l + b"\n" for l in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    assert len(lines) % 4 == 0
    return [b"".join(lines[i:i + 4]) for i in range(0, len(lines), 4)]


def interleaved(a: bytes, b: bytes) -> bytes:
    return b"".join(x + y for x, y in zip(records(a), records(b)))


def split(fq: bytes) -> bytes:
    r = records(fq)
    return b"".join(r[0::2]) + b"".join(r[1::2])


# ---- device buffers between guards -----------------------------------------------------------------------------------------------

class Buf:
    """n bytes on the device that start off bytes behind a 16-byte boundary, GUARD bytes of 'I' on either side."""

    def __init__(self, n, off=0, data=None):
        import torch
        self.t = torch.full((n + 2 * GUARD + 32,), ord("I"), dtype=torch.uint8, device="cuda")
        self.base = (-self.t.data_ptr()) % 16 + GUARD + off
        self.n = n
        self.ptr = self.t.data_ptr() + self.base
        assert self.ptr % 16 == off
        if data is not None:
            self.t[self.base:self.base + n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()

    def back(self, what):
        """the n bytes; the guards must come back untouched"""
        raw = self.t.cpu().numpy().tobytes()
        assert raw[:self.base] == b"I" * self.base and raw[self.base + self.n:] == b"I" * (len(raw) - self.base - self.n), \
            "a guard byte of %s was written" % what
        return raw[self.base:self.base + self.n]


def first_difference(got, want, what):
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        bad = np.flatnonzero(a != b)
        raise AssertionError("%s: %d bytes differ, the first at %d of %d" % (what, len(bad), bad[0], len(want)))


def check(ctx, a, b, offs=(0, 0, 0), what=""):
    """sfq_interleave of a and b, then sfq_split_pairs of its output, each against the reference; offs: the device offsets of a, b
    and both outputs."""
    want = interleaved(a, b)
    pairs = len(records(a))
    A, B, out = Buf(len(a), offs[0], a), Buf(len(b), offs[1], b), Buf(len(a) + len(b), offs[2])
    n, p = ctx.interleave(A.ptr, len(a), B.ptr, len(b), out.ptr, out.n)
    got = out.back("the interleaved output")
    assert (A.back("A"), B.back("B")) == (a, b)
    assert (n, p) == (len(a) + len(b), pairs), what
    first_difference(got, want, what + " interleave, offsets %s" % (offs,))
    # and back: the round trip
    T, out2 = Buf(len(want), offs[0], want), Buf(len(want), offs[2])
    at, p = ctx.split_pairs(T.ptr, len(want), out2.ptr, out2.n)
    got = out2.back("the split output")
    assert T.back("the text") == want
    assert (at, p) == (len(a), pairs), what
    first_difference(got, a + b, what + " split, offsets %s" % (offs,))
    assert a + b == split(want)
    return want


def record(rng, length, hdr=None):
    return b"".join([hdr if hdr is not None else b"@r%d" % int(rng.integers(0, 10 ** int(rng.integers(1, 9)))), b"\n",
                     np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, length)].tobytes(), b"\n+\n",
                     rng.integers(ord("!"), ord("~") + 1, length, dtype=np.uint8).tobytes(), b"\n"])


def reads(n, lo, hi, seed):
    """n records of lo .. hi bases"""
    rng = np.random.default_rng(seed)
    return b"".join(record(rng, int(rng.integers(lo, hi + 1))) for _ in range(n))


def starts_of(fq):
    return np.cumsum([0] + [len(r) for r in records(fq)])[:-1]


def longer_first_header(fq, by):
    return fq[:1] + b"h" * by + fq[1:]


# ---- 1, 2: the smallest texts, the pair counts -------------------------------------------------------------------------------------

def test_smallest_texts(ctx):
    r = b"@\nA\n+\nI\n"
    assert len(r) < UNIT
    check(ctx, r, r.replace(b"A", b"C"), what="one pair of eight bytes")
    e = b"@h\n\n+\n\n"
    check(ctx, e, e, what="empty lines")
    check(ctx, e * 70 + r * 3, r * 70 + e * 3, what="empty lines, more pieces than a window in a row")
    assert len(e) * WINDOW < ROW


@pytest.mark.parametrize("pairs", (1, 2, 3, 4, WINDOW - 1, WINDOW, WINDOW + 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1))
def test_pair_counts(ctx, pairs):
    check(ctx, reads(pairs, 1, 40, seed=pairs), reads(pairs, 1, 40, seed=1000 + pairs), what="%d pairs" % pairs)


# ---- 3: alignment --------------------------------------------------------------------------------------------------------------

def test_alignment(ctx):
    a, b = reads(14, 90, 110, seed=3), reads(14, 90, 110, seed=4)
    assert 2500 < len(a) < 3600
    for off in range(UNIT):
        check(ctx, a, b, (off, 0, 0), "A's offset")
        check(ctx, a, b, (0, off, 0), "B's offset")
        check(ctx, a, b, (0, 0, off), "the output's offset")
    grown = {len(longer_first_header(a, k)) % UNIT for k in range(UNIT)}
    assert grown == set(range(UNIT))
    for k in range(UNIT):
        check(ctx, longer_first_header(a, k), b, (0, 0, 0), "na % 16")


# ---- 4: borders ----------------------------------------------------------------------------------------------------------------

BORDERS = [20 * UNIT, ROW, SPAN, WG_TILE]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("where", ("A", "B", "out"))
def test_a_record_start_on_and_around_every_border(ctx, where, border):
    a, b = reads(400, 80, 120, seed=border), reads(400, 80, 120, seed=border + 1)
    assert min(len(a), len(b)) > WG_TILE + SPAN
    for d in (-1, 0, 1):
        target = border + d
        s = starts_of({"A": a, "B": b, "out": interleaved(a, b)}[where])
        s = int(s[(s <= target) & (s > 0)].max())                     # an early record start: the first header grows until it is there
        a2, b2 = (a, longer_first_header(b, target - s)) if where == "B" else (longer_first_header(a, target - s), b)
        assert target in starts_of({"A": a2, "B": b2, "out": interleaved(a2, b2)}[where])
        check(ctx, a2, b2, what="a record start of %s at %d" % (where, target))


# ---- 5: skew -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ("A", "B", "first", "last"))
def test_one_long_record_among_short_ones(ctx, where):
    rng = np.random.default_rng(5)
    n = 300
    long = record(rng, 200000)
    assert len(long) > 2 * WG_TILE
    a, b = [record(rng, 100) for _ in range(n)], [record(rng, 100) for _ in range(n)]
    if where == "A": a[n // 2] = long
    if where == "B": b[n // 3] = long
    if where == "first": a[0] = long
    if where == "last": b[n - 1] = long
    check(ctx, b"".join(a), b"".join(b), what="a long record: " + where)


def test_short_mates_against_long_mates(ctx):
    check(ctx, reads(500, 36, 36, seed=6), reads(500, 251, 251, seed=7), what="36 against 251 bases")


# ---- 6: more span counts than one block of the scan ------------------------------------------------------------------------------------

def test_more_spans_than_a_scan_block(ctx):
    a, b = capi.synth_fastq(56000, 150, seed=8), capi.synth_fastq(56000, 150, seed=9)
    assert min(len(a), len(b)) > SCAN_BLOCK * SPAN
    check(ctx, a, b, (3, 9, 5), "2 x 17 MB")


# ---- 7: B without its final line end ---------------------------------------------------------------------------------------------

def test_b_without_the_final_line_end(ctx):
    a, b = reads(100, 50, 150, seed=10), reads(100, 50, 150, seed=11)[:-1]
    want = check(ctx, a, b, what="B without the final line end")
    assert len(want) == len(a) + len(b) and want[-1:] != b"\n"
    r = b"@\nA\n+\nI\n"
    check(ctx, r, r[:-1], what="one pair, B without the final line end")


# ---- 9: refusals -----------------------------------------------------------------------------------------------------------------

def refused(ctx, code, a, b=None, cap=None, needs=None):
    """the call fails with `code` and leaves its output as it was"""
    n = len(a) + (len(b) if b is not None else 0)
    A, out = Buf(max(len(a), 1), 0, a if a else None), Buf(max(n, 1), 5)
    B = Buf(max(len(b), 1), 0, b if b else None) if b is not None else None
    with pytest.raises(capi.SfqError) as e:
        if b is not None:
            ctx.interleave(A.ptr, len(a), B.ptr, len(b), out.ptr, n if cap is None else cap)
        else:
            ctx.split_pairs(A.ptr, len(a), out.ptr, n if cap is None else cap)
    assert e.value.code == code, str(e.value)
    assert out.back("the output of a refused call") == b"I" * out.n, "a refused call wrote to its output"
    if needs is not None:
        assert e.value.needed == needs
    return str(e.value)


def test_refusals(ctx):
    a, b = reads(20, 30, 60, seed=12), reads(21, 30, 60, seed=13)
    msg = refused(ctx, E_FORMAT, a, b)
    assert "20" in msg and "21" in msg                                  # both counts
    b = reads(20, 30, 60, seed=13)
    refused(ctx, E_FORMAT, a + b"extra\n", b)                           # five lines at the end of a text
    refused(ctx, E_FORMAT, a, b + b"extra\n")
    refused(ctx, E_FORMAT, b"@h\nA\n+\nI\nx\n", b"@h\nA\n+\nI\n")
    refused(ctx, E_FORMAT, reads(21, 30, 60, seed=14))                  # an odd record count to split
    refused(ctx, E_FORMAT, a + b"extra\n")
    refused(ctx, E_FORMAT, a[:-1], b)                                   # A without its final line end
    refused(ctx, E_ARG, b"", b)
    refused(ctx, E_ARG, a, b"")
    refused(ctx, E_ARG, b"")
    refused(ctx, E_OVERFLOW, a, b, cap=len(a) + len(b) - 1, needs=len(a) + len(b))
    refused(ctx, E_OVERFLOW, a + b, cap=len(a) + len(b) - 1)
    check(ctx, a, b, what="after the refusals")


# ---- 10 - 12: the host entries ---------------------------------------------------------------------------------------------------

def mates(n, length, seed):
    """n pairs whose headers differ in ' 1:N:0:' against ' 2:N:0:' alone"""
    rng = np.random.default_rng(seed)
    a, b = [], []
    x = rng.integers(1000, 30000, n); y = rng.integers(1000, 30000, n)
    for i in range(n):
        h = b"@M7:42:000000000-A7XYZ:1:%d:%d:%d " % (1101 + i * 8 // n, int(x[i]), int(y[i]))
        for out, tag in ((a, b"1:N:0:ATCACG"), (b, b"2:N:0:ATCACG")):
            out.append(h + tag + b"\n" + np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)].tobytes() + b"\n+\n" +
                       rng.integers(ord("#"), ord("J") + 1, length, dtype=np.uint8).tobytes() + b"\n")
    return b"".join(a), b"".join(b)


ILLUMINA8 = capi.quality_map_preset("illumina8")


def numpy_mapped(fq: bytes, lut: bytes) -> bytes:
    """every 4th line through the table"""
    t = np.frombuffer(lut, np.uint8)
    lines = fq.split(b"\n")
    lines[3::4] = [t[np.frombuffer(l, np.uint8)].tobytes() for l in lines[3::4]]
    return b"\n".join(lines)


def same_archive(a, b):
    return (bytes(a.data) == bytes(b.data) and bytes(a.blocks) == bytes(b.blocks) and
            (a.first_hdrs, a.prior, a.chains, a.rec_prior) == (b.first_hdrs, b.prior, b.chains, b.rec_prior) and
            list(a.res.stream_bytes) == list(b.res.stream_bytes) and list(a.res.stream_offset) == list(b.res.stream_offset))


CASES = {
    "adaptive": (2000, dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO)),
    "frozen": (20000, dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN)),
}
_texts = {}


def texts(case):
    """(A, B, the interleaved text), computed once"""
    if case not in _texts:
        a, b = mates(CASES[case][0], 100, seed=len(case))
        _texts[case] = (a, b, interleaved(a, b))
    return _texts[case]


@pytest.fixture
def pctx(ctx):
    """The session's context; afterwards no split, no map, checksums and statistics off."""
    try:
        yield ctx
    finally:
        ctx.set_pair_split(False)
        ctx.set_quality_map(None)
        ctx.set_checksums(False)
        ctx.set_stats(False)


@pytest.mark.parametrize("case", sorted(CASES))
def test_encode_pairs_host_codes_the_interleaved_text(pctx, case):
    ctx = pctx
    a, b, both = texts(case)
    kw = CASES[case][1]
    want = ctx.encode_host(both, **kw)
    got = ctx.encode_pairs_host(a, b, **kw)
    assert same_archive(got, want)                                    # streams, block index, first headers, priors, chain index
    if case == "frozen":
        assert len(want.chains) > 0 and len(want.rec_prior) > 0
    # the decode switch
    cap = len(both) + 4096
    assert ctx.decode_host(got, level=3, out_cap=cap) == both and ctx.pair_split() is None
    ctx.set_pair_split(True)
    assert ctx.decode_host(got, level=3, out_cap=cap) == a + b
    assert ctx.pair_split() == (len(a), CASES[case][0])
    ctx.set_pair_split(False)
    assert ctx.decode_host(got, level=3, out_cap=cap) == both and ctx.pair_split() is None


def test_encode_pairs_host_with_a_quality_map_statistics_and_checksums(pctx):
    ctx = pctx
    a, b, both = texts("adaptive")
    kw = CASES["adaptive"][1]
    mapped = numpy_mapped(both, ILLUMINA8)
    assert mapped != both
    plain = ctx.encode_host(mapped, **kw)
    ctx.set_quality_map(ILLUMINA8)
    assert same_archive(ctx.encode_pairs_host(a, b, **kw), plain)
    ctx.set_quality_map(None)
    ctx.set_checksums(True); ctx.set_stats(True)
    enc = ctx.encode_pairs_host(a, b, **kw)
    assert enc.text_crc == zlib.crc32(both)
    bounds = [int(x.first_record) for x in enc.blocks]
    recs = util.split_records(both, 1)
    assert enc.crcs == [zlib.crc32(b"".join(recs[i:j])) for i, j in zip(bounds, bounds[1:] + [len(recs)])]
    want = ref_stats(both)
    assert enc.stats == want, diff(enc.stats, want)
    # the switch with block checksums installed (decode_host installs enc.crcs): passes, and fails on a flipped one
    ctx.set_checksums(False)
    ctx.set_pair_split(True)
    cap = len(both) + 4096
    assert ctx.decode_host(enc, level=3, out_cap=cap) == a + b and ctx.pair_split() == (len(a), len(recs) // 2)
    bad = enc.clone()
    bad.crcs = list(enc.crcs)
    bad.crcs[1] ^= 1
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(bad, level=3, out_cap=cap)
    assert e.value.code == E_CORRUPT and ctx.pair_split() is None
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_range_host(enc, 1, 2, level=3, out_cap=cap)
    assert e.value.code == E_UNSUPPORTED
    ctx.set_pair_split(False)
    text, _ = ctx.decode_range_host(enc, 1, 2, level=3, out_cap=cap)
    assert text == b"".join(recs[bounds[1]:bounds[3]])


def test_it_pays(pctx):
    """20 000 pairs of 100 bases whose headers differ in ' 1:N:0:' against ' 2:N:0:', adaptive tables, one block: the rec stream of
    the pairs call against the sum of two separate calls.  The oracle measured 0.565 on this construction; the
    margin up to 0.75 is for the generator's seed."""
    ctx = pctx
    a, b = mates(20000, 100, seed=12)
    kw = dict(level=3, block_reads=0)
    rec = capi.STREAM_NAMES.index("rec")
    apart = sum(int(ctx.encode_host(t, **kw).res.stream_bytes[rec]) for t in (a, b))
    pairs = ctx.encode_pairs_host(a, b, **kw)
    assert pairs.res.n_blocks == 1
    together = int(pairs.res.stream_bytes[rec])
    print("rec stream: %d bytes apart, %d bytes as pairs, %.3f" % (apart, together, together / apart))
    assert together <= 0.75 * apart

"""Picked lines on the GPU (pick.hip): sfq_pick_lines against a few lines of Python over the records of the text --
FASTA, the names, the base lines, the quality lines -- on texts whose pieces are one byte, longer than a workgroup's tile and
everything between, in buffers at every alignment and between guard bytes; ranges of records; the refusals; the decode switch
(sfq_ctx_set_pick) behind every decoder, with checksums and with the pair split.  Every comparison is exact byte equality.

What holds for the bytes behind the result (slimfastq_amd.h): a call that succeeds writes d_out[0, *out_bytes) and nothing else,
inside out_cap too; a refused call writes nothing at all.  Every check below fills the output with a marker first and asserts that."""
import numpy as np
import pytest

from slimfastq_amd import capi
from test_pairs import Buf, E_ARG, E_CORRUPT, E_FORMAT, E_OVERFLOW, first_difference, reads, record, records

pytestmark = pytest.mark.gpu
UNIT, ROW, SPAN, WG_TILE, WINDOW, SCAN_BLOCK = 16, 1024, 16 << 10, 64 << 10, 64, 1024
FASTA, NAMES, BASES, QUALS = capi.PICK_FASTA, capi.PICK_NAMES, capi.PICK_BASES, capi.PICK_QUALS
ALL = (FASTA, NAMES, BASES, QUALS)
NAME = {FASTA: "fasta", NAMES: "names", BASES: "bases", QUALS: "quals"}


def picked(fq, what, r0=0, nr=None):
    out = []
    for r in records(fq)[r0:None if nr is None else r0 + nr]:
        l = r.split(b"\n"); l = [x + b"\n" for x in l[:-1]] + ([l[-1]] if l[-1] else [])   # four lines, the last maybe without '\n'
        out.append({1: b">" + l[0][1:] + l[1], 2: l[0][1:], 3: l[1], 4: l[3]}[what])
    return b"".join(out)


def check(ctx, fq, what, offs=(0, 0), r0=0, nr=None, msg="", slack=37):
    """sfq_pick_lines of fq against picked(); offs: the device offsets of the text and the output.  The output holds `slack` bytes
    more than the result: they and the guards come back as they were."""
    want = picked(fq, what, r0, nr)
    T, out = Buf(len(fq), offs[0], fq), Buf(len(want) + slack, offs[1])
    n, recs = ctx.pick_lines(T.ptr, len(fq), what, out.ptr, out.n, r0, nr)
    got = out.back("the picked output")
    assert T.back("the text") == fq, "the text was written"
    label = "%s %s, offsets %s, records %s..+%s" % (msg, NAME[what], offs, r0, nr)
    assert n == len(want), label
    assert recs == len(records(fq)[r0:None if nr is None else r0 + nr]), label
    first_difference(got[:n], want, label)
    assert got[n:] == b"I" * slack, label + ": bytes behind the result were written"
    return want


# ---- 1: the smallest texts ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ALL, ids=NAME.get)
def test_smallest_texts(ctx, what):
    for fq in (b"@\nA\n+\nI\n", b"@h\n\n+\n\n", b"@\nA\n+\nI"):
        check(ctx, fq, what, msg=repr(fq))
    # b"@h\n\n+\n\n" without its final '\n' is three line ends with no byte behind them: three lines (a last line that exists has a
    # byte), for which records() has no answer either -- refused
    refused(ctx, E_FORMAT, b"@h\n\n+\n", what)


# ---- 2: every border of the copy ------------------------------------------------------------------------------------------------------

_texts = {}


def text(name):
    if name not in _texts:
        _texts[name] = {"mixed": lambda: reads(700, 1, 70, 2), "short": lambda: reads(2100, 1, 8, 3)}[name]()
    return _texts[name]


@pytest.mark.parametrize("what", ALL, ids=NAME.get)
def test_every_border_of_the_copy(ctx, what):
    fq = text("mixed")
    for w in (FASTA, BASES):                                          # piece starts at every offset mod 16, source and destination
        rs = records(fq)
        src = np.cumsum([0] + [len(r) for r in rs])[:-1]
        dst = np.cumsum([0] + [len(picked(r, w)) for r in rs])[:-1]
        assert set(src % UNIT) == set(range(UNIT)) and set(dst % UNIT) == set(range(UNIT))
    check(ctx, fq, what, msg="700 records of 1..70 bases")
    fq = text("short")
    assert len(records(fq)) > 2 * SCAN_BLOCK and len(picked(fq, FASTA)) / 2100 * WINDOW < ROW     # the pieces of a window in less than a row
    check(ctx, fq, what, msg="2100 records of 1..8 bases")


# ---- 3: long pieces -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ("middle", "first", "last"))
def test_long_pieces(ctx, where):
    rng = np.random.default_rng(5)
    long = record(rng, 70000)
    assert len(long) > 2 * WG_TILE and 70000 > WG_TILE > SPAN
    rs = [record(rng, int(rng.integers(1, 4))) for _ in range(40)]
    rs[{"middle": 17, "first": 0, "last": 39}[where]] = long
    for what in ALL:
        check(ctx, b"".join(rs), what, offs=(3, 9), msg="a long record " + where)


# ---- 4, 5: pieces of one byte ------------------------------------------------------------------------------------------------------------

def empties(n, first=0):
    return b"".join(b"@r%d\n\n+\n\n" % i for i in range(first, first + n))


def test_one_byte_pieces(ctx):
    fq = empties(300)
    for what in (BASES, QUALS):
        assert check(ctx, fq, what, msg="300 empty records") == b"\n" * 300      # 64 pieces in 64 bytes, sixteen in a unit
        for off in (1, 15):
            check(ctx, fq, what, offs=(0, off), msg="300 empty records")
    rng = np.random.default_rng(6)
    fq = empties(100) + record(rng, 40000) + empties(100, 100)
    for what in ALL:
        check(ctx, fq, what, msg="100 empty records, 40 000 bases, 100 empty records")
    fq = b"".join(b"@\n" + b"ACGT"[:i % 4 + 1] + b"\n+\n" + b"IIII"[:i % 4 + 1] + b"\n" for i in range(300))
    assert check(ctx, fq, NAMES, msg="300 headers of one byte") == b"\n" * 300
    check(ctx, fq, FASTA, msg="300 headers of one byte")


def test_one_byte_pieces_across_a_span_border(ctx):
    fq = empties(17500)
    assert len(fq) < 1 << 20
    assert len(check(ctx, fq, BASES, msg="17 500 empty base lines")) > SPAN + 64 * UNIT
    check(ctx, fq, QUALS, offs=(5, 11), msg="17 500 empty quality lines")


# ---- 6: placement -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ALL, ids=NAME.get)
def test_placement(ctx, what):
    fq = text("mixed")
    for i in (0, 1, 7, 15):
        for o in (0, 1, 7, 15):
            check(ctx, fq, what, offs=(i, o))


# ---- 7: ranges --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ALL, ids=NAME.get)
def test_ranges(ctx, what):
    fq = text("mixed")
    n = len(records(fq))
    whole = check(ctx, fq, what)
    assert check(ctx, fq, what, r0=0, nr=n) == whole
    for r0, nr in ((1, 1), (2, 1), (n - 1, 1), (n - 1, None), (333, 200), (350, None), (201, 64), (0, 1)):
        check(ctx, fq, what, r0=r0, nr=nr, offs=(r0 % 16, (nr or 0) % 16))
    cut = fq[:-1]                                                     # without the final '\n': the last record in and out of the range
    assert cut[-1:] != b"\n"
    assert check(ctx, cut, what)[-1:] == (b"\n" if what != QUALS else cut[-1:])
    check(ctx, cut, what, r0=n - 3, nr=3)
    check(ctx, cut, what, r0=n - 3, nr=None)
    check(ctx, cut, what, r0=n - 3, nr=2)
    check(ctx, cut, what, r0=n - 1, nr=1)


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------------------

def refused(ctx, code, fq, what, r0=0, nr=None, cap=None, needs=None):
    """the call fails with `code` and leaves its output, marker-filled, and the guards as they were"""
    T, out = Buf(max(len(fq), 1), 3, fq if fq else None), Buf(max(len(fq), 1) + 16, 5)
    with pytest.raises(capi.SfqError) as e:
        ctx.pick_lines(T.ptr, len(fq), what, out.ptr, out.n if cap is None else cap, r0, nr)
    assert e.value.code == code, str(e.value)
    assert out.back("the output of a refused call") == b"I" * out.n, "a refused call wrote to its output"
    if fq:
        assert T.back("the text") == fq
    if needs is not None:
        assert e.value.needed == needs
    return str(e.value)


def test_refusals(ctx):
    fq = reads(200, 20, 40, seed=8)
    n = len(records(fq))
    for what in ALL:
        refused(ctx, E_FORMAT, fq + b"extra\n", what)                 # lines % 4 != 0
        refused(ctx, E_ARG, b"", what)
        refused(ctx, E_ARG, fq, what, nr=0)
        refused(ctx, E_ARG, fq, what, r0=n - 9, nr=10)                # one past the end
        refused(ctx, E_ARG, fq, what, r0=n, nr=None)
        want = picked(fq, what)
        refused(ctx, E_OVERFLOW, fq, what, cap=len(want) - 1, needs=len(want))
        T, out = Buf(len(fq), 0, fq), Buf(len(want), 0)               # ... and with exactly that size it succeeds
        assert ctx.pick_lines(T.ptr, len(fq), what, out.ptr, len(want)) == (len(want), n)
        assert out.back("an output of exactly the size needed") == want
    refused(ctx, E_ARG, fq, 0)
    refused(ctx, E_ARG, fq, 5)
    # records 130 and 5, in different wavefronts, begin with '>'
    rs = records(fq)
    for i in (130, 5):
        rs[i] = b">" + rs[i][1:]
    bad = b"".join(rs)
    at = sum(len(r) for r in rs[:5])
    for what in (FASTA, NAMES):
        msg = refused(ctx, E_FORMAT, bad, what)
        assert "record 5 " in msg and "byte %d)" % at in msg, msg
        msg = refused(ctx, E_FORMAT, bad, what, r0=6, nr=None)
        assert "record 130 " in msg, msg
    check(ctx, bad, BASES, msg="'>' records")
    check(ctx, bad, QUALS, msg="'>' records")
    check(ctx, bad, FASTA, r0=6, nr=124, msg="a range between the '>' records")
    check(ctx, bad, NAMES, r0=131, nr=None, msg="a range behind the '>' records")
    check(ctx, fq, FASTA, msg="after the refusals")


# ---- 9: through the decoders --------------------------------------------------------------------------------------------------------------

DECODERS = {
    "adaptive": (lambda: capi.synth_fastq(3000, 150, seed=31), dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO)),
    "frozen": (lambda: capi.synth_fastq(3000, 150, seed=31), dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN)),
    "long_adaptive": (lambda: capi.synth_fastq(8, 150, seed=5, kind=1), dict(level=3, block_reads=2, tables=capi.TABLES_ADAPTIVE)),
    "long_frozen": (lambda: capi.synth_fastq(8, 150, seed=5, kind=1), dict(level=3, block_reads=2, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN)),
}


@pytest.fixture
def pctx(ctx):
    """The session's context; afterwards no pick, no split, checksums off."""
    try:
        yield ctx
    finally:
        ctx.set_pick(0)
        ctx.set_pair_split(False)
        ctx.set_checksums(False)


@pytest.mark.parametrize("case", sorted(DECODERS))
def test_through_the_decoders(pctx, case):
    ctx = pctx
    fq = DECODERS[case][0]()
    rs = records(fq)
    ctx.set_checksums(True)                                           # decode_host installs the blocks' CRCs: those of the full text
    enc = ctx.encode_host(fq, **DECODERS[case][1])
    ctx.set_checksums(False)
    nb = len(enc.blocks)
    assert nb >= 4 and len(enc.crcs) == nb
    cap = len(fq) + 4096
    bounds = [int(b.first_record) for b in enc.blocks] + [len(rs)]
    b0, bn = nb // 3, max(1, nb // 3)
    window = b"".join(rs[bounds[b0]:bounds[b0 + bn]])
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_pick() is None
    for w in ALL:
        ctx.set_pick(w)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(fq, w), "%s, the whole call, %s" % (case, NAME[w]))
        assert ctx.get_pick() == (w, len(fq), len(rs))
        got, res = ctx.decode_range_host(enc, b0, bn, level=3, out_cap=cap)
        first_difference(got, picked(window, w), "%s, blocks %d..+%d, %s" % (case, b0, bn, NAME[w]))
        assert ctx.get_pick() == (w, len(window), len(records(window)))
    bad = enc.clone()
    bad.crcs = list(enc.crcs)
    bad.crcs[1] ^= 1
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(bad, level=3, out_cap=cap)
    assert e.value.code == E_CORRUPT and ctx.get_pick() is None
    with pytest.raises(capi.SfqError) as e:
        ctx.set_pick(5)
    assert e.value.code == E_ARG
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(fq, QUALS), "the setting stays")
    ctx.set_pick(0)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_pick() is None


# ---- 10: with pairs -------------------------------------------------------------------------------------------------------------------------

def test_with_pairs(pctx):
    ctx = pctx
    a, b = reads(1500, 30, 60, seed=21), reads(1500, 30, 60, seed=22)
    ra, rb = records(a), records(b)
    ctx.set_checksums(True)
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=7, tables=capi.TABLES_ADAPTIVE)
    ctx.set_checksums(False)
    cap = len(a) + len(b) + 4096
    for w in ALL:
        ctx.set_pair_split(True)
        ctx.set_pick(w)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(a, w) + picked(b, w), "the split, " + NAME[w])
        assert ctx.pair_split() == (len(picked(a, w)), 1500)
        assert ctx.get_pick() == (w, len(a) + len(b), 3000)
        ctx.set_pair_split(False)
        wa, wb = b"".join(ra[700:900]), b"".join(rb[700:900])
        first, second, _ = ctx.decode_pair_range_host(enc, 700, 200, out_cap=cap)      # (cuts at *split)
        first_difference(first, picked(wa, w), "pairs 700..+200, first mates, " + NAME[w])
        first_difference(second, picked(wb, w), "pairs 700..+200, second mates, " + NAME[w])
        assert ctx.pair_split() == (len(picked(wa, w)), 200)
        assert ctx.get_pick() == (w, len(wa) + len(wb), 400)
    ctx.set_pick(0)
    first, second, _ = ctx.decode_pair_range_host(enc, 700, 200, out_cap=cap)
    assert (first, second) == (b"".join(ra[700:900]), b"".join(rb[700:900])) and ctx.get_pick() is None

"""Demultiplexed records on the GPU (dmx.hip, slimfastq_amd.h "demultiplexed records"): sfq_demux_records against the restatement of
the header's rule in demux_rule.py, built independently of the C code.  Every comparison is exact: the bytes, the parts' offsets,
the units per sample, every counter of the report.  Every output is filled with a marker: a call writes its result and nothing
behind it, a refused call nothing at all; the text is never written."""
import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Demux, DemuxPart, DEMUX_HEADER as H, DEMUX_BASES as B
from demux_rule import TO_END, Refused, demux, records, text_of
from test_pairs import Buf, first_difference

pytestmark = pytest.mark.gpu
E_ARG, E_FORMAT, E_OVERFLOW, E_UNSUPPORTED = -1, -4, -5, -7
ACGT = np.frombuffer(b"ACGT", np.uint8)
TILE = 1024                                                            # the sort's tile (kernels.h DMX_TILE): a power of two below 4097


def bases(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def rec(hdr, b, quals=None, plus=b"+"):
    return hdr + b"\n" + b + b"\n" + plus + b"\n" + (b"I" * len(b) if quals is None else quals) + b"\n"


def rows_of(n, length, seed=0):
    """n distinct barcodes of the given length: the numbers 0 .. n - 1 permuted, two bits a base"""
    assert n <= 4 ** min(length, 12)
    rng = np.random.default_rng(1000 + seed)
    ids = rng.permutation(4 ** min(length, 12))[:n] if length <= 12 else rng.choice(4 ** 12, n, replace=False)
    tail = bases(rng, length)
    return [bytes(b"ACGT"[(int(v) >> (2 * i)) & 3] for i in range(min(length, 12))) + tail[12:] for v in ids]


def spoil(rng, code, p_exact=0.5, alphabet=b"ACGTN.acgt"):
    """a barcode as a read carries it: as it is, or with one or two bytes changed -- to another base, an N, a '.', or lower case"""
    if rng.random() < p_exact:
        return code
    c = bytearray(code)
    for _ in range(int(rng.integers(1, 3))):
        i = int(rng.integers(0, len(c)))
        c[i] = alphabet[int(rng.integers(0, len(alphabet)))]
    return bytes(c)


def lane(rng, units, rows, l0, where="hdr", pairs=False, junk=0.2, lens=(20, 60), alphabet=b"ACGTN.acgt"):
    """a text of units whose barcodes are spoiled rows (or junk): where = 'hdr' (index field), 'inline' (the read's first bases),
    'inline2' (part 0 in mate 0's bases, part 1 in mate 1's); records of unequal lengths; alphabet: what a spoiled byte becomes"""
    out = []
    Bn = len(rows[0])
    for u in range(units):
        code = bases(rng, Bn) if rng.random() < junk else spoil(rng, rows[int(rng.integers(0, len(rows)))], alphabet=alphabet)
        c0, c1 = code[:l0], code[l0:]
        for g in range(2 if pairs else 1):
            L = int(rng.integers(lens[0], lens[1]))
            b = bases(rng, L)
            if where == "hdr":
                field = c0 + (b"+" + c1 if c1 else b"")
            else:
                field = b"0"
                if where == "inline" and g == 0:
                    b = code + b
                if where == "inline2":
                    b = (c0 if g == 0 else c1) + b
            q = rng.integers(33, 74, len(b), dtype=np.uint8).tobytes()
            out.append(rec(b"@r%d/%d %d:N:0:" % (u, g + 1, g + 1) + field, b, q))
    return b"".join(out)


def hdr_parts(l0, l1=0):
    return [DemuxPart(H, 0, 0, 0, l0)] + ([DemuxPart(H, 0, 1, 0, l1)] if l1 else [])


def check(ctx, fq, rule, rows, offs=(0, 0), msg="", slack=37):
    """sfq_demux_records against the rule; returns (parts, units, counts) of the rule"""
    parts, units, c = demux(fq, rule, rows)
    want = b"".join(parts)
    T, out = Buf(len(fq), offs[0], fq), Buf(len(want) + slack, offs[1])
    n, off, got_units, rep = ctx.demux_records(T.ptr, len(fq), rule, rows, out.ptr, out.n)
    got = out.back("the output")
    assert T.back("the text") == fq, "the text was written"
    what = "%s, %d samples, offsets %s" % (msg, rule.n_samples, offs)
    assert n == len(want), (what, n, len(want))
    first_difference(got[:n], want, what)
    assert got[n:] == b"I" * (out.n - n), what + ": bytes behind the result were written"
    assert off == list(np.concatenate([[0], np.cumsum([len(p) for p in parts])])), what
    assert got_units == units, what
    assert (rep.n_in_range, rep.n_units, rep.n_assigned, rep.n_perfect, rep.n_short, rep.n_far, rep.n_ambiguous, rep.text_bytes, rep.out_bytes,
            rep.bases_clipped) == (c["n_in_range"], c["n_units"], c["n_assigned"], c["n_perfect"], c["n_short"], c["n_far"], c["n_ambiguous"],
                                   len(fq), len(want), c["bases_clipped"]), what
    assert rep.n_assigned + rep.n_short + rep.n_far + rep.n_ambiguous == rep.n_units
    return parts, units, c


def refused(ctx, code, fq, rule, rows, cap=None, needs=None):
    with pytest.raises(Refused) as r:
        demux(fq, rule, rows, out_cap=cap)
    assert r.value.code == code
    T, out = Buf(max(len(fq), 1), 3, fq if fq else None), Buf(max(len(fq), 1) + 16, 5)
    with pytest.raises(capi.SfqError) as e:
        ctx.demux_records(T.ptr, len(fq), rule, rows, out.ptr, out.n if cap is None else cap)
    assert e.value.code == code, str(e.value)
    assert out.back("the output of a refused call") == b"I" * out.n, "a refused call wrote to its output"
    if fq:
        assert T.back("the text") == fq
    if needs is not None:
        assert e.value.needed == needs == r.value.needed
    return str(e.value), r.value


# ---- classes: the digit boundaries of the sort ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("ns", [1, 2, 63, 64, 127, 128, 255, 256, 257, 4096])
def test_class_counts(ctx, ns, split):
    rng = np.random.default_rng(ns * 2 + split)
    rows = rows_of(ns, 7, ns)
    units = 2500 if ns < 4096 else 700
    fq = lane(rng, units, rows, 7, "hdr", pairs=split, junk=0.1)
    rule = Demux(hdr_parts(7), n_samples=ns, max_mm=1, pairs=split, split_mates=split)
    assert rule.n_parts == (2 if split else 1) * (ns + 1)
    parts, units_per, c = check(ctx, fq, rule, rows, msg="classes")
    assert c["n_assigned"] > units // 4 and c["n_assigned"] < units
    if ns >= 63:
        assert sum(1 for u in units_per[:ns] if u) > 50, "the units do not spread over the samples"
    if ns == 4096:
        assert any(units_per[s] for s in range(256, 4096)) and 0 in units_per[:ns], "a second digit and empty parts"


def test_all_units_to_one_sample(ctx):
    rng = np.random.default_rng(5)
    rows = rows_of(96, 6)
    fq = lane(rng, 3000, [rows[41]], 6, "hdr", junk=0)
    parts, units, c = check(ctx, fq, Demux(hdr_parts(6), n_samples=96, max_mm=6), rows, msg="one sample")
    assert c["n_far"] == 0 and c["n_short"] == 0 and units[41] > 1500
    fq = b"".join(rec(b"@x:" + rows[41], bases(rng, int(rng.integers(1, 90)))) for _ in range(3000))
    parts, units, _ = check(ctx, fq, Demux(hdr_parts(6), n_samples=96, max_mm=0), rows, msg="one sample, exact")
    assert units == [3000 if s == 41 else 0 for s in range(97)] and parts[41] == fq
    assert [len(p) for p in parts[:41] + parts[42:]] == [0] * 96          # empty parts: equal consecutive offsets (check compared them)


def test_all_units_unassigned(ctx):
    rng = np.random.default_rng(6)
    rows = rows_of(300, 8)
    fq = b"".join(rec(b"@x:NNNNNNNN", bases(rng, int(rng.integers(0, 70)))) for _ in range(2100))
    for split in (0, 1):
        parts, units, c = check(ctx, fq, Demux(hdr_parts(8), n_samples=300, max_mm=2, pairs=split, split_mates=split), rows, msg="all unassigned")
        assert c["n_far"] == c["n_units"] and units[300] == c["n_units"] and sum(units[:300]) == 0


# ---- unit counts: the tile's and the wavefront's boundaries ----------------------------------------------------------------------------

@pytest.mark.parametrize("units", [1, 2, 63, 64, 65, 255, 256, 257, 1023, TILE, 1025, 4097, 70001])
def test_unit_counts(ctx, units):
    rng = np.random.default_rng(units)
    rows = rows_of(5, 6, 3)
    fq = lane(rng, units, rows, 6, "inline", junk=0.3, lens=(0, 40))
    rule = Demux([DemuxPart(B, 0, 0, 0, 6)], n_samples=5, max_mm=1)
    check(ctx, fq, rule, rows, offs=(units % 16, (units * 7) % 16), msg="%d units" % units)
    if units in (257, 4097):                                           # and in pairs, split, over 300 classes: two digit passes
        rows = rows_of(300, 6, 4)
        fq = lane(rng, units, rows, 3, "inline2", pairs=True, lens=(0, 40))
        rule = Demux([DemuxPart(B, 0, 0, 0, 3), DemuxPart(B, 1, 0, 0, 3)], n_samples=300, max_mm=0, pairs=1, split_mates=1)
        check(ctx, fq, rule, rows, msg="%d pairs" % units)


# ---- barcodes and verdicts -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l0,l1", [(1, 0), (6, 0), (8, 0), (31, 0), (32, 0), (16, 16), (8, 8), (1, 31), (31, 1)])
def test_barcode_lengths(ctx, l0, l1):
    Bn = l0 + l1
    rng = np.random.default_rng(Bn * 40 + l1)
    rows = rows_of(4 if Bn == 1 else 40, Bn, Bn)
    fq = lane(rng, 1500, rows, l0, "hdr", junk=0.15)
    for mm in sorted({0, 1, min(2, Bn), Bn}):
        parts, units, c = check(ctx, fq, Demux(hdr_parts(l0, l1), n_samples=len(rows), max_mm=mm), rows, msg="B %d+%d, mm %d" % (l0, l1, mm))
        if mm == Bn:
            assert c["n_far"] == 0
    # inline, at a position, the same barcodes
    fq = b"".join(rec(b"@r", bases(rng, 5) + spoil(rng, rows[int(rng.integers(0, len(rows)))]) + bases(rng, int(rng.integers(0, 30)))) for _ in range(1500))
    check(ctx, fq, Demux([DemuxPart(B, 0, 0, 5, l0)] + ([DemuxPart(B, 0, 0, 5 + l0, l1)] if l1 else []), n_samples=len(rows), max_mm=1), rows,
          offs=(Bn % 16, 9), msg="inline B %d+%d" % (l0, l1))


def test_observed_bytes_that_are_no_bases(ctx):
    rows = [b"ACGTAC", b"TTTTTT", b"ACGTAA"]
    obs = [b"ACGTAC", b"acgtac", b"AcGtAc", b"NCGTAC", b"nCGTAC", b".CGTAC", b"ACGTA.", b"ACGTAN", b"NNNNNN", b"......", b"TTTTTN", b"TTTT.N",
           b"ACGTA\r", b"ACGTA@", b"ACGTA\x00", b"ACGTA\xc1", b"ACGTAa", b"acgtaA", b"tttttt", b"ACGTAG", b"BDHUBD", b"\x01\x03\x07\x14\x01\x03"]
    fq = b"".join(rec(b"@r%d:" % i + o, b"ACGT") for i, o in enumerate(obs))
    for mm in (0, 1, 2, 6):
        check(ctx, fq, Demux(hdr_parts(6), n_samples=3, max_mm=mm), rows, msg="no bases, mm %d" % mm)
    parts, units, c = check(ctx, fq, Demux(hdr_parts(6), n_samples=3, max_mm=0), rows)
    assert c["n_perfect"] == c["n_assigned"] == 6                      # the exact rows in either case, nothing with an N or a '.'
    # the same bytes inline, one record each, at every alignment of the text
    for i, o in enumerate(obs):
        check(ctx, rec(b"@r", o + b"AC"), Demux([DemuxPart(B, 0, 0, 0, 6)], n_samples=3, max_mm=1), rows, offs=(i % 16, 0), msg="inline %r" % o)


def test_ties_runners_up_and_far(ctx):
    rows = [b"AAAAAAAA", b"AAAAAACC", b"GGGGGGGG", b"GGGGTTTT"]
    cases = {b"AAAAAAAC": "ambiguous",        # one from row 0, one from row 1
             b"AAAAAAAA": 0,                  # exact; the runner-up two above
             b"AAAAAACA": "ambiguous",        # the same the other way round
             b"GGGGGGTT": "ambiguous",        # two from row 2, two from row 3
             b"GGGGGTTT": 3,                  # one from row 3, the runner-up (row 2) at three
             b"GGGGGGGT": 2,                  # one from row 2, row 3 at three
             b"CCCCCCCC": "far",
             b"AAAAAANN": "ambiguous",        # two from rows 0 and 1
             b"TAAAAAAA": 0}                  # one from row 0, the runner-up (row 1) at three
    fq = b"".join(rec(b"@q 1:N:0:" + o, b"ACGTACGT") for o in cases)
    parts, units, c = check(ctx, fq, Demux(hdr_parts(8), n_samples=4, max_mm=2), rows, msg="ties")
    for o, v in cases.items():
        r = rec(b"@q 1:N:0:" + o, b"ACGTACGT")
        where = [i for i, p in enumerate(parts) if r in p]
        assert where == [4 if isinstance(v, str) else v], (o, v, where)
    assert (c["n_ambiguous"], c["n_far"], c["n_perfect"], c["n_assigned"]) == (4, 1, 1, 4)
    # a unique minimum with the runner-up ONE above it: assigned, not ambiguous
    rows2 = [b"ACGTAC", b"ACGTTT"]
    fq = rec(b"@a:ACGTAG", b"A") + rec(b"@b:ACGTTG", b"A") + rec(b"@c:ACGTAC", b"A")      # distances (1, 2), (2, 1), (0, 2)
    parts, units, c = check(ctx, fq, Demux(hdr_parts(6), n_samples=2, max_mm=2), rows2, msg="runner-up")
    assert units == [2, 1, 0] and c["n_ambiguous"] == 0 and c["n_perfect"] == 1
    parts, units, c = check(ctx, fq, Demux(hdr_parts(6), n_samples=2, max_mm=0), rows2, msg="runner-up, mm 0")
    assert units == [1, 0, 2] and c["n_far"] == 2


# ---- header forms ----------------------------------------------------------------------------------------------------------------------

def test_header_forms(ctx):
    rows = [b"ATCACGTTAGGC", b"CGATGTACAGTG"]
    i5 = DemuxPart(H, 0, 1, 0, 6)
    hdrs = [b"@no colon ATCACG+TTAGGC", b"@ends in a colon:", b":", b"@", b"@x:ATCACG", b"@x:ATCACG+", b"@x:+TTAGGC", b"@x:ATCACG+TTAGGC",
            b"@x:ATCACG+TTAGGC+CGATGT", b"@x:ATCACG++TTAGGC", b"@x:ATCACGA+TTAGGCA", b"@x:ATCAC+TTAGGC", b"@x:ATCACG+TTAGG",
            b"@x:CGATGT+ACAGTG:ATCACG+TTAGGC", b"@x:ATCACG+TTAGGC:", b"@x+y:CGATGT+ACAGTG", b"@x ATCACG+TTAGGC:CGATGT", b":ATCACG+TTAGGC",
            b"@x:ATCACG+TTAGGC extra", b"@x:atcacg+ttaggc", b"@x:ATCACG+TTAGGC\r", b"@x:\rATCACG+TTAGGC", b"+:+", b"@:+:+ATCACG"]
    fq = b"".join(rec(h, b"ACGT") for h in hdrs)
    parts, units, c = check(ctx, fq, Demux([DemuxPart(H, 0, 0, 0, 6), i5], n_samples=2, max_mm=0), rows, msg="header forms")
    assert c["n_short"] >= 9 and c["n_perfect"] >= 6
    check(ctx, fq, Demux([DemuxPart(H, 0, 0, 0, 6)], n_samples=2, max_mm=1), [r[:6] for r in rows], msg="header forms, one part")
    check(ctx, fq, Demux([DemuxPart(H, 0, 1, 0, 6)], n_samples=2, max_mm=1), [r[6:] for r in rows], msg="header forms, subfield 1 alone")
    # pos > 0 in a subfield, and a field longer than pos + len
    check(ctx, fq, Demux([DemuxPart(H, 0, 0, 1, 5), DemuxPart(H, 0, 1, 2, 4)], n_samples=2, max_mm=1), [r[1:6] + r[8:] for r in rows], msg="header forms, pos")
    # every header length from 1 byte on, so that the field lies at every place of the aligned words; long headers up to 8190 bytes
    for lens in (range(1, 80), (255, 256, 257, 1000, 4095, 4096, 8189, 8190)):
        hs = []
        for L in lens:
            for tail in (b":ATCACG+TTAGGC", b":CGATGT+ACAGTG", b":ATCACG", b""):
                hs.append((b"@" + b"h" * L)[:max(L - len(tail), 0)] + tail if L >= len(tail) else (b"@" + b"h" * L)[:L])
            hs.append((b":" + b"+" * L)[:L])
            hs.append((b"@" + b":" * L)[:L])
        fq = b"".join(rec(h, b"AC") for h in hs)
        for off in (0, 5, 11):
            check(ctx, fq, Demux([DemuxPart(H, 0, 0, 0, 6), i5], n_samples=2, max_mm=1), rows, offs=(off, 0), msg="header lengths")


# ---- bases and the clip ------------------------------------------------------------------------------------------------------------------

def test_short_base_lines_and_clip(ctx):
    rng = np.random.default_rng(8)
    rows = [b"ACGTAC", b"TGCATG"]
    reads = [b"", b"A", b"ACGTA", b"ACGTAC", b"ACGTACG", b"NACGTAC", b"TGCATG", b"TGCATGA" * 5, b"TTACGTAC", b"TTTGCATG", b"TTTGCAT", b"TT", b"TTTGCATGN"]
    fq = b"".join(rec(b"@r%d" % i, b, bases(rng, len(b))) for i, b in enumerate(reads))
    for pos in (0, 2):
        for clip in (0, 1):
            parts, units, c = check(ctx, fq, Demux([DemuxPart(B, 0, 0, pos, 6)], n_samples=2, max_mm=0, clip=clip), rows, msg="clip %d at %d" % (clip, pos))
            assert c["n_short"] == sum(1 for b in reads if len(b) < pos + 6)
            assert c["bases_clipped"] == clip * (pos + 6) * c["n_assigned"] and c["n_assigned"] >= 3
    # clipped to an empty line: the record keeps its four line ends
    parts, _, _ = check(ctx, rec(b"@e", b"ACGTAC", b"!!!!!!"), Demux([DemuxPart(B, 0, 0, 0, 6)], n_samples=2, clip=1), rows, msg="clip to empty")
    assert parts[0] == b"@e\n\n+\n\n"
    # a barcode in the header: nothing to clip
    fq = rec(b"@x:ACGTAC", b"ACGTACGG") + rec(b"@x:TGCATG", b"")
    parts, _, c = check(ctx, fq, Demux(hdr_parts(6), n_samples=2, clip=1), rows, msg="clip, header")
    assert c["bases_clipped"] == 0 and b"".join(parts) == fq
    # many records, lengths around the clip, '+' lines that repeat the header
    recs = []
    for i in range(3000):
        b = spoil(rng, rows[i & 1]) + bases(rng, int(rng.integers(0, 50)))
        b = b[:int(rng.integers(0, len(b) + 1))] if i % 7 == 0 else b
        recs.append(rec(b"@r%d" % i, b, rng.integers(33, 74, len(b), dtype=np.uint8).tobytes(), plus=b"+r%d" % i if i % 3 == 0 else b"+"))
    fq = b"".join(recs)
    for offs in ((0, 0), (3, 13)):
        check(ctx, fq, Demux([DemuxPart(B, 0, 0, 0, 6)], n_samples=2, max_mm=1, clip=1), rows, offs=offs, msg="clip, many")


def test_clip_refuses_unequal_lines(ctx):
    rows = [b"ACGTAC", b"TGCATG"]
    good = [rec(b"@r%d" % i, b"ACGTACGG") for i in range(700)]
    bad = list(good)
    for i in (650, 333, 699):
        bad[i] = rec(b"@r%d" % i, b"ACGTACGG", b"IIIIIII")
    fq = b"".join(bad)
    rule = Demux([DemuxPart(B, 0, 0, 0, 6)], n_samples=2, clip=1)
    msg, r = refused(ctx, E_FORMAT, fq, rule, rows)
    assert r.record == 333 and "record 333 " in msg and "byte %d)" % r.offset in msg
    rule.first_record = 334
    msg, r = refused(ctx, E_FORMAT, fq, rule, rows)
    assert r.record == 650 and "record 650 " in msg and "byte %d)" % r.offset in msg
    rule.first_record, rule.n_records = 334, 316                       # records 334 .. 649: the bad ones lie outside
    check(ctx, fq, rule, rows, msg="clip, the bad records outside the range")
    rule = Demux([DemuxPart(B, 0, 0, 0, 6)], n_samples=2, clip=0)      # without clip the same text is accepted
    check(ctx, fq, rule, rows, msg="unequal lines without clip")


# ---- pairs -----------------------------------------------------------------------------------------------------------------------------

def test_pairs(ctx):
    rng = np.random.default_rng(9)
    rows = rows_of(30, 10, 9)
    fq = lane(rng, 2001, rows, 6, "inline2", pairs=True, lens=(0, 50))
    p = [DemuxPart(B, 0, 0, 0, 6), DemuxPart(B, 1, 0, 0, 4)]
    for split in (0, 1):
        for clip in (0, 1):
            parts, units, c = check(ctx, fq, Demux(p, n_samples=30, max_mm=1, pairs=1, split_mates=split, clip=clip), rows, offs=(split * 5, clip * 9),
                                    msg="pairs, split %d, clip %d" % (split, clip))
            assert c["n_units"] == 2001 and c["n_in_range"] == 4002 and c["bases_clipped"] == clip * 10 * c["n_assigned"]
            if split:
                for s in range(31):                                    # the mates of a sample stay in step
                    assert len(records(parts[2 * s])) == len(records(parts[2 * s + 1])) == units[s]
    # the barcode in the second mate's header, the first mate's says nothing
    codes = [spoil(rng, rows[i % 30]) for i in range(500)]
    fq2 = b"".join(rec(b"@p%d/1" % i, b"AC") + rec(b"@p%d/2 2:N:0:" % i + c, b"GT") for i, c in enumerate(codes))
    check(ctx, fq2, Demux([DemuxPart(H, 1, 0, 0, 10)], n_samples=30, max_mm=1, pairs=1), rows, msg="mate 1's header")
    check(ctx, fq2, Demux([DemuxPart(H, 1, 0, 0, 6), DemuxPart(H, 0, 0, 0, 4)], n_samples=30, max_mm=1, pairs=1), rows, msg="mate 0 without a field")
    fq2 = b"".join(rec(b"@p%d/1 1:N:0:" % i + c[6:], b"AC") + rec(b"@p%d/2 2:N:0:" % i + c[:6], b"GT") for i, c in enumerate(codes))
    check(ctx, fq2, Demux([DemuxPart(H, 1, 0, 0, 6), DemuxPart(H, 0, 0, 0, 4)], n_samples=30, max_mm=1, pairs=1), rows, msg="mate 1's header, then mate 0's")
    # an odd count
    rule = Demux(p, n_samples=30, pairs=1)
    one = len(text_of(records(fq)[0]))
    refused(ctx, E_FORMAT, fq[one:], rule, rows)
    rule.n_records = 7
    refused(ctx, E_FORMAT, fq, rule, rows)
    rule.first_record, rule.n_records = 1, 8                           # an odd first record: the check's
    assert capi.demux_check(rule, rows) == E_ARG
    refused(ctx, E_ARG, fq, rule, rows)


# ---- ranges and refusals -------------------------------------------------------------------------------------------------------------------

def test_ranges(ctx):
    rng = np.random.default_rng(10)
    rows = rows_of(9, 6, 1)
    fq = lane(rng, 3000, rows, 6, "hdr")
    for r0, nr in ((0, 1), (2999, 1), (2999, TO_END), (1000, 1025), (1, 2999), (17, TO_END), (0, 3000)):
        parts, units, c = check(ctx, fq, Demux(hdr_parts(6), n_samples=9, first_record=r0, n_records=nr), rows, msg="range %d+%d" % (r0, nr))
        assert c["n_in_range"] == (3000 - r0 if nr == TO_END else nr)
    for r0, nr in ((3000, TO_END), (3000, 1), (0, 3001), (2999, 2), (TO_END, TO_END), (5, TO_END - 3)):
        msg, _ = refused(ctx, E_ARG, fq, Demux(hdr_parts(6), n_samples=9, first_record=r0, n_records=nr), rows)
        assert "3000 records" in msg


def test_refusals(ctx):
    rng = np.random.default_rng(11)
    rows = rows_of(9, 6, 1)
    fq = lane(rng, 300, rows, 6, "hdr")
    rule = Demux(hdr_parts(6), n_samples=9)
    refused(ctx, E_FORMAT, fq[:-1], rule, rows)                        # no final line end
    refused(ctx, E_FORMAT, fq + b"@x", rule, rows)                     # lines that are no multiple of four (and no final line end)
    refused(ctx, E_FORMAT, fq + b"@x\n", rule, rows)
    refused(ctx, E_FORMAT, b"\n", rule, rows)
    refused(ctx, E_ARG, b"", rule, rows)
    bad = Demux(hdr_parts(6), n_samples=9, max_mm=7)
    refused(ctx, E_ARG, fq, bad, rows)
    refused(ctx, E_ARG, fq, rule, rows[:8] + [rows[0]])                # two equal rows
    # room: one byte short, with the size needed; the exact size
    parts, _, _ = demux(fq, rule, rows)
    need = sum(len(p) for p in parts)
    assert need == len(fq)
    refused(ctx, E_OVERFLOW, fq, rule, rows, cap=need - 1, needs=need)
    check(ctx, fq, rule, rows, slack=0, msg="the exact room")
    ranged = Demux(hdr_parts(6), n_samples=9, first_record=10, n_records=100)
    need = sum(len(p) for p in demux(fq, ranged, rows)[0])
    refused(ctx, E_OVERFLOW, fq, ranged, rows, cap=need - 1, needs=need)
    check(ctx, fq, ranged, rows, slack=0, msg="the exact room of a range")
    cl = Demux([DemuxPart(B, 0, 0, 0, 6)], n_samples=9, clip=1, max_mm=6)
    need = sum(len(p) for p in demux(fq, cl, rows)[0])
    assert need < len(fq)
    refused(ctx, E_OVERFLOW, fq, cl, rows, cap=need - 1, needs=need)
    check(ctx, fq, cl, rows, slack=0, msg="the exact room of a clip")


@pytest.mark.parametrize("toff", range(16))
def test_alignments(ctx, toff):
    rng = np.random.default_rng(20 + toff)
    rows = rows_of(20, 8, 2)
    fq = lane(rng, 700, rows, 8, "hdr", lens=(0, 30))
    fqi = lane(rng, 700, rows, 8, "inline", lens=(0, 30))
    for ooff in ((toff * 5) % 16, (toff + 8) % 16, 15 - toff):
        check(ctx, fq, Demux(hdr_parts(8), n_samples=20), rows, offs=(toff, ooff), msg="alignments")
        check(ctx, fqi, Demux([DemuxPart(B, 0, 0, 0, 8)], n_samples=20, clip=1), rows, offs=(toff, ooff), msg="alignments, inline and clip")


# ---- determinism -------------------------------------------------------------------------------------------------------------------------

def test_the_same_call_gives_the_same_bytes(ctx):
    rng = np.random.default_rng(12)
    rows = rows_of(300, 8, 5)
    fq = lane(rng, 20000, rows, 8, "hdr", lens=(0, 30))
    rule = Demux(hdr_parts(8), n_samples=300, max_mm=1)
    T = Buf(len(fq), 0, fq)
    got = []
    fresh = capi.Context(0, table_budget=1 << 30)
    try:
        for c in (ctx, ctx, fresh):
            out = Buf(len(fq), 0)
            n, off, units, rep = c.demux_records(T.ptr, len(fq), rule, rows, out.ptr, out.n)
            got.append((out.back("the output")[:n], off, units))
    finally:
        fresh.close()
    assert got[0] == got[1] == got[2]
    assert got[0][0] == b"".join(demux(fq, rule, rows)[0])

"""Trimmed records on the GPU (trim.hip, slimfastq_amd.h "trimmed records"): sfq_trim_records against a restatement of the header's rule
in Python over test_pairs.records(), on the smallest texts, with every term at its boundary, with the deciding bytes on either side of
every border of the kernels, in buffers at every alignment between guard bytes; the refusals; the report field by field.  Every
comparison is exact byte equality.  Every output is filled with a marker: a call writes its result and nothing else, a refused call
nothing at all."""
import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Trim
from test_pairs import Buf, reads, record, records, first_difference

pytestmark = pytest.mark.gpu
UNIT, ROW, SPAN, WG_TILE = 16, 1024, 16 << 10, 64 << 10
E_ARG, E_FORMAT, E_OVERFLOW, E_UNSUPPORTED = -1, -4, -5, -7
OFF32 = 0xFFFFFFFF


# ---- the rule --------------------------------------------------------------------------------------------------------------------

def terms(l2, l4, t):
    """(s, e, [a_lead > 0, b_trail < L, b_win < L, b_ad < L]) of one record's lines 2 and 4"""
    L = len(l2)
    assert len(l4) == L
    q = [b - t.qual_base for b in l4]
    a_head, b_tail = min(t.head, L), L - min(t.tail, L)
    a_lead = next((p for p in range(L) if q[p] >= t.lead_q), L) if t.lead_q else 0
    b_trail = 1 + max((p for p in range(L) if q[p] >= t.trail_q), default=-1) if t.trail_q else L
    b_win = b_ad = L
    w = t.win_len
    if w:
        b_win = next((p for p in range(0, L - w + 1) if 100 * sum(q[p:p + w]) < t.win_q_x100 * w), L)
    n = t.adapter_len
    if n:
        ad, up = bytes(t.adapter[:n]), l2.upper()
        for p in range(L):
            k = min(n, L - p)
            if k >= t.adapter_min and sum(up[p + j] != ad[j] for j in range(k)) <= t.adapter_mm * k // n:
                b_ad = p
                break
    s, e = max(a_head, a_lead), min(b_tail, b_trail, b_win, b_ad)
    e = max(e, s)
    if t.max_len != OFF32:
        e = min(e, s + t.max_len)
    return s, e, [a_lead > 0, b_trail < L, b_win < L, b_ad < L]


def trimmed(fq, t):
    """(the trimmed text, the report's fields)"""
    out, changed, emptied, bin_, bout, ncut = [], 0, 0, 0, 0, [0] * 4
    rs = records(fq)
    for r in rs:
        parts = r.split(b"\n")
        L = len(parts[1])
        s, e, cut = terms(parts[1], parts[3], t)
        parts[1], parts[3] = parts[1][s:e], parts[3][s:e]
        out.append(b"\n".join(parts))
        changed += (s, e) != (0, L)
        emptied += L > 0 and s == e
        bin_ += L
        bout += e - s
        ncut = [a + b for a, b in zip(ncut, cut)]
    res = b"".join(out)
    return res, (len(rs), changed, emptied, len(fq), len(res), bin_, bout, ncut)


def fields(rep):
    return (rep.n_records, rep.n_changed, rep.n_emptied, rep.text_bytes, rep.out_bytes, rep.bases_in, rep.bases_out, list(rep.n_cut))


def check(ctx, fq, t, offs=(0, 0), msg="", slack=37):
    """sfq_trim_records against the rule; returns the restatement's (result, report)"""
    want, rep_want = trimmed(fq, t)
    T, out = Buf(len(fq), offs[0], fq), Buf(len(want) + slack, offs[1])
    n, rep = ctx.trim_records(T.ptr, len(fq), t, out.ptr, out.n)
    got = out.back("the output")
    assert T.back("the text") == fq, "the text was written"
    what = "%s, offsets %s" % (msg, offs)
    assert n == len(want), (what, n, len(want))
    first_difference(got[:n], want, what)
    assert got[n:] == b"I" * (out.n - n), what + ": bytes behind the result were written"
    assert fields(rep) == rep_want, what
    return want, rep_want


def refused(ctx, code, fq, t, cap=None, needs=None, says=None):
    T, out = Buf(max(len(fq), 1), 3, fq if fq else None), Buf(max(len(fq), 1) + 16, 5)
    with pytest.raises(capi.SfqError) as e:
        ctx.trim_records(T.ptr, len(fq), t, out.ptr, out.n if cap is None else cap)
    assert e.value.code == code, str(e.value)
    assert out.back("the output of a refused call") == b"I" * out.n, "a refused call wrote to its output"
    if fq:
        assert T.back("the text") == fq
    if needs is not None:
        assert e.value.needed == needs
    if says is not None:
        assert says in str(e.value), str(e.value)


def rec(bases, quals=None, hdr=b"@r", plus=b"+"):
    return hdr + b"\n" + bases + b"\n" + plus + b"\n" + (b"I" * len(bases) if quals is None else quals) + b"\n"


def bases_of(fq):
    return [r.split(b"\n")[1] for r in records(fq)]


# ---- the smallest texts --------------------------------------------------------------------------------------------------------------

SMALLEST = [b"@\nA\n+\nI\n", b"@h\n\n+\n\n", b"@\nA\n+\nI"]
# every single term, once so that it cuts b"@\nA\n+\nI\n" and once so that it does not ('I' is quality 40)
SINGLE = [(dict(), False), (dict(head=1), True), (dict(head=0), False), (dict(tail=1), True), (dict(max_len=0), True), (dict(max_len=1), False),
          (dict(lead_q=41), True), (dict(lead_q=40), False), (dict(trail_q=41), True), (dict(trail_q=40), False),
          (dict(win_len=1, win_q_x100=4001), True), (dict(win_len=1, win_q_x100=4000), False), (dict(win_len=2, win_q_x100=9000), False),
          (dict(adapter=b"A", adapter_min=1), True), (dict(adapter=b"C", adapter_min=1), False), (dict(adapter=b"AC", adapter_min=1), True),
          (dict(adapter=b"AC", adapter_min=2), False)]


@pytest.mark.parametrize("fq", SMALLEST)
def test_smallest_texts(ctx, fq):
    for kw, cuts in SINGLE:
        want, rep = check(ctx, fq, Trim(**kw), msg="%r under %r" % (fq, kw))
        assert want.count(b"\n") == fq.count(b"\n")                    # the record keeps its four lines
        if bases_of(fq) != [b""]:
            assert (rep[1] == 1) == cuts, kw
    check(ctx, b"@\nC\n+\n!\n" + fq, Trim(lead_q=1), msg="a record in front that is cut to nothing")
    check(ctx, fq[:8] + b"\n" + fq if fq.endswith(b"I") else fq + fq, Trim(tail=1), msg="twice")


# ---- each term at its boundary -------------------------------------------------------------------------------------------------------

def test_crops_at_their_boundaries(ctx):
    L = 21
    fq = rec(b"ACGTACGTACGTACGTACGTA", bytes(range(40, 61))) + rec(b"", b"") + rec(b"ACG", b"#5I") + rec(b"ACGTACGTACGTACGTACGTAC" * 3)
    for v in (0, 1, L - 1, L, L + 1, OFF32 - 1):
        check(ctx, fq, Trim(head=v), msg="head %d" % v)
        check(ctx, fq, Trim(tail=v), msg="tail %d" % v)
        check(ctx, fq, Trim(max_len=v), msg="maxlen %d" % v)
        check(ctx, fq, Trim(head=3, max_len=v), msg="head 3, maxlen %d" % v)
    check(ctx, fq, Trim(head=OFF32, tail=OFF32), msg="both crops as large as they get")
    for h, t in ((10, 10), (10, 11), (11, 10), (11, 11), (20, 20), (0, 21), (21, 0)):
        want, _ = check(ctx, fq, Trim(head=h, tail=t), msg="head %d and tail %d" % (h, t))
        assert len(bases_of(want)[0]) == max(0, L - h - t)


def test_quality_cuts_at_their_boundaries(ctx):
    L = 40
    hi, lo = b"5", b"4"                                                # qualities 20 and 19
    quals = [hi + lo * (L - 1), lo * (L - 1) + hi, lo * L, hi * L, lo * 17 + hi + lo * 22, b" " * 5 + hi * 30 + b" " * 5, hi + lo * (L - 2) + hi,
             b"\x7f\xff" * 20]
    fq = b"".join(rec(b"ACGT" * 10, q) for q in quals) + rec(b"", b"") + b"@x\nACGT\n+\n" + b"45~4"    # the last line without its '\n'
    for q in (19, 20, 21):
        for kw in (dict(lead_q=q), dict(trail_q=q), dict(lead_q=q, trail_q=q)):
            check(ctx, fq, Trim(**kw), msg=repr(kw))
    want, rep = check(ctx, fq, Trim(lead_q=20), msg="q5=20")
    assert [len(b) for b in bases_of(want)[:7]] == [L, 1, 0, L, L - 17, L - 5, L]
    want, rep = check(ctx, fq, Trim(trail_q=20), msg="q3=20")
    assert [len(b) for b in bases_of(want)[:7]] == [1, L, 0, L, 18, L - 5, L]
    # a byte below the base is a negative quality; bases 0 and 126; a bound above every byte
    check(ctx, fq, Trim(lead_q=1, trail_q=1, qual_base=33), msg="the bytes below 33 alone are cut")
    check(ctx, fq, Trim(lead_q=0x35, trail_q=0x35, qual_base=0), msg="base 0")
    check(ctx, fq, Trim(lead_q=1, trail_q=1, qual_base=126), msg="base 126")
    check(ctx, fq, Trim(lead_q=130, trail_q=129, qual_base=126), msg="byte 255 alone passes the cut from the back")
    check(ctx, fq, Trim(lead_q=300), msg="no byte holds quality 300")
    check(ctx, fq, Trim(trail_q=OFF32), msg="nor 2^32 - 1")


def test_the_window_at_its_boundaries(ctx):
    w = 4
    bad = b"5545"                                                      # the sum 79 over the base 33, where 80 passes
    cases = [b"4" * (w - 1), bad[:w], b"5" * w, b"5" * w + b"4", b"4" + b"5" * w, b"5" * 20, bad + b"5" * 20, b"5" * 20 + bad, b"5" * 9 + b"4" + b"5" * 9,
             b"4" * 20, b"6" * 3 + b"2" + b"5" * 10]
    fq = b"".join(rec((b"ACGTN" * 8)[:len(q)], q) for q in cases)
    for thr in (1975, 1976, 2000, 2001, 2025, 2026):
        check(ctx, fq, Trim(win_len=w, win_q_x100=thr), msg="window of 4 below %d / 100" % thr)
    want, _ = check(ctx, fq, Trim(win_len=w, win_q_x100=2000), msg="a sum exactly at the threshold passes")
    assert [len(b) for b in bases_of(want)] == [3, 0, 4, 1, 0, 20, 0, 19, 6, 0, 1]
    long_q = bytes(33 + (i * 7) % 41 for i in range(150))
    fq = fq + rec((b"ACGT" * 38)[:150], long_q) + b"@x\nACGTACGT\n+\n" + b"55555544"
    for wl in (1, 2, 15, 16, 17, 31, 32):
        for thr in (0, 1, 1725, 2000, 2500, 4000, 9400):
            check(ctx, fq, Trim(win_len=wl, win_q_x100=thr), msg="window of %d below %d / 100" % (wl, thr))
    check(ctx, fq, Trim(win_len=5, win_q_x100=100, qual_base=60), msg="negative qualities in the sum")
    check(ctx, fq, Trim(win_len=32, win_q_x100=OFF32), msg="a bound no window reaches")


ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTC"
assert len(ADAPTER) == 32


@pytest.mark.parametrize("alen", [1, 2, 13, 16, 17, 31, 32])
def test_adapter_places_and_overlaps(ctx, alen):
    a = ADAPTER[:alen]
    fill = b"T" * 40                                                   # (no T in front of the adapter's first bases: no chance overlap)
    amin = min(3, alen)
    cases = [a + fill, fill[:7] + a + fill, fill + a, fill, fill + a + fill[:5] + a, a.lower() + fill, fill[:9] + bytes(c | 0x20 if i & 1 else c for i, c in enumerate(a))]
    fq = b"".join(rec(c) for c in cases)
    fq += rec(fill, hdr=b"@" + a) + rec(fill, hdr=b"@" + a, plus=b"+" + a) + rec(fill[:alen + 8], quals=a + b"I" * 8)
    fq += b"".join(rec(fill + a[:k]) for k in range(max(amin - 1, 0), alen))        # every partial overlap from adapter_min - 1 on
    fq += rec(a[:alen // 2]) + rec(a) + rec(b"") + rec(a[:amin])
    want, _ = check(ctx, fq, Trim(adapter=a), msg="adapter of %d" % alen)
    got = [len(b) for b in bases_of(want)]
    assert got[:7] == [0, 7, 40, 40, 40, 0, 9], "at the line's start, inside, at its end, nowhere, twice, in lower and in mixed case"
    assert got[7:10] == [40, 40, alen + 8], "an occurrence outside line 2 is none"
    check(ctx, fq, Trim(adapter=a, adapter_min=1), msg="adapter of %d, overlap 1" % alen)
    check(ctx, fq, Trim(adapter=a, adapter_min=alen), msg="adapter of %d, whole occurrences alone" % alen)
    # every offset mod 16 of the text: the same records behind a header that grows byte by byte
    for k in range(16):
        check(ctx, b"@" + b"h" * k + b"\n" + fq[3:], Trim(adapter=a), offs=(k % 3, 0), msg="adapter of %d, shifted by %d" % (alen, k))
    if alen >= 13:
        # mismatches: exactly met and exceeded by one, over the full length and over a partial overlap where the division bites
        def broken(seq, n):
            s = bytearray(seq)
            for i in range(n):
                j = (i * 5 + 1) % len(s)
                s[j] = ord("N") if i & 1 else {65: 67, 67: 71, 71: 84, 84: 65}[s[j]]
            return bytes(s)
        mm = 3
        k = alen * 2 // 3                                               # mm * k / alen = 1 or 2: fewer than mm
        allowed = mm * k // alen
        assert 0 < allowed < mm
        cases = [fill + broken(a, mm) + fill, fill + broken(a, mm + 1) + fill, fill + broken(a[:k], allowed), fill + broken(a[:k], allowed + 1),
                 fill + a[:5] + b"N" + a[6:], fill + a[:5] + b"n" + a[6:], fill + a[:5] + bytes([a[5] | 0x20]) + a[6:]]
        fq2 = b"".join(rec(c) for c in cases)
        want, _ = check(ctx, fq2, Trim(adapter=a, adapter_mm=mm), msg="adapter of %d, three mismatches" % alen)
        got = [len(b) for b in bases_of(want)]
        assert got[0] == 40 and got[2] == 40 and got[4:] == [40, 40, 40], got
        want, _ = check(ctx, fq2, Trim(adapter=a, adapter_mm=0), msg="adapter of %d, no mismatch" % alen)
        assert [len(b) for b in bases_of(want)][4:] == [len(cases[4]), len(cases[5]), 40]      # an N is a mismatch, lower case is not
        for m in (1, 2, alen):
            check(ctx, fq2 + fq, Trim(adapter=a, adapter_mm=m, adapter_min=2), msg="adapter of %d, mm %d" % (alen, m))


# ---- the deciding bytes on either side of every border ---------------------------------------------------------------------------------

BORDERS = [20 * UNIT, ROW, SPAN, WG_TILE]
TAIL = b"".join(rec(b"T" * 30, b"5" * 30) for _ in range(5))


def placed(bases, quals, at, line, off, border, d):
    """a record whose byte `at` of line 2 or 4 lies at border + d, counted from the 16-byte boundary in front of the text"""
    inner = (len(bases) + 1 + 2) if line == 4 else 0
    hlen = border + d - off - 1 - inner - at                           # the header's length: the byte lies at hlen + 1 + inner + at
    fq = rec(bases, quals, hdr=b"@" + b"h" * (hlen - 1)) + TAIL
    line_at = fq.split(b"\n")[line - 1]
    assert fq.index(line_at) + at + off == border + d
    return fq


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("off", [0, 7])
def test_deciding_bytes_on_either_side_of_every_border(ctx, border, off):
    L = 90
    bases = (b"CT" * 60)[:L]
    for d in (-1, 0):
        for p in (0, 1, 37, L - 1):
            q = b"4" * p + b"5" + b"4" * (L - 1 - p)                  # the one byte of quality 20
            fq = placed(bases, q, p, 4, off, border, d)
            want, _ = check(ctx, fq, Trim(lead_q=20, trail_q=20), offs=(off, 0), msg="the byte that decides q5 and q3 at %d%+d" % (border, d))
            assert bases_of(want)[0] == bases[p:p + 1]
        for wl in (4, 17, 32):
            for left in sorted({1, wl // 2, wl - 1}):                  # bytes of the failing window in front of the border
                p = 40
                q = b"5" * p + b"4" + b"5" * (L - 1 - p)              # the first failing window begins at p - wl + 1
                fq = placed(bases, q, p - wl + 1 + left, 4, off, border, d)
                want, _ = check(ctx, fq, Trim(win_len=wl, win_q_x100=2000), offs=(off, 3), msg="a failing window of %d across %d%+d" % (wl, border, d))
                assert len(bases_of(want)[0]) == p - wl + 1
        for alen in (2, 13, 32):
            a = ADAPTER[:alen]
            for left in sorted({1, alen // 2, alen - 1}):
                b = bases[:30] + a + bases[:25]
                fq = placed(b, None, 30 + left, 2, off, border, d)
                want, _ = check(ctx, fq, Trim(adapter=a, adapter_min=alen), offs=(off, 0), msg="an occurrence of %d across %d%+d" % (alen, border, d))
                assert bases_of(want)[0] == bases[:30]
                # the same place, the line ends in the occurrence: a partial overlap, and its rest at the start of the '+' line is none
                b = bases[:30] + a[:left]
                fq = rec(b, hdr=fq[:fq.index(b"\n")], plus=a[left:] + b"+") + TAIL
                want, _ = check(ctx, fq, Trim(adapter=a, adapter_min=1), offs=(off, 0), msg="a partial overlap of %d at %d%+d" % (left, border, d))
                assert bases_of(want)[0] == bases[:30]
                check(ctx, fq, Trim(adapter=a, adapter_min=left + 1), offs=(off, 0), msg="... one base short of the overlap asked for")


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_record_longer_than_a_tile(ctx, where):
    """70 000 bases: the record's positions come from many spans and several workgroups"""
    rng = np.random.default_rng(4)
    short = [record(rng, int(rng.integers(20, 60))) for _ in range(40)]
    L = 70000
    bases = bytearray(np.frombuffer(b"CT", np.uint8)[rng.integers(0, 2, L)].tobytes())
    a = ADAPTER[:20]
    at = {"first": 100, "middle": 35000, "last": L - 50}[where]
    other = {"first": 60000, "middle": 69000, "last": 20}[where]
    bases[at:at + 20] = a
    bases = bytes(bases)
    q = bytearray(b"5" * L)
    q[other] = ord("4")
    quals = bytes(q)
    fq = b"".join(short[:20]) + rec(bases, quals, hdr=b"@long") + b"".join(short[20:])
    for off in (0, 9):
        want, _ = check(ctx, fq, Trim(adapter=a), offs=(off, 0), msg="the adapter in its %s span" % where)
        assert len(bases_of(want)[20]) == at
        want, _ = check(ctx, fq, Trim(win_len=7, win_q_x100=2000), offs=(off, 3), msg="a failing window")
        assert len(bases_of(want)[20]) == other - 6
    lowq = bytearray(b"4" * L)
    lowq[at] = lowq[at + 17] = ord("5")
    fq = b"".join(short[:20]) + rec(bases, bytes(lowq), hdr=b"@long") + b"".join(short[20:])
    want, _ = check(ctx, fq, Trim(lead_q=20, trail_q=20), msg="the cuts from both ends")
    assert bases_of(want)[20] == bases[at:at + 18]
    check(ctx, fq, Trim(head=at, tail=L - at - 1000, lead_q=20, trail_q=20, win_len=32, win_q_x100=1950, adapter=a, adapter_mm=2), msg="all terms")


# ---- alignment, compaction, everything and nothing --------------------------------------------------------------------------------------

ALL = dict(head=2, tail=1, max_len=50, lead_q=5, trail_q=8, win_len=6, win_q_x100=2250, adapter=ADAPTER[:13], adapter_mm=1, adapter_min=3)
TEXTS = {"reads": (700, 1, 70, 2), "tiny": (2100, 1, 8, 3)}      # tiny: more than two scan blocks of pieces
_text = {}


def text(name):
    if name not in _text:
        rng = np.random.default_rng(7)
        rs = records(reads(*TEXTS[name]))
        for i in range(0, len(rs), 3):                                 # an adapter, whole or cut off, at the end of every third base line
            p = rs[i].split(b"\n")
            k = int(rng.integers(1, 14))
            p[1] = (p[1] + ADAPTER[:k])[-len(p[1]):] if len(p[1]) else p[1]
            rs[i] = b"\n".join(p)
        _text[name] = b"".join(rs)
    return _text[name]


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_every_term_on_random_reads(ctx, name):
    fq = text(name)
    want, rep = check(ctx, fq, Trim(**ALL), msg="all terms")
    assert 0 < rep[1] <= rep[0] and all(rep[7]) and len(records(want)) == rep[0]
    for kw in (dict(lead_q=30), dict(trail_q=30), dict(win_len=4, win_q_x100=3000), dict(adapter=ADAPTER[:13]), dict(head=3), dict(max_len=5)):
        check(ctx, fq, Trim(**kw), msg=repr(kw))


def test_every_alignment_of_text_and_output(ctx):
    fq = text("reads")[:3300]
    fq = fq[:fq.rindex(b"\n@") + 1]
    t = Trim(**ALL)
    for o in range(UNIT):
        check(ctx, fq, t, offs=(o, 0), msg="the text's offset")
        check(ctx, fq, t, offs=(0, o), msg="the output's offset")
        check(ctx, fq, t, offs=(o, 15 - o), msg="both")
        check(ctx, fq[:-1], t, offs=(o, o), msg="both, no final line end")


def test_everything_trimmed_to_nothing(ctx):
    fq = text("reads")
    want, rep = check(ctx, fq, Trim(max_len=0), msg="maxlen=0")
    assert want.count(b"\n") == fq.count(b"\n") and all(b == b"" for b in bases_of(want))
    assert rep[2] == rep[1] == sum(len(b) > 0 for b in bases_of(fq))
    check(ctx, fq[:-1], Trim(max_len=0), offs=(5, 11), msg="maxlen=0, no final line end")
    check(ctx, fq, Trim(head=OFF32), msg="head as large as it gets")


def test_nothing_on_is_the_text(ctx):
    for name in sorted(TEXTS):
        fq = text(name)
        for offs in ((0, 0), (3, 9)):
            want, rep = check(ctx, fq, Trim(), offs=offs, msg="no term")
            assert want == fq and rep[1] == 0
    want, _ = check(ctx, text("reads")[:-1], Trim(), msg="no term, no final line end")
    assert want == text("reads")[:-1]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    fq = reads(200, 20, 40, seed=8)
    t = Trim(head=3, trail_q=20)
    refused(ctx, E_FORMAT, fq + b"extra\n", t, says="lines")
    refused(ctx, E_ARG, b"", t)
    rs = records(fq)
    for bad in (150, 3):                                              # the smallest record whose lines 2 and 4 differ is named
        rs[bad] = rs[bad][:-2] + b"\n"
        broken = b"".join(rs)
        refused(ctx, E_FORMAT, broken, t, says="record %d (at byte %d)" % (bad, sum(len(r) for r in rs[:bad])))
        refused(ctx, E_FORMAT, broken, Trim(), says="record %d " % bad)
    want, _ = trimmed(fq, t)
    assert len(want) < len(fq)
    refused(ctx, E_OVERFLOW, fq, t, cap=len(want) - 1, needs=len(want))
    T, out = Buf(len(fq), 0, fq), Buf(len(want), 0)                   # ... and with exactly that size it succeeds
    assert ctx.trim_records(T.ptr, len(fq), t, out.ptr, len(want))[0] == len(want)
    assert out.back("an output of exactly the size needed") == want
    for bad in (Trim(win_len=33), Trim(adapter=b"ACGN"), Trim(adapter=b"acgt"), Trim(adapter=b"A", adapter_len=33), Trim(adapter=b"ACG", adapter_mm=4),
                Trim(adapter=b"ACG", adapter_min=0), Trim(adapter=b"ACG", adapter_min=4), Trim(qual_base=127)):
        assert capi.trim_check(bad) == E_ARG
        refused(ctx, E_ARG, fq, bad)
    check(ctx, fq, t, msg="after the refusals")

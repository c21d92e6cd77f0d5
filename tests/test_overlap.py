"""Overlapping mates on the GPU (ovl.hip, slimfastq_amd.h "overlapping mates"): sfq_overlap_pairs against a restatement of the header's
rule in Python over test_pairs.records() -- every offset d, the maximum by (ov, d) -- on the smallest texts, at every insert size, with
the deciding mismatch on either side of every border of the packing, with every threshold at its boundary, in buffers at every
alignment between guard bytes; the refusals; the report field by field, the histogram included.  Every comparison is exact byte
equality.  Every output is filled with a marker: a call writes its result and nothing else, a refused call nothing at all."""
import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Overlap
from test_pairs import Buf, records, first_difference

pytestmark = pytest.mark.gpu
UNIT, MAX_LEN, NHIST = 16, 512, 1025
E_ARG, E_FORMAT, E_OVERFLOW = -1, -4, -5
TO_END = 0xFFFFFFFFFFFFFFFF
COMP = {65: 84, 67: 71, 71: 67, 84: 65}


# ---- the rule --------------------------------------------------------------------------------------------------------------------

def winner(a, b, o):
    """(d, mm) of the pair's overlap, or None: a = line 2 of X, b = line 2 of Y"""
    La, Lb = len(a), len(b)
    # bytes that are no base become 0 in a and 1 in b': they mismatch everything
    A = np.array([c & ~0x20 if c & ~0x20 in COMP else 0 for c in a], np.uint8)
    B = np.array([COMP.get(c & ~0x20, 1) for c in reversed(b)], np.uint8)          # b'[j] = comp(b[Lb-1-j])
    best = None
    for d in range(-(Lb - 1), La):
        lo, hi = max(0, d), min(La, d + Lb)
        ov = hi - lo
        if ov < o.min_overlap:
            continue
        mm = int(np.count_nonzero(A[lo:hi] != B[lo - d:hi - d]))
        if mm <= o.max_mm and 100 * mm <= o.max_mm_pct * ov and (best is None or (ov, d) > best[0]):
            best = ((ov, d), mm)
    return None if best is None else (best[0][1], best[1])


def overlapped(fq, o):
    """(the text as sfq_overlap_pairs leaves it, the report's fields, the winners (d, mm) or None or "skipped" per pair)"""
    rs = records(fq)
    first = o.first_record
    count = len(rs) - first if o.n_records == TO_END else o.n_records
    assert first + count <= len(rs) and count % 2 == 0
    out, wins = list(rs), []
    pairs = skipped = overlap = ncut = bin_ = bout = mism = 0
    hist = [0] * NHIST
    for x in range(first, first + count, 2):
        X, Y = rs[x].split(b"\n"), rs[x + 1].split(b"\n")
        a, b = X[1], Y[1]
        assert len(X[3]) == len(a) and len(Y[3]) == len(b)
        pairs += 1
        bin_ += len(a) + len(b)
        ka, kb = len(a), len(b)
        if len(a) > MAX_LEN or len(b) > MAX_LEN:
            skipped += 1
            wins.append("skipped")
        else:
            w = winner(a, b, o)
            wins.append(w)
            if w is None:
                hist[0] += 1
            else:
                ins = w[0] + len(b)
                assert 1 <= ins <= len(a) + len(b) - o.min_overlap
                hist[ins] += 1
                overlap += 1
                mism += w[1]
                ka, kb = min(len(a), ins), min(len(b), ins)
                ncut += ka < len(a) or kb < len(b)
        if o.cut:
            X[1], X[3], Y[1], Y[3] = X[1][:ka], X[3][:ka], Y[1][:kb], Y[3][:kb]
            out[x], out[x + 1] = b"\n".join(X), b"\n".join(Y)
            bout += ka + kb
        else:
            bout += len(a) + len(b)
    res = b"".join(out)
    return res, (pairs, skipped, overlap, ncut, len(fq), len(res), bin_, bout, mism, hist), wins


def fields(rep):
    return (rep.n_pairs, rep.n_skipped, rep.n_overlap, rep.n_cut, rep.text_bytes, rep.out_bytes, rep.bases_in, rep.bases_out, rep.mismatches,
            list(rep.insert_hist))


def check(ctx, fq, o, offs=(0, 0), msg="", slack=37, want=None):
    """sfq_overlap_pairs against the rule; returns the restatement's (result, report, winners)"""
    res, rep_want, wins = overlapped(fq, o) if want is None else want
    T, out = Buf(len(fq), offs[0], fq), Buf(len(res) + slack, offs[1])
    n, rep = ctx.overlap_pairs(T.ptr, len(fq), o, out.ptr, out.n)
    got = out.back("the output")
    assert T.back("the text") == fq, "the text was written"
    what = "%s, offsets %s" % (msg, offs)
    assert n == len(res), (what, n, len(res))
    if o.cut:
        first_difference(got[:n], res, what)
        assert got[n:] == b"I" * (out.n - n), what + ": bytes behind the result were written"
    else:
        assert got == b"I" * out.n, what + ": a call that does not cut wrote to its output"
    got_f = fields(rep)
    for name, g, w in zip(("n_pairs", "n_skipped", "n_overlap", "n_cut", "text_bytes", "out_bytes", "bases_in", "bases_out", "mismatches", "insert_hist"),
                          got_f, rep_want):
        assert g == w, (what, name, g if name != "insert_hist" else [(i, x, y) for i, (x, y) in enumerate(zip(g, w)) if x != y])
    return res, rep_want, wins


def refused(ctx, code, fq, o, cap=None, needs=None, says=None):
    T, out = Buf(max(len(fq), 1), 3, fq if fq else None), Buf(max(len(fq), 1) + 16, 5)
    with pytest.raises(capi.SfqError) as e:
        ctx.overlap_pairs(T.ptr, len(fq), o, out.ptr, out.n if cap is None else cap)
    assert e.value.code == code, str(e.value)
    assert out.back("the output of a refused call") == b"I" * out.n, "a refused call wrote to its output"
    if fq:
        assert T.back("the text") == fq
    if needs is not None:
        assert e.value.needed == needs
    if says is not None:
        assert says in str(e.value), str(e.value)


def rec(bases, quals=None, hdr=b"@r", plus=b"+"):
    return hdr + b"\n" + bases + b"\n" + plus + b"\n" + (bytes(33 + i % 41 for i in range(len(bases))) if quals is None else quals) + b"\n"


def pair(a, b, hdr=b"@r"):
    return rec(a, hdr=hdr + b"/1") + rec(b, hdr=hdr + b"/2")


def rc(s):
    return bytes(COMP[c] for c in reversed(s))


def bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def mates(rng, frag, La, Lb):
    """the two reads of a fragment: what is behind the insert is read-through, random bases"""
    a, b = frag[:La], rc(frag)[:Lb]
    return a + bases(rng, La - len(a)), b + bases(rng, Lb - len(b))


def other(c):
    return {65: 67, 67: 71, 71: 84, 84: 65}[c]


def bases_of(fq):
    return [r.split(b"\n")[1] for r in records(fq)]


# ---- the smallest texts --------------------------------------------------------------------------------------------------------------

def test_smallest_texts(ctx):
    o = Overlap(min_overlap=1, max_mm=0, max_mm_pct=0)
    _, rep, wins = check(ctx, pair(b"A", b"T", hdr=b"@"), o, msg="A against T")
    assert wins == [(0, 0)] and rep[2] == 1 and rep[9][1] == 1
    _, rep, wins = check(ctx, pair(b"A", b"A", hdr=b"@"), o, msg="A against A")
    assert wins == [None] and rep[9][0] == 1
    for fq in (pair(b"", b""), pair(b"", b"ACGT"), pair(b"ACGT", b""), pair(b"", b"") + pair(b"A", b"T")):
        _, rep, wins = check(ctx, fq, o, msg="empty base lines")
        assert wins[0] is None and rep[1] == 0
    fq = pair(b"ACGTTGCA", b"TGCAACGT")[:-1]
    want, _, wins = check(ctx, fq, Overlap(min_overlap=4), msg="no final line end")
    assert wins == [(0, 0)]
    fq = pair(b"ACGTTGCAGG", b"TGCAACGTCC")[:-1]                    # ... whose last line is cut: the insert is 8
    want, _, wins = check(ctx, fq, Overlap(min_overlap=4, max_mm=0), offs=(5, 3), msg="no final line end, cut")
    assert wins == [(-2, 0)] and bases_of(want) == [b"ACGTTGCA", b"TGCAACGT"]
    check(ctx, fq, Overlap(min_overlap=4, max_mm=0, cut=0), msg="no final line end, counted only")


# ---- every offset ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("La,Lb", [(40, 40), (40, 27), (27, 40)])
def test_every_insert_size(ctx, La, Lb):
    rng = np.random.default_rng(La * 100 + Lb)
    genome = bases(rng, 400)
    o = Overlap(min_overlap=8)
    every = []
    for ins in range(1, 81):
        a, b = mates(rng, genome[100:100 + ins], La, Lb)
        fq = pair(a, b)
        every.append(fq)
        want, rep, wins = check(ctx, fq, o, msg="insert %d" % ins)
        if 8 <= ins <= La + Lb - 8:                                    # (below 8 bases a chance overlap may win; the rule's answer holds all the same)
            assert wins[0] is not None and rep[9][wins[0][0] + Lb] == 1
        if 12 <= ins <= La + Lb - 12:
            assert wins[0] == (ins - Lb, 0), (ins, wins)
            assert [len(x) for x in bases_of(want)] == [min(La, ins), min(Lb, ins)]
    want, rep, wins = check(ctx, b"".join(every), o, offs=(7, 9), msg="all 80 inserts in one text")
    assert rep[0] == 80 and sum(rep[9]) == 80
    check(ctx, b"".join(every), Overlap(min_overlap=8, cut=0), msg="all 80 inserts, counted only")


# ---- the packing's borders ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [31, 32, 33, 63, 64, 65, 511, 512, 513])
def test_the_deciding_mismatch_at_every_packing_border(ctx, L):
    """one mismatch decides (max_mm 0 against 1, only the true offset is long enough): at the overlap's first and last base and on either
    side of every 32-base word border of a and of b'"""
    rng = np.random.default_rng(L)
    for d in (0, -3, 5):
        ins = d + L
        frag = bases(rng, ins)
        a, b = mates(rng, frag, L, L)
        lo, hi = max(0, d), min(L, d + L)
        at = {lo, hi - 1}
        for w in range(32, L, 32):
            at |= {w - 1, w, w - 1 + d, w + d}                         # a's borders and b's (position p of a lies against p - d of b')
        at = sorted(p for p in at if lo <= p < hi)
        variants = []
        for p in at:
            broken = bytearray(a)
            broken[p] = other(broken[p])
            variants.append(pair(bytes(broken), b))
            broken = bytearray(b)                                      # the same place, broken in the second mate: b[Lb - 1 - (p - d)]
            broken[L - 1 - (p - d)] = other(broken[L - 1 - (p - d)])
            variants.append(pair(a, bytes(broken)))
        fq = pair(a, b) + b"".join(variants)
        ov = min(hi - lo, MAX_LEN)
        w0 = overlapped(fq, Overlap(min_overlap=ov, max_mm=0, max_mm_pct=100))
        w1 = overlapped(fq, Overlap(min_overlap=ov, max_mm=1, max_mm_pct=100))
        if L > MAX_LEN:
            assert w0[2] == ["skipped"] * (1 + len(variants)) and w0[0] == fq and w0[1][1] == 1 + len(variants)
        else:
            assert w0[2] == [(d, 0)] + [None] * len(variants)
            assert w1[2] == [(d, 0)] + [(d, 1)] * len(variants)
        check(ctx, fq, Overlap(min_overlap=ov, max_mm=0, max_mm_pct=100), want=w0, msg="L %d, d %d, no mismatch allowed" % (L, d))
        check(ctx, fq, Overlap(min_overlap=ov, max_mm=1, max_mm_pct=100), want=w1, offs=(3, 0), msg="L %d, d %d, one allowed" % (L, d))


def test_a_long_mate_beside_a_short_one(ctx):
    rng = np.random.default_rng(77)
    frag = bases(rng, 600)
    fq = b""
    for La, Lb in ((512, 40), (40, 512), (512, 1), (1, 512), (513, 40), (40, 513), (300, 200)):
        a, b = mates(rng, frag[:max(La, Lb)], La, Lb)
        fq += pair(a, b)
    _, rep, wins = check(ctx, fq, Overlap(min_overlap=20), msg="lengths far apart")
    assert rep[1] == 2 and wins[0] == (472, 0) and wins[1] == (0, 0) and wins[6] == (100, 0)
    check(ctx, fq, Overlap(min_overlap=1, max_mm=600, max_mm_pct=100), msg="everything accepted")


# ---- the thresholds at their boundaries ------------------------------------------------------------------------------------------------

def test_thresholds_at_their_boundaries(ctx):
    rng = np.random.default_rng(5)
    L, d = 60, -10
    frag = bases(rng, L + d)
    a, b = mates(rng, frag, L, L)                                      # the overlap is 50 bases

    def with_mm(k):
        x = bytearray(a)
        for i in range(k):
            x[7 * i] = other(x[7 * i])
        return pair(bytes(x), b)
    fq = b"".join(with_mm(k) for k in range(8))
    for mm in (0, 3, 4, 5):
        _, _, wins = check(ctx, fq, Overlap(min_overlap=50, max_mm=mm, max_mm_pct=100), msg="mm %d" % mm)
        assert wins == [(d, k) if k <= mm else None for k in range(8)]   # mm == max_mm passes, one more does not
    for pct in (5, 6, 7, 8):                                           # 100 * 3 == 6 * 50: three mismatches pass at 6 %, four do not
        _, _, wins = check(ctx, fq, Overlap(min_overlap=50, max_mm=50, max_mm_pct=pct), msg="pct %d" % pct)
        assert wins == [(d, k) if 100 * k <= pct * 50 else None for k in range(8)]
    assert 100 * 3 == 6 * 50
    for mo in (49, 50, 51):                                            # ov == min_overlap passes, one less does not
        _, _, wins = check(ctx, fq, Overlap(min_overlap=mo, max_mm=0, max_mm_pct=0), msg="min %d" % mo)
        assert wins[0] == ((d, 0) if mo <= 50 else None)
    check(ctx, fq, Overlap(min_overlap=1, max_mm=0, max_mm_pct=0), msg="min 1")
    check(ctx, fq, Overlap(min_overlap=MAX_LEN), msg="min 512")
    check(ctx, fq, Overlap(min_overlap=50, max_mm=0xFFFFFFFF, max_mm_pct=100), msg="mm as large as it gets")


def test_what_a_mismatch_is(ctx):
    rng = np.random.default_rng(6)
    a, b = mates(rng, bases(rng, 45), 50, 50)
    o = Overlap(min_overlap=45, max_mm=0)
    n_in_a, n_in_b = a[:9] + b"N" + a[10:], b[:9] + b"n" + b[10:]
    odd = a[:20] + b"." + a[21:]
    fq = pair(a, b) + pair(n_in_a, b) + pair(a, n_in_b) + pair(a.lower(), b) + pair(a, b.lower()) + pair(a.lower(), b.lower()) + pair(odd, b)
    fq += pair(bytes(c | 0x20 if i & 1 else c for i, c in enumerate(a)), b)
    _, _, wins = check(ctx, fq, o, msg="N and lower case")
    assert wins == [(-5, 0), None, None, (-5, 0), (-5, 0), (-5, 0), None, (-5, 0)]
    _, _, wins = check(ctx, fq, Overlap(min_overlap=45, max_mm=1), msg="N and lower case, one mismatch")
    assert wins[1] == wins[2] == wins[6] == (-5, 1)
    # an N on both sides of one place is one mismatch, not two; N against N does not match
    q = 50 - 1 - (9 + 5)
    both = pair(n_in_a, b[:q] + b"N" + b[q + 1:])
    _, _, wins = check(ctx, both, Overlap(min_overlap=45, max_mm=1), msg="N against N")
    assert wins == [(-5, 1)]
    _, _, wins = check(ctx, pair(b"N" * 30, b"N" * 30), Overlap(min_overlap=1, max_mm=0), msg="all N")
    assert wins == [None]


def test_ties(ctx):
    fq = pair(b"A" * 40, b"T" * 30)
    want, rep, wins = check(ctx, fq, Overlap(min_overlap=8), msg="every offset accepted")
    assert wins == [(10, 0)] and want == fq and rep[3] == 0 and rep[9][40] == 1      # the largest ov, then the largest d: nothing is cut
    want, _, wins = check(ctx, pair(b"A" * 30, b"T" * 40), Overlap(min_overlap=8), msg="the longer mate second")
    assert wins == [(0, 0)] and [len(x) for x in bases_of(want)] == [30, 40]
    want, _, wins = check(ctx, pair(b"AC" * 20, b"GT" * 20), Overlap(min_overlap=8), msg="a period of two")
    assert wins == [(0, 0)]


# ---- the range -------------------------------------------------------------------------------------------------------------------------

def ranged_text():
    rng = np.random.default_rng(8)
    out = []
    for i in range(11):
        a, b = mates(rng, bases(rng, 30 + 5 * i), 60, 60)
        out += [rec(a, hdr=b"@p%d/1" % i), rec(b, hdr=b"@p%d/2" % i)]
    return out


def test_ranges(ctx):
    rs = ranged_text()
    fq = rec(b"ACGTACGTAC", hdr=b"@lone") + b"".join(rs)               # the pairs begin at record 1
    o = Overlap(first_record=1, min_overlap=20)
    want, rep, _ = check(ctx, fq, o, msg="an odd first record")
    assert rep[0] == 11 and rep[3] > 5
    want, rep, _ = check(ctx, fq, Overlap(first_record=3, n_records=6, min_overlap=20), msg="records in front of and behind the range")
    assert rep[0] == 3
    assert records(want)[:3] == records(fq)[:3] and records(want)[9:] == records(fq)[9:] and records(want)[3:9] != records(fq)[3:9]
    # with an even first record the mates are others: X is a second mate, Y the next pair's first
    check(ctx, fq, Overlap(first_record=0, n_records=22, min_overlap=20), msg="pairs out of step")
    check(ctx, fq, Overlap(first_record=23, min_overlap=20), msg="an empty range at the text's end")
    check(ctx, fq, Overlap(first_record=21, n_records=2, min_overlap=20), msg="the last pair alone")
    refused(ctx, E_FORMAT, fq, Overlap(first_record=0, min_overlap=20), says="odd")
    refused(ctx, E_FORMAT, fq, Overlap(first_record=1, n_records=5, min_overlap=20), says="odd")
    refused(ctx, E_ARG, fq, Overlap(first_record=24, min_overlap=20))
    refused(ctx, E_ARG, fq, Overlap(first_record=1, n_records=24, min_overlap=20))
    # unequal lines 2 and 4: the smallest such record of the range is named; outside the range it is copied like any other
    r2 = records(fq)
    for bad in (14, 5):
        r2[bad] = r2[bad][:-2] + b"\n"
        broken = b"".join(r2)
        refused(ctx, E_FORMAT, broken, o, says="record %d (at byte %d)" % (bad, sum(len(r) for r in r2[:bad])))
    r2 = records(fq)
    r2[0] = r2[0][:-2] + b"\n"
    r2[22] = r2[22][:-2] + b"\n"
    broken = b"".join(r2)
    T, out = Buf(len(broken), 0, broken), Buf(len(broken), 0)
    n, rep = ctx.overlap_pairs(T.ptr, len(broken), Overlap(first_record=1, n_records=20, min_overlap=20), out.ptr, out.n)
    got = records(out.back("the output")[:n])
    assert got[0] == r2[0] and got[21:] == r2[21:] and rep.n_pairs == 10


def test_refusals(ctx):
    fq = b"".join(ranged_text())
    o = Overlap(min_overlap=20)
    refused(ctx, E_FORMAT, fq + b"extra\n", o, says="lines")
    refused(ctx, E_ARG, b"", o)
    want, rep, _ = overlapped(fq, o)
    assert len(want) < len(fq)
    refused(ctx, E_OVERFLOW, fq, o, cap=len(want) - 1, needs=len(want))
    T, out = Buf(len(fq), 0, fq), Buf(len(want), 0)                   # ... and with exactly that size it succeeds
    assert ctx.overlap_pairs(T.ptr, len(fq), o, out.ptr, len(want))[0] == len(want)
    assert out.back("an output of exactly the size needed") == want
    for bad in (Overlap(min_overlap=0), Overlap(min_overlap=MAX_LEN + 1), Overlap(max_mm_pct=101), Overlap(n_records=0)):
        assert capi.overlap_check(bad) == E_ARG
        refused(ctx, E_ARG, fq, bad)
    T = Buf(len(fq), 0, fq)
    with pytest.raises(capi.SfqError) as e:                            # a cut needs an output
        ctx.overlap_pairs(T.ptr, len(fq), o, None, 0)
    assert e.value.code == E_ARG
    check(ctx, fq, o, msg="after the refusals")


def test_counting_without_a_cut(ctx):
    fq = b"".join(ranged_text())
    cutting, counting = Overlap(min_overlap=20), Overlap(min_overlap=20, cut=0)
    _, rep_cut, _ = check(ctx, fq, cutting, msg="cut")
    res, rep, _ = check(ctx, fq, counting, msg="counted only")
    assert res == fq
    assert rep[:5] == rep_cut[:5] and rep[6] == rep_cut[6] and rep[8:] == rep_cut[8:]       # all but out_bytes and bases_out
    assert rep[5] == len(fq) and rep[7] == rep[6] and rep_cut[7] < rep_cut[6]
    T = Buf(len(fq), 5, fq)
    n, got = ctx.overlap_pairs(T.ptr, len(fq), counting, None, 0)     # no output at all
    assert n == len(fq) and fields(got) == rep and T.back("the text") == fq


def test_every_alignment_of_text_and_output(ctx):
    rng = np.random.default_rng(9)
    fq = b""
    for i in range(8):
        a, b = mates(rng, bases(rng, 20 + 13 * i), 61, 59)
        fq += pair(a, b, hdr=b"@p%d" % i)
    o = Overlap(min_overlap=12)
    want = overlapped(fq, o)
    cut_short = overlapped(fq[:-1], o)
    assert want[1][3] >= 3
    for k in range(UNIT):
        check(ctx, fq, o, offs=(k, 0), want=want, msg="the text's offset")
        check(ctx, fq, o, offs=(0, k), want=want, msg="the output's offset")
        check(ctx, fq, o, offs=(k, 15 - k), want=want, msg="both")
        check(ctx, fq[:-1], o, offs=(k, k), want=cut_short, msg="both, no final line end")
    for k in range(UNIT):                                              # every offset of the base lines themselves: a header that grows
        check(ctx, b"@" + b"h" * k + fq[1:], o, offs=(k % 5, 0), msg="shifted by %d" % k)


# ---- many pairs ------------------------------------------------------------------------------------------------------------------------

_many = {}


def many_pairs():
    """4096 pairs of 2 x 100 from one random genome, the insert uniform in [20, 240], 0.5 % substitutions; the rule's answer, once"""
    if not _many:
        rng = np.random.default_rng(10)
        genome = bases(rng, 50000)
        out = []
        for i in range(4096):
            ins = int(rng.integers(20, 241))
            at = int(rng.integers(0, len(genome) - ins))
            a, b = mates(rng, genome[at:at + ins], 100, 100)
            a, b = bytearray(a), bytearray(b)
            for read in (a, b):
                for p in np.flatnonzero(rng.random(100) < 0.005):
                    read[p] = other(read[p])
            out.append(pair(bytes(a), bytes(b), hdr=b"@r%d" % i))
        _many["fq"] = b"".join(out)
        _many["want"] = overlapped(_many["fq"], Overlap())
    return _many["fq"], _many["want"]


def test_many_pairs(ctx):
    fq, want = many_pairs()
    res, rep, wins = want
    cut = sum(w is not None and w[0] + 100 < 100 for w in wins)
    whole = sum(w is not None and w[0] + 100 >= 100 for w in wins)
    none = sum(w is None for w in wins)
    assert cut + whole + none == 4096 and rep[1] == 0
    assert min(cut, whole, none) >= 4096 // 5, (cut, whole, none)     # by construction about 36 / 32 / 32 %
    assert rep[3] == cut and rep[2] == cut + whole and rep[9][0] == none
    check(ctx, fq, Overlap(), want=want, offs=(3, 11), msg="4096 pairs, the default rule")
    counted = (fq, rep[:5] + (len(fq), rep[6], rep[6]) + rep[8:], wins)
    check(ctx, fq, Overlap(cut=0), want=counted, msg="4096 pairs, counted only")

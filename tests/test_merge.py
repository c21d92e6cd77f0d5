"""Merged mates on the GPU (mrg.hip, slimfastq_amd.h "merged mates"): sfq_merge_pairs against a restatement of the header's rule in
Python over test_pairs.records() -- the overlap test's winner, then the table position by position -- on the smallest texts, at every
insert size, with every row of the table at every border of a lane's eight bytes and of a 16-byte store, at the lengths that end the
search's words and the merge's rounds, in buffers at every alignment between guard bytes; the ranges and refusals; the report field by
field.  Every comparison is exact byte equality.  Every output is filled with a marker: a call writes its result and nothing else, a
refused call nothing at all, and the text is never written."""
import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Merge
from test_overlap import winner, pair, rec, mates, bases, other, rc, many_pairs
from test_pairs import Buf, records, first_difference

pytestmark = pytest.mark.gpu
UNIT, MAX_LEN, NHIST = 16, 512, 1025
E_ARG, E_FORMAT, E_OVERFLOW = -1, -4, -5
TO_END = 0xFFFFFFFFFFFFFFFF
COMP = {65: 84, 67: 71, 71: 67, 84: 65}
VALID = frozenset(b"ACGTacgt")
NAMES = ("n_pairs", "n_skipped", "n_merged", "text_bytes", "out_bytes", "merged_bytes", "bases_in", "bases_merged", "mismatches",
         "n_x_wins", "n_y_wins", "insert_hist")


# ---- the rule --------------------------------------------------------------------------------------------------------------------

def merged_record(X, Y, d, qual_base):
    """(the merged record, x wins, y wins, ties among the x wins, agreeing positions): X, Y = the mates' four lines, d the winner"""
    a, qa, b, qb = X[1], X[3], Y[1], Y[3]
    La, Lb = len(a), len(b)
    ins = d + Lb
    ob, oq = bytearray(), bytearray()
    xw = yw = ties = agree = 0
    for p in range(ins):
        j = p - d
        in_a, in_b = p < La, 0 <= j < Lb
        assert in_a or in_b
        x = qx = y = qy = None
        vx = vy = False
        if in_a:
            x, qx = a[p], qa[p]
            vx = x in VALID
        if in_b:
            yb, qy = b[Lb - 1 - j], qb[Lb - 1 - j]
            vy = yb in VALID
            y = COMP[yb & ~0x20] if vy else yb
        if not in_b:
            base, q = x, qx
        elif not in_a:
            base, q = y, qy
        elif vx and vy:
            if x & ~0x20 == y:
                base, q = x, max(qx, qy)
                agree += 1
            else:
                q = qual_base + min(max(abs(qx - qy), 2), 126 - qual_base)
                if qx >= qy:
                    base = x
                    xw += 1
                    ties += qx == qy
                else:
                    base = y
                    yw += 1
        elif vy:                                                       # only yb valid
            base, q = y, qy
        else:                                                          # only x valid, or neither
            base, q = x, qx
        ob.append(base)
        oq.append(q)
    return X[0] + b"\n" + bytes(ob) + b"\n" + X[2] + b"\n" + bytes(oq) + b"\n", xw, yw, ties, agree


def merged(fq, m, wins=None):
    """(the result, the report's fields in NAMES' order, the winners (d, mm) or None or "skipped" per pair, (ties, agreeing positions));
    wins: the winners where they are known already"""
    rs = records(fq)
    first = m.first_record
    count = len(rs) - first if m.n_records == TO_END else m.n_records
    assert first + count <= len(rs) and count % 2 == 0
    front, rest, found = [], [], []
    pairs = skipped = nm = bin_ = bm = mism = xw = yw = ties = agree = 0
    hist = [0] * NHIST
    for i, x in enumerate(range(first, first + count, 2)):
        X, Y = rs[x].split(b"\n"), rs[x + 1].split(b"\n")
        a, b = X[1], Y[1]
        assert len(X[3]) == len(a) and len(Y[3]) == len(b)
        pairs += 1
        bin_ += len(a) + len(b)
        w = None
        if len(a) > MAX_LEN or len(b) > MAX_LEN:
            skipped += 1
            found.append("skipped")
        else:
            w = winner(a, b, m) if wins is None else wins[i]
            found.append(w)
            hist[0 if w is None else w[0] + len(b)] += 1
        if w is None:
            rest += [rs[x], rs[x + 1]]
        else:
            ins = w[0] + len(b)
            assert 1 <= ins <= len(a) + len(b) - m.min_overlap
            r, rx, ry, rt, ra = merged_record(X, Y, w[0], m.qual_base)
            assert len(r) <= len(rs[x]) + len(rs[x + 1])
            front.append(r)
            nm += 1; bm += ins; mism += w[1]; xw += rx; yw += ry; ties += rt; agree += ra
    front, rest = b"".join(front), b"".join(rest)
    return front + rest, (pairs, skipped, nm, len(fq), len(front) + len(rest), len(front), bin_, bm, mism, xw, yw, hist), found, (ties, agree)


def fields(rep):
    return tuple(getattr(rep, n) for n in NAMES[:-1]) + (list(rep.insert_hist),)


def check(ctx, fq, m, offs=(0, 0), msg="", slack=37, want=None):
    """sfq_merge_pairs against the rule; returns the restatement's (result, report, winners, (ties, agreeing))"""
    want = merged(fq, m) if want is None else want
    res, rep_want = want[0], want[1]
    T, out = Buf(len(fq), offs[0], fq), Buf(len(res) + slack, offs[1])
    n, mb, rep = ctx.merge_pairs(T.ptr, len(fq), m, out.ptr, out.n)
    got = out.back("the output")
    assert T.back("the text") == fq, "the text was written"
    what = "%s, offsets %s" % (msg, offs)
    assert (n, mb) == (len(res), rep_want[5]), (what, n, mb, len(res), rep_want[5])
    first_difference(got[:n], res, what)
    assert got[n:] == b"I" * (out.n - n), what + ": bytes behind the result were written"
    for name, g, w in zip(NAMES, fields(rep), rep_want):
        assert g == w, (what, name, g if name != "insert_hist" else [(i, x, y) for i, (x, y) in enumerate(zip(g, w)) if x != y], w if name != "insert_hist" else "")
    return want


def refused(ctx, code, fq, m, cap=None, needs=None, says=None):
    T, out = Buf(max(len(fq), 1), 3, fq if fq else None), Buf(max(len(fq), 1) + 16, 5)
    with pytest.raises(capi.SfqError) as e:
        ctx.merge_pairs(T.ptr, len(fq), m, out.ptr, out.n if cap is None else cap)
    assert e.value.code == code, str(e.value)
    assert "merged mates:" in str(e.value), str(e.value)
    assert out.back("the output of a refused call") == b"I" * out.n, "a refused call wrote to its output"
    if fq:
        assert T.back("the text") == fq
    if needs is not None:
        assert e.value.needed == needs
    if says is not None:
        assert says in str(e.value), str(e.value)


def pairq(a, qa, b, qb, hdr=b"@r"):
    return rec(bytes(a), bytes(qa), hdr=hdr + b"/1") + rec(bytes(b), bytes(qb), hdr=hdr + b"/2")


def lines2(fq):
    return [r.split(b"\n")[1] for r in records(fq)]


# ---- the smallest texts --------------------------------------------------------------------------------------------------------------

def test_smallest_texts(ctx):
    m = Merge(min_overlap=1, max_mm=0, max_mm_pct=0)
    res, rep, wins, _ = check(ctx, pair(b"A", b"T", hdr=b"@"), m, msg="A against T")
    assert wins == [(0, 0)] and res == b"@/1\nA\n+\n!\n" and rep[2] == 1 and rep[5] == len(res)
    fq = pair(b"A", b"A", hdr=b"@")
    res, rep, wins, _ = check(ctx, fq, m, msg="A against A")
    assert wins == [None] and res == fq and rep[2] == 0 and rep[5] == 0
    for fq in (pair(b"", b""), pair(b"", b"ACGT"), pair(b"ACGT", b""), pair(b"", b"") + pair(b"A", b"T")):
        res, rep, wins, _ = check(ctx, fq, m, msg="empty base lines")
        assert wins[0] is None and rep[1] == 0
    fq = pair(b"ACGTTGCA", b"TGCAACGT")[:-1]                           # no final line end, the last pair merges
    res, rep, wins, _ = check(ctx, fq, Merge(min_overlap=4), offs=(5, 3), msg="no final line end, merged")
    assert wins == [(0, 0)] and res.endswith(b"\n") and rep[5] == len(res) and lines2(res) == [b"ACGTTGCA"]
    fq = pair(b"ACGTTGCA", b"TGCAACGT") + pair(b"AAAAAAAA", b"CCCCCCCC")[:-1]      # ... and one whose last pair does not
    res, rep, wins, _ = check(ctx, fq, Merge(min_overlap=4, max_mm=0), offs=(2, 9), msg="no final line end, unmerged")
    assert wins == [(0, 0), None] and not res.endswith(b"\n") and res[rep[5]:] == fq[len(fq) // 2 + 1:]


# ---- every insert ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("La,Lb", [(40, 40), (40, 27), (27, 40)])
def test_every_insert_size(ctx, La, Lb):
    """d < 0, d = 0, d > 0, I < La, I = La, I > La, and the positions that lie only in a and only in b'"""
    rng = np.random.default_rng(La * 100 + Lb)
    genome = bases(rng, 400)
    m = Merge(min_overlap=8)
    every = []
    for ins in range(1, 81):
        a, b = mates(rng, genome[100:100 + ins], La, Lb)
        fq = pair(a, b)
        every.append(fq)
        res, rep, wins, _ = check(ctx, fq, m, msg="insert %d" % ins)
        if 12 <= ins <= La + Lb - 12:
            assert wins[0] == (ins - Lb, 0), (ins, wins)
            assert rep[2] == 1 and rep[5] == len(res) and [len(x) for x in lines2(res)] == [ins]
            assert lines2(res)[0] == genome[100:100 + ins]             # the fragment itself
    res, rep, wins, _ = check(ctx, b"".join(every), m, offs=(7, 9), msg="all 80 inserts in one text")
    assert rep[0] == 80 and sum(rep[11]) == 80 and 0 < rep[2] < 80


# ---- every row of the table ------------------------------------------------------------------------------------------------------------

def lower(c):
    return c | 0x20


# an edit of position p of the merged read: x = a[p], qx = qa[p], yb = b[k], qy = qb[k]; returns the row it makes (base from, quality)
def differ(dq):
    def edit(a, qa, b, qb, p, k):
        a[p] = other(a[p])
        qa[p], qb[k] = 60 + max(dq, 0), 60 + max(-dq, 0)
    return edit


def agree(dq):
    def edit(a, qa, b, qb, p, k):
        qa[p], qb[k] = 60 + max(dq, 0), 60 + max(-dq, 0)
    return edit


def extreme(a, qa, b, qb, p, k):
    a[p] = other(a[p])
    qa[p], qb[k] = 126, 33


def extreme_y(a, qa, b, qb, p, k):
    a[p] = other(a[p])
    qa[p], qb[k] = 33, 126


def n_in_x(a, qa, b, qb, p, k):
    a[p] = ord("N")


def n_in_y(a, qa, b, qb, p, k):
    b[k] = ord("n")


def dots(a, qa, b, qb, p, k):
    a[p] = b[k] = ord(".")


def lower_x(a, qa, b, qb, p, k):
    a[p] = lower(a[p])


def lower_y(a, qa, b, qb, p, k):
    b[k] = lower(b[k])


def lower_y_wins(a, qa, b, qb, p, k):                                  # ... comes back upper case and complemented
    a[p] = other(a[p])
    b[k] = lower(b[k])
    qa[p], qb[k] = 40, 70


def lower_x_wins(a, qa, b, qb, p, k):
    a[p] = lower(other(a[p]))
    qa[p], qb[k] = 70, 40


def lower_y_beside_n(a, qa, b, qb, p, k):
    a[p] = ord("N")
    b[k] = lower(b[k])


EDITS = [differ(0), differ(1), differ(-1), differ(30), differ(-30), agree(0), agree(1), agree(-1), extreme, extreme_y, n_in_x, n_in_y, dots,
         lower_x, lower_y, lower_y_wins, lower_x_wins, lower_y_beside_n]


@pytest.mark.parametrize("qual_base", [33, 64, 124])
def test_every_row_of_the_table(ctx, qual_base):
    """One pair of 2 x 50 with a 45-base insert, one overlap position edited to make each row, at the overlap's first and last position
    and at 7, 8, 15, 16: the borders of a lane's eight bytes and of a 16-byte store.  Positions 63 and 64 do not exist in a 45-base
    read: a pair of 2 x 100 with a 90-base insert carries the same edits there (and at all the others)."""
    rng = np.random.default_rng(6)
    m = Merge(min_overlap=30, max_mm=5, max_mm_pct=20, qual_base=qual_base)
    text, n_pairs = [], 0
    for L, ins, at in ((50, 45, (0, 44, 7, 8, 15, 16)), (100, 90, (0, 89, 7, 8, 15, 16, 63, 64))):
        d = ins - L
        a, b = mates(rng, bases(rng, ins), L, L)
        # a byte of Y outside the overlap, lower case and no base: read-through, it reaches nothing
        b = b[:L - 2] + b".g"
        q0 = bytes(33 + (7 * i) % 60 for i in range(L))
        text.append(pairq(a, q0, b, q0[::-1]))
        n_pairs += 1
        for edit in EDITS:
            for p in at:
                k = L - 1 - (p - d)
                A, QA, B, QB = bytearray(a), bytearray(q0), bytearray(b), bytearray(q0[::-1])
                edit(A, QA, B, QB, p, k)
                text.append(pairq(A, QA, B, QB, hdr=b"@e%d" % n_pairs))
                n_pairs += 1
    fq = b"".join(text)
    want = merged(fq, m)
    res, rep, wins, (ties, agreeing) = want
    assert all(w is not None and w[1] <= 1 for w in wins) and rep[2] == n_pairs, "an edit changed the winner"
    assert rep[9] >= 5 * 14 and rep[10] >= 4 * 14 and ties >= 14       # every "differ" edit at every position
    got = records(res)
    assert len(got) == n_pairs
    # the rows, read off the restatement's own result at the first pair's edits (position 0 of the 45-base read)
    row = {e: got[1 + 6 * i].split(b"\n") for i, e in enumerate(EDITS)}
    plain = got[0].split(b"\n")
    floor, cap = qual_base + 2, 126
    assert row[EDITS[0]][3][0] == floor and row[EDITS[1]][3][0] == floor and row[EDITS[2]][3][0] == floor      # a difference of 0 and of 1
    assert row[EDITS[3]][3][0] == qual_base + min(30, 126 - qual_base)
    assert row[extreme][3][0] == cap and row[extreme_y][3][0] == cap
    assert row[extreme][1][0] == other(plain[1][0]) and row[extreme_y][1][0] == plain[1][0]
    assert row[n_in_x][1][0] == plain[1][0] and row[n_in_y][1][0] == plain[1][0] and row[dots][1][0] == ord(".")
    assert row[lower_x][1][0] == lower(plain[1][0]) and row[lower_y][1][0] == plain[1][0]
    assert row[lower_y_wins][1][0] == plain[1][0] and row[lower_x_wins][1][0] == lower(other(plain[1][0]))
    assert row[lower_y_beside_n][1][0] == plain[1][0]
    check(ctx, fq, m, want=want, offs=(1, 6), msg="every row, qual_base %d" % qual_base)


# ---- lengths -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [31, 32, 33, 63, 64, 65, 511, 512, 513])
def test_lengths(ctx, L):
    rng = np.random.default_rng(L)
    m = Merge(min_overlap=20, max_mm=1)
    text = []
    for d in (0, -3, 5):
        frag = bases(rng, d + L)
        a, b = mates(rng, frag, L, L)
        broken = bytearray(a)
        broken[max(0, d)] = other(broken[max(0, d)])                   # the overlap's first position, by the two quality rows
        text += [pair(a, b, hdr=b"@d%d" % (d + 3)), pair(bytes(broken), b, hdr=b"@x%d" % (d + 3))]
    fq = b"".join(text)
    want = merged(fq, m)
    res, rep, wins, _ = want
    if L > MAX_LEN:
        assert wins == ["skipped"] * 6 and res == fq and rep[1] == 6 and rep[2] == 0 and rep[5] == 0
    else:
        assert wins == [(0, 0), (0, 1), (-3, 0), (-3, 1), (5, 0), (5, 1)]
        assert [len(x) for x in lines2(res)] == [L, L, L - 3, L - 3, L + 5, L + 5]
    check(ctx, fq, m, want=want, offs=(L % 16, 3), msg="L %d" % L)


def test_the_longest_merged_read(ctx):
    rng = np.random.default_rng(994)
    frag = bases(rng, 994)
    a, b = mates(rng, frag, 512, 512)
    fq = pair(b"ACGT" * 5, b"ACGT" * 5) + pair(a, b, hdr=b"@longest") + pair(b"A" * 40, b"C" * 40)
    m = Merge(min_overlap=30, max_mm=0)
    want = merged(fq, m)
    assert want[2][1] == (482, 0) and lines2(want[0])[1 if want[2][0] else 0] == frag
    check(ctx, fq, m, want=want, offs=(9, 4), msg="I = 994")


def test_lines_1_and_3_longer_than_any_staging(ctx):
    rng = np.random.default_rng(9000)
    a, b = mates(rng, bases(rng, 130), 100, 100)
    name = b"@" + bytes(rng.integers(48, 123, 8999, dtype=np.uint8))
    fq = pair(b"ACGTACGTAC", b"GGGGGGGGGG")
    fq += rec(a, hdr=name, plus=b"+" + name[1:]) + rec(b, hdr=name)
    fq += pair(b"ACGTTGCA", b"TGCAACGT")
    m = Merge(min_overlap=8)
    want = merged(fq, m)
    assert want[2] == [None, (30, 0), (0, 0)] and len(want[0]) > 18000
    for offs in ((0, 0), (5, 11), (15, 1)):
        check(ctx, fq, m, want=want, offs=offs, msg="a header of 9000 bytes")


# ---- alignment ---------------------------------------------------------------------------------------------------------------------------

def mixed_pairs():
    rng = np.random.default_rng(9)
    fq = b""
    for i in range(8):
        a, b = mates(rng, bases(rng, 20 + 13 * i), 61, 59)
        if i in (1, 4, 6):
            b = bases(rng, 59)                                         # another fragment's mate: nothing to merge
        fq += pair(a, b, hdr=b"@p%d" % i)
    return fq


def test_every_alignment_of_text_and_output(ctx):
    fq = mixed_pairs()
    m = Merge(min_overlap=12)
    want = merged(fq, m)
    cut_short = merged(fq[:-1], m)
    assert want[1][2] >= 3 and want[1][0] - want[1][2] >= 3
    for k in range(UNIT):
        check(ctx, fq, m, offs=(k, 0), want=want, msg="the text's offset")
        check(ctx, fq, m, offs=(0, k), want=want, msg="the output's offset")
        check(ctx, fq, m, offs=(k, 15 - k), want=want, msg="both")
        check(ctx, fq[:-1], m, offs=(k, k), want=cut_short, msg="both, no final line end")
    ends = set()
    for k in range(UNIT):                                              # a header that grows: the merged part ends, and the piece copy starts, at every offset
        grown = b"@" + b"h" * k + fq[1:]
        w = check(ctx, grown, m, offs=(k % 5, 0), msg="shifted by %d" % k)
        ends.add(w[1][5] % UNIT)
    assert len(ends) == UNIT
    # exactly the room needed is enough, one byte less is not
    check(ctx, fq, m, offs=(3, 0), want=want, slack=0, msg="out_cap = needed")
    refused(ctx, E_OVERFLOW, fq, m, cap=len(want[0]) - 1, needs=len(want[0]))


# ---- ranges and refusals -----------------------------------------------------------------------------------------------------------------

def ranged_text():
    rng = np.random.default_rng(8)
    out = []
    for i in range(11):
        a, b = mates(rng, bases(rng, 30 + 5 * i), 60, 60)
        if i in (2, 7, 10):
            b = bases(rng, 60)
        out += [rec(a, hdr=b"@p%d/1" % i), rec(b, hdr=b"@p%d/2" % i)]
    return out


def test_ranges(ctx):
    rs = ranged_text()
    fq = rec(b"ACGTACGTAC", hdr=b"@lone") + b"".join(rs)               # the pairs begin at record 1
    m = Merge(first_record=1, min_overlap=20)
    res, rep, _, _ = check(ctx, fq, m, msg="an odd first record")
    assert rep[0] == 11 and rep[2] >= 6 and b"@lone" not in res        # records outside the range are dropped
    res, rep, wins, _ = check(ctx, fq, Merge(first_record=3, n_records=6, min_overlap=20), msg="records in front of and behind the range")
    assert rep[0] == 3 and wins[1] is None and len(records(res)) == 4 and res[rep[5]:] == rs[4] + rs[5]
    # with an even first record the mates are others: X is a second mate, Y the next pair's first
    check(ctx, fq, Merge(first_record=0, n_records=22, min_overlap=20), msg="pairs out of step")
    res, rep, _, _ = check(ctx, fq, Merge(first_record=23, min_overlap=20), msg="an empty range at the text's end")
    assert res == b"" and rep[0] == 0
    res, rep, _, _ = check(ctx, fq, Merge(first_record=21, n_records=2, min_overlap=20), msg="the last pair alone")
    assert res == rs[20] + rs[21]
    check(ctx, fq, Merge(first_record=19, n_records=2, min_overlap=20), msg="one pair that merges")
    refused(ctx, E_FORMAT, fq, Merge(first_record=0, min_overlap=20), says="odd")
    refused(ctx, E_FORMAT, fq, Merge(first_record=1, n_records=5, min_overlap=20), says="odd")
    refused(ctx, E_ARG, fq, Merge(first_record=24, min_overlap=20))
    refused(ctx, E_ARG, fq, Merge(first_record=1, n_records=24, min_overlap=20))
    # unequal lines 2 and 4: the smallest such record of the range is named; outside the range it is ignored
    r2 = records(fq)
    for bad in (14, 5):
        r2[bad] = r2[bad][:-2] + b"\n"
        broken = b"".join(r2)
        refused(ctx, E_FORMAT, broken, m, says="record %d (at byte %d)" % (bad, sum(len(r) for r in r2[:bad])))
    r2 = records(fq)
    r2[0] = r2[0][:-2] + b"\n"
    r2[22] = r2[22][:-2] + b"\n"
    broken = b"".join(r2)
    inside = Merge(first_record=1, n_records=20, min_overlap=20)
    want = merged(b"".join(r2[1:21]), Merge(min_overlap=20))
    T, out = Buf(len(broken), 0, broken), Buf(len(broken), 0)
    n, mb, rep = ctx.merge_pairs(T.ptr, len(broken), inside, out.ptr, out.n)
    assert out.back("the output")[:n] == want[0] and (n, mb, rep.n_pairs) == (len(want[0]), want[1][5], 10)


def test_refusals(ctx):
    fq = b"".join(ranged_text())
    m = Merge(min_overlap=20)
    refused(ctx, E_FORMAT, fq + b"extra\n", m, says="lines")
    refused(ctx, E_ARG, b"", m)
    want = merged(fq, m)
    assert len(want[0]) < len(fq)
    refused(ctx, E_OVERFLOW, fq, m, cap=len(want[0]) - 1, needs=len(want[0]))
    refused(ctx, E_OVERFLOW, fq, m, cap=0, needs=len(want[0]))
    for bad in (Merge(min_overlap=0), Merge(min_overlap=MAX_LEN + 1), Merge(max_mm_pct=101), Merge(n_records=0), Merge(qual_base=32), Merge(qual_base=125)):
        assert capi.merge_check(bad) == E_ARG
        refused(ctx, E_ARG, fq, bad)
    assert capi.merge_check(Merge(qual_base=33)) == 0 and capi.merge_check(Merge(qual_base=124)) == 0
    T = Buf(len(fq), 0, fq)
    with pytest.raises(capi.SfqError) as e:                            # a merge needs an output
        ctx.merge_pairs(T.ptr, len(fq), m, None, 0)
    assert e.value.code == E_ARG
    check(ctx, fq, m, want=want, msg="after the refusals")


# ---- many pairs ----------------------------------------------------------------------------------------------------------------------------

def test_many_pairs(ctx):
    """test_overlap's 4096 pairs of 2 x 100, the default rule.  The restatement gives 2603 merged of 4096, 893 positions where X wins
    (44 of them ties) and 792 where Y wins, 166 555 agreeing positions, 552 106 merged bytes of a 1 742 676-byte text."""
    fq, (_, _, wins) = many_pairs()
    m = Merge()
    want = merged(fq, m, wins=wins)
    res, rep, found, (ties, agreeing) = want
    assert found == wins
    print("merged %d of %d, x wins %d, y wins %d, ties %d, agreeing %d, merged bytes %d of %d" % (rep[2], rep[0], rep[9], rep[10], ties, agreeing, rep[5], len(fq)))
    assert rep[0] == 4096 and rep[2] >= 1638 and rep[0] - rep[2] >= 819
    assert rep[9] >= 100 and rep[10] >= 100 and ties >= 10
    check(ctx, fq, m, want=want, offs=(3, 11), msg="4096 pairs, the default rule")

"""CPU: the inputs of prior_mint.py are what test_prior_edges.py takes them for.  By the oracle's own results (O.qlt_histogram,
O.qlt_prior_rows, O.qlt_frozen_rows) every text holds the classes it claims, every count table is scaled by the shifts it names, every row
family has the floors, the ties and the correction it was built for, and the text coded under the families meets every (member, symbol) MIN
times or more.  These are conditions on the inputs, not measurements."""
import numpy as np
import pytest

import prior_mint as M
import util
from oracle import oracle as O


@pytest.mark.parametrize("name", M.TEXTS)
def test_text_holds_what_it_claims(name):
    t = M.text(name)
    assert M.legal(t), name
    assert (name in M.WAVE_TEXTS) == M.is_wave(t)
    got = M.classes(name)
    for cls in M.claims(name):
        assert got.get(cls, 0) >= 1, (name, cls)
    qoff, qlen = M.lines(t)
    assert int(qlen.min()) >= 1                              # (colour space: a symbol behind the primer's)


def test_crowded_workgroups_hold_more_keys_than_the_table_has_slots():
    """256 records of 150 uniform qualities: 27 457 / 36 255 / 28 972 distinct keys at levels 1 / 2 / 3 where this text was made, against
    HIST_S = 16 384 slots -- and a wave workgroup's four records of 4096 symbols fill the table to 80 % and more without crowding it."""
    t = M.text("crowded")
    qoff, qlen = M.lines(t)
    for level in (1, 2, 3, 4):
        for w in (0, 1):
            r = slice(w * M.HIST_T, (w + 1) * M.HIST_T)
            assert np.count_nonzero(O.qlt_histogram(t["fq"], qoff[r], qlen[r], level, 0, 1)) > M.HIST_S, (level, w)
    t = M.text("wave-uniform-8")
    qoff, qlen = M.lines(t)
    keys = np.count_nonzero(O.qlt_histogram(t["fq"], qoff[:4], np.minimum(qlen[:4], M.PRIOR_SYMBOLS), 3, 0, 1))
    assert M.HIST_S // 2 < keys < M.HIST_S, keys


def test_hot_text_has_a_key_past_the_harvest_and_the_memory_arm():
    t = M.text("hot")
    qoff, qlen = M.lines(t)
    for level in (1, 2, 3, 4):
        h = O.qlt_histogram(t["fq"], qoff[:M.HIST_T], qlen[:M.HIST_T], level, 0, 1)
        assert int(h.max()) >= 768 and np.count_nonzero(h) < M.HIST_S // 2, level


def test_tail_texts_end_where_they_say():
    seen = set()
    for name in M.TAILS:
        t = M.text(name)
        fq = t["fq"]
        starts, lens = util.line_table(fq)
        k, L = int(starts[-1]) % 4, int(lens[-1])
        assert name == "tail-%d-%d" % (k, L) and len(fq) == int(starts[-1]) + L + 1 and len(starts) == 4 * 13
        for step in (s * c for s in M.STEPS for c in M.SCALES):
            assert 12 % step == 0                            # record 12, the last, is sampled
        assert max(fq[int(starts[-1]):-1]) < 33 + 63          # no escape in the last line: a byte that is not read counts as one
        seen.add((k, L))
    assert seen == {(k, L) for k in range(4) for L in M.TAIL_LENS}
    # the last dword of the text is a part of one, with a symbol in it, in some of them: what the bytewise tail alone reads
    assert sum((k + L + 1) % 4 >= 2 for k, L in seen) == 12


def test_wave_texts_hold_every_length_and_escapes():
    for kind in ("uniform", "walk"):
        lens = set()
        for n in (5, 8, 9):
            t = M.text("wave-%s-%d" % (kind, n))
            qoff, qlen = M.lines(t)
            assert len(qlen) == n and len(t["fq"]) // n > 4000
            lens |= set(qlen.tolist())
        assert lens >= set(M.WAVE_LENS) and any(5000 <= L <= 9000 for L in lens)
    assert M.classes("wave-uniform-9")["escapes"] >= 1000 and M.classes("wave-walk-9")["escapes"] == 0
    c = M.classes("wave-drops-8")
    assert c["d3-early"] >= 2 and c["d3-late"] >= 2


@pytest.mark.parametrize("level", (1, 2, 3, 4))
def test_count_tables_are_scaled_by_the_shifts_they_name(level):
    tb = M.table(level)
    counts = tb["counts"].reshape(-1, 64)
    assert len(counts) == M.q_rows(level) and set(tb["kinds"].values()) == set(M.KINDS)
    assert {0, len(counts) - 1, 1023, 1024, 1025} <= set(tb["kinds"])
    rows = O.qlt_prior_rows(tb["counts"])
    for c, kind in tb["kinds"].items():
        mx, sh = int(counts[c].max()), tb["shifts"][c]
        f = rows[c, :64] & 0xffff
        assert int(f[0]) == (6 * mx) >> sh <= 32000 and (sh == 0 or (6 * mx) >> (sh - 1) > 32000), (c, kind)
        iend = int(rows[c, 65])
        assert iend == int(np.flatnonzero(counts[c])[-1]) + 1
        if kind == "zero-tail":                              # iend covers symbols of frequency 0, the highest seen among them
            assert f[:iend].tolist().count(0) == iend - 2 and int(rows[c, iend - 1] >> 16) == iend - 1
        if kind in ("two-largest", "three-largest", "all-equal"):
            n = {"two-largest": 2, "three-largest": 3, "all-equal": 64}[kind]
            assert len(set(f[:n].tolist())) == 1 and (n == 64 or f[n] < f[0]) and np.all(np.diff(rows[c, :n] >> 16) > 0)
        if kind == "only-0":
            assert iend == 1
        if kind == "only-63":
            assert iend == 64 and int(rows[c, 0] >> 16) == 63
    named = {k: tb["shifts"][c] for c, k in tb["kinds"].items()}
    assert [named["max:%d" % m] for m in (5333, 5334, 10666, 10667, 10668, 42667)] == [0, 1, 1, 2, 2, 3]
    at_32000 = [c for c, k in tb["kinds"].items() if k == "max:42667"]
    assert at_32000 and all(int(rows[c, 0] & 0xffff) == 32000 for c in at_32000)      # the largest frequency the rule gives, reached exactly
    # the ordinary text the rows are coded over starts every line in context 0, a chosen row
    assert M.legal(M.ordinary()) and 0 in tb["kinds"]


@pytest.mark.parametrize("level", (1, 3))
def test_row_families_have_the_floors_the_ties_and_the_correction(level):
    f = M.family(level)
    rows66, frozen = f["rows66"], f["frozen"]
    assert np.array_equal(util.unpack_prior(f["prior"], M.q_rows(level)), rows66)      # the canonical form: the blob gives the rows back
    first = {}
    for c in np.flatnonzero(rows66[:, 65]):
        first.setdefault(M.member_of(int(c)), int(c))
    assert set(first) == set(M.MEMBERS)
    x = lambda c: np.array([dict((int(s) >> 16, int(s) & 0xffff) for s in rows66[c, :int(rows66[c, 65])]).get(s, 0) + 1 for s in range(64)], np.uint64)
    for kind, c in first.items():
        g = (frozen[c] >> 16).astype(np.int64)
        assert int(g.sum()) == 65536 and np.array_equal(np.cumsum(g) - g, frozen[c] & 0xffff)
        floors = np.maximum(1, (x(c) << np.uint64(16)) // x(c).sum()).astype(np.int64)
        if kind.startswith("triple:"):
            assert int((g == 1).sum()) >= 60 and int(floors.sum()) > 65536 and int((floors == floors.max()).sum()) == 3
            lowest = min(int(s) for s in kind.split(":")[1:])
            assert g[lowest] == floors[lowest] - (int(floors.sum()) - 65536)          # the negative correction, to the first of the three
        if kind.startswith("limit:"):
            s = int(kind[6:])
            assert g[s] == 65473 and int((g == 1).sum()) == 63
        if kind == "all-32000":
            assert (g == 1024).all()
        if kind.startswith("spike:"):
            s = int(kind[6:])                                 # (32 001 of 32 064: the other 63 have floors of 2, cums two apart)
            assert (np.delete(g, s) == 2).all() and g[s] == floors[s] + 65536 - int(floors.sum()) == 65410
    unlisted = [c for c in range(len(rows66)) if M.member_of(c) is None]
    assert len(unlisted) >= len(rows66) // 18 and not rows66[unlisted, 65].any() and (frozen[unlisted] >> 16 == 1024).all()
    # rows whose neighbouring cums differ by 1: what the decoder's searches are walked through
    assert int(((frozen[list(first.values())] >> 16) == 1).sum()) >= 4 * 61 + 2 * 63


@pytest.mark.parametrize("level", (1, 3))
def test_family_text_meets_every_member_and_symbol(level):
    """(at level 1, where this text was made, every member is used 40 times or more for every symbol 1 .. 63; at level 3, 35 times)"""
    t = M.family_text()
    assert M.legal(t) and b"!" not in b"".join(t["fq"].split(b"\n")[3::4])
    uses = M.family_uses(level)
    assert uses[:, 1:].min() >= M.MIN, uses[:, 1:].min(axis=1)
    assert uses[:, 63].min() >= M.MIN                        # the escape, under every member
    f = M.family(level)
    qoff, qlen = M.lines(t)
    streams, sizes, extra = O.qlt_encode_chains(t["fq"], qoff, qlen, level, t["br"], t["cr"], f["frozen"])
    assert len(sizes) == 750 and extra == int(uses[:, 63].sum())
    back = O.qlt_decode_chains(streams, sizes, qoff, qlen, level, t["br"], t["cr"], f["frozen"])
    a = np.frombuffer(t["fq"], np.uint8)
    for o, n in zip(qoff[:50], qlen[:50]):
        assert back[int(o):int(o) + int(n)] == a[int(o):int(o) + int(n)].tobytes()

"""The dedup switch (sfq_ctx_set_dedup) behind every host decoder: a small archive with planted duplicates comes back without them by
the Python rule of test_dedup.py, behind the trim (test_trim.py's rule) and the selection (test_select.py's), in front of the merge
(test_merge.py's), the pair split, the pair window's split and the picks; installed checksums stay those of the decoded text; with
the context's set, calls on windows of blocks are one call on the whole.  Every comparison is exact byte equality."""
import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Dedup, Merge, Select, Trim
from test_dedup import distinct
from test_merge_decode import files, parts, split
from test_pairs import records, first_difference
from test_select import MODES, keep, picked
from test_trim import trimmed

pytestmark = pytest.mark.gpu
E_ARG = -1
PAIRS = 1200
PICKS = (capi.PICK_FASTA, capi.PICK_NAMES, capi.PICK_BASES, capi.PICK_QUALS)


@pytest.fixture
def dctx(ctx):
    """The session's context; afterwards no dedup, no set, no merge, no trim, no selection, no pick, no split, checksums off."""
    try:
        yield ctx
    finally:
        ctx.set_dedup(None)
        ctx.dedup_set_destroy()
        ctx.set_merge(None)
        ctx.set_trim(None)
        ctx.set_select(None)
        ctx.set_pick(0)
        ctx.set_pair_split(False)
        ctx.set_checksums(False)


_planted = []


def planted():
    """two files of 1200 reads of 60 bases: test_merge_decode's 600 pairs and 600 copies of some of them, shuffled; every third copy
    with the last base of its first mate changed -- no duplicate as it stands, one behind a trim of the last two bases"""
    if not _planted:
        a, b = files("mixed")
        ra, rb = records(a), records(b)
        rng = np.random.default_rng(77)
        order = [(i, False) for i in range(600)] + [(int(i), j % 3 == 0) for j, i in enumerate(rng.integers(0, 200, 600))]
        order = [order[int(i)] for i in rng.permutation(PAIRS)]
        fa, fb = [], []
        for i, changed in order:
            x = ra[i].split(b"\n")
            if changed:
                x[1] = x[1][:-1] + (b"A" if x[1][-1:] != b"A" else b"C")
            fa.append(b"\n".join(x))
            fb.append(rb[i])
        a, b = b"".join(fa), b"".join(fb)
        _planted.append((a, b, b"".join(x + y for x, y in zip(fa, fb))))
    return _planted[0]


def dd(fq, d=None, seen=None):
    """the text without its duplicates; seen: the set's keys, extended"""
    d = Dedup() if d is None else d
    kept, _, _, _, mine = distinct(fq, d, seen)
    if seen is not None:
        seen.update(mine)
    rs = records(fq)
    return b"".join(rs[r] for r in kept)


def fields(rep):
    return (rep.n_in_range, rep.n_units, rep.n_kept, rep.n_dup_set, rep.n_dup_call, rep.text_bytes, rep.kept_bytes)


def report(fq, d, seen=None):
    kept, units, in_set, in_call, _ = distinct(fq, d, seen)
    G = 2 if d.pairs else 1
    return (units * G, units, len(kept) // G, in_set, in_call, len(fq), sum(len(records(fq)[r]) for r in kept))


def test_records_behind_every_host_decoder(dctx):
    ctx = dctx
    fq = planted()[2]                                                 # the interleaved text, coded as records that stand alone
    rs = records(fq)
    ctx.set_checksums(True)                                           # the blocks' CRCs are installed: those of the decoded text
    enc = ctx.encode_host(fq, level=3, block_reads=100, **MODES["frozen"])
    ctx.set_checksums(False)
    assert len(enc.blocks) == 24 and len(enc.crcs) == 24
    cap = len(fq) + 4096
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_dedup() is None
    want = dd(fq)
    assert len(fq) // 3 < len(want) < 3 * len(fq) // 4
    ctx.set_dedup(Dedup())
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), want, "alone")
    assert fields(ctx.get_dedup()) == report(fq, Dedup()) and ctx.get_dedup().set_keys == 0
    # checksums on: they are those of the decoded text
    ctx.set_checksums(True)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), want, "with checksums")
    assert ctx.checksums() == (enc.crcs, enc.text_crc)
    ctx.set_checksums(False)
    # a window of blocks; the rule's range inside it
    window = b"".join(rs[200:700])
    got, _ = ctx.decode_range_host(enc, 2, 5, level=3, out_cap=cap)
    first_difference(got, dd(window), "blocks 2..+5")
    assert fields(ctx.get_dedup()) == report(window, Dedup())
    d = Dedup(first_record=50, n_records=300)
    ctx.set_dedup(d)
    got, _ = ctx.decode_range_host(enc, 2, 5, level=3, out_cap=cap)
    first_difference(got, dd(window, d), "records 50..+300 of blocks 2..+5")
    assert fields(ctx.get_dedup()) == report(window, d)
    # the context's set: windows of blocks, one behind the other, are the whole text
    ctx.dedup_set_create(len(rs), len(fq), 0)
    ctx.set_dedup(Dedup(use_set=True))
    seen, out = {}, b""
    for b0, n in ((0, 7), (7, 1), (8, 16)):
        part = b"".join(rs[100 * b0:100 * (b0 + n)])
        exp = report(part, Dedup(use_set=True), seen)
        got, _ = ctx.decode_range_host(enc, b0, n, level=3, out_cap=cap)
        first_difference(got, dd(part, Dedup(use_set=True), seen), "blocks %d..+%d into the set" % (b0, n))
        assert fields(ctx.get_dedup()) == exp and ctx.get_dedup().set_keys == len(seen)
        out += got
    assert out == want and exp[3] > 0
    assert ctx.decode_host(enc, level=3, out_cap=cap) == b"" and ctx.get_dedup().n_dup_set == len(rs)    # every key is known by now
    ctx.dedup_set_destroy()
    with pytest.raises(capi.SfqError) as e:                           # the rule asks for a set that is gone
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG
    # the picks behind
    ctx.set_dedup(Dedup())
    for w in PICKS:
        ctx.set_pick(w)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(want, w), "pick %d" % w)
        assert ctx.get_pick() == (w, len(want), len(records(want)))
    ctx.set_pick(0)
    # a trim and a selection in front: the dedup judges the trimmed keys of the records the selection kept
    t, s = Trim(tail=2), Select(motif=b"ACG", min_len=58)
    t_text = trimmed(fq, t)[0]
    chain = dd(keep(t_text, s))
    assert 0 < len(chain) and len(records(dd(t_text))) < len(records(want)) and chain != keep(trimmed(want, t)[0], s)
    ctx.set_trim(t)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), dd(t_text), "behind the trim")
    ctx.set_select(s)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), chain, "behind the trim and the selection")
    assert ctx.get_dedup().text_bytes == ctx.get_select().kept_bytes == len(keep(t_text, s))
    ctx.set_select(Select(min_len=1000))                              # ... one that keeps nothing: nothing is left to judge
    assert ctx.decode_host(enc, level=3, out_cap=cap) == b"" and ctx.get_dedup() is None
    ctx.set_select(None)
    ctx.set_trim(None)
    with pytest.raises(capi.SfqError) as e:
        ctx.set_dedup(Dedup(pairs=2))
    assert e.value.code == E_ARG
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), want, "the setting stayed")
    # off again: today's bytes
    ctx.set_dedup(None)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_dedup() is None


def test_pairs_behind_every_host_decoder(dctx):
    ctx = dctx
    a, b, inter = planted()
    rs = records(inter)
    ctx.set_checksums(True)
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=14, **MODES["frozen"])
    ctx.set_checksums(False)
    cap = len(inter) + 4096
    d = Dedup(pairs=1)
    want = dd(inter, d)
    assert 2 * 600 < len(records(want)) < 2 * 900 and want != dd(inter)
    ctx.set_dedup(d)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), want, "interleaved")
    assert fields(ctx.get_dedup()) == report(inter, d) and ctx.pair_split() is None
    wa, wb = split(want)
    ctx.set_pair_split(True)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), wa + wb, "split")
    assert ctx.pair_split() == (len(wa), len(records(want)) // 2)
    ctx.set_pick(capi.PICK_BASES)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(wa, capi.PICK_BASES) + picked(wb, capi.PICK_BASES), "split and picked")
    ctx.set_pick(0)
    ctx.set_pair_split(False)
    # a window of pairs: the entry supplies the range
    for first_pair, n in ((100, 400), (101, 30), (0, PAIRS)):
        win = dd(b"".join(rs[2 * first_pair:2 * (first_pair + n)]), d)
        first, second, _ = ctx.decode_pair_range_host(enc, first_pair, n, out_cap=cap)
        assert (first, second) == split(win), "pairs %d..+%d" % (first_pair, n)
        assert ctx.pair_split() == (len(first), len(records(win)) // 2)
        assert fields(ctx.get_dedup())[:5] == report(b"".join(rs[2 * first_pair:2 * (first_pair + n)]), d)[:5]
    # ... behind a selection of pairs, which has cut to the window
    s = Select(motif=b"ACGT", pairs=capi.SELECT_EITHER)
    ctx.set_select(s)
    win = dd(keep(b"".join(rs[200:1000]), s), d)
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 400, out_cap=cap)
    assert (first, second) == split(win) and 0 < len(win)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), dd(keep(inter, s), d), "behind a selection of pairs")
    ctx.set_select(None)
    # the merge behind: it sees the pairs that are left
    m = Merge(min_overlap=12)
    front, rest, rep = parts(want, m)
    assert 0 < len(front) and 0 < len(rest)
    ctx.set_merge(m)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), front + rest, "merged")
    assert ctx.get_merge()[0].n_pairs == len(records(want)) // 2 and ctx.get_merge()[1] == len(front)
    ra, rb = split(rest)
    ctx.set_pair_split(True)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), front + ra + rb, "merged and split")
    ctx.set_pair_split(False)
    p_front, p_rest, _ = parts(dd(b"".join(rs[200:1000]), d), m)
    pa, pb = split(p_rest)
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 400, out_cap=cap)
    assert (first, second) == (p_front + pa, pb)
    # refused at the decode call: duplicates by record where mates must stay in step; a range under the pair window
    ctx.set_dedup(Dedup())
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)                    # the merge is on
    assert e.value.code == E_ARG and "distinct records:" in str(e.value)
    ctx.set_merge(None)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), dd(inter), "by record: no pass behind that wants pairs")
    ctx.set_pair_split(True)
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG and "distinct records:" in str(e.value)
    ctx.set_pair_split(False)
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_pair_range_host(enc, 100, 400, out_cap=cap)
    assert e.value.code == E_ARG and "distinct records:" in str(e.value)
    for bad in (Dedup(pairs=1, first_record=2), Dedup(pairs=1, n_records=100)):
        ctx.set_dedup(bad)
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_pair_range_host(enc, 100, 400, out_cap=cap)
        assert e.value.code == E_ARG
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), dd(inter, Dedup(pairs=1, n_records=100)), "the other decoders take a range")
    # off again: today's bytes
    ctx.set_dedup(None)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == inter and ctx.get_dedup() is None
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 400, out_cap=cap)
    assert (first, second) == split(b"".join(rs[200:1000])) and ctx.get_dedup() is None

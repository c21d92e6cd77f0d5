"""The merge switch (sfq_ctx_set_merge) behind every host decoder: a small paired archive comes back as [merged part | rest] by the
Python rule of test_merge.py, behind the trim (test_trim.py's rule) and the selection (test_select.py's), in front of the pair split
and the pair window's split, which take the rest alone, and of the picks, which take either part; every boundary reported is that of
the result as handed back.  Every comparison is exact byte equality."""
import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Merge, Overlap, Select, Trim
from test_merge import fields, merged
from test_overlap import bases, mates, rec
from test_pairs import records, first_difference
from test_select import MODES, keep, picked
from test_trim import trimmed

pytestmark = pytest.mark.gpu
E_ARG = -1
PAIRS = 600
PICKS = (capi.PICK_FASTA, capi.PICK_NAMES, capi.PICK_BASES, capi.PICK_QUALS)


@pytest.fixture
def mctx(ctx):
    """The session's context; afterwards no merge, no overlap, no trim, no selection, no pick, no split, checksums off."""
    try:
        yield ctx
    finally:
        ctx.set_merge(None)
        ctx.set_overlap(None)
        ctx.set_trim(None)
        ctx.set_select(None)
        ctx.set_pick(0)
        ctx.set_pair_split(False)
        ctx.set_checksums(False)


_files = {}


def files(kind="mixed"):
    """two files of 600 reads of 60 bases.  mixed: the inserts uniform in [15, 140], two thirds merge; all: in [30, 100], every pair
    merges; none: the second mates are those of other fragments"""
    if kind not in _files:
        rng = np.random.default_rng({"mixed": 31, "all": 32, "none": 33}[kind])
        genome = bases(rng, 20000)
        lo, hi = (30, 101) if kind == "all" else (15, 141)
        a, b = [], []
        for i in range(PAIRS):
            ins = int(rng.integers(lo, hi))
            at = int(rng.integers(0, len(genome) - ins))
            x, y = mates(rng, genome[at:at + ins], 60, 60)
            if kind == "none":
                y = bases(rng, 60)
            a.append(rec(x, hdr=b"@p%d/1" % i))
            b.append(rec(y, hdr=b"@p%d/2" % i))
        _files[kind] = b"".join(a), b"".join(b)
    return _files[kind]


def split(fq):
    rs = records(fq)
    return b"".join(rs[0::2]), b"".join(rs[1::2])


def parts(text, m):
    """(the merged part, the rest, the report's fields) of the rule applied to a text"""
    res, rep, _, _ = merged(text, m)
    return res[:rep[5]], res[rep[5]:], rep


def in_window(rep, inter, block_reads, first_pair, n):
    """the report of a window's pairs as a pair window's decode gives it: text_bytes is the text of the blocks that hold the window"""
    b0, b1 = 2 * first_pair // block_reads, (2 * (first_pair + n) - 1) // block_reads
    return rep[:3] + (len(b"".join(records(inter)[b0 * block_reads:(b1 + 1) * block_reads])),) + rep[4:]


def encoded(ctx, kind, block_reads):
    a, b = files(kind)
    inter = b"".join(x + y for x, y in zip(records(a), records(b)))
    return ctx.encode_pairs_host(a, b, level=3, block_reads=block_reads, **MODES["frozen"]), inter


def test_the_switch_behind_every_host_decoder(mctx):
    ctx = mctx
    a, b = files()
    inter = b"".join(x + y for x, y in zip(records(a), records(b)))
    ctx.set_checksums(True)                                           # the blocks' CRCs are installed: those of the decoded text
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=14, **MODES["frozen"])
    ctx.set_checksums(False)
    cap = len(inter) + 4096
    assert ctx.decode_host(enc, level=3, out_cap=cap) == inter and ctx.get_merge() is None
    m = Merge(min_overlap=12)
    front, rest, rep = parts(inter, m)
    assert rep[0] == PAIRS and min(rep[2], rep[0] - rep[2]) > PAIRS // 5 and 0 < len(front) < len(front) + len(rest) < len(inter)
    # alone, through each of the three entries
    ctx.set_merge(m)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), front + rest, "alone")
    got, size = ctx.get_merge()
    assert fields(got) == rep and size == len(front) and ctx.pair_split() is None
    w_front, w_rest, w_rep = parts(b"".join(records(inter)[14:56]), m)
    got, _ = ctx.decode_range_host(enc, 1, 3, level=3, out_cap=cap)
    first_difference(got, w_front + w_rest, "blocks 1..+3")
    assert fields(ctx.get_merge()[0]) == w_rep and ctx.get_merge()[1] == len(w_front)
    p_front, p_rest, p_rep = parts(b"".join(records(inter)[200:300]), m)
    pa, pb = split(p_rest)
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 50, out_cap=cap)
    first_difference(first, p_front + pa, "a window of pairs, the merged part and the first mates")
    first_difference(second, pb, "a window of pairs, second mates")
    assert fields(ctx.get_merge()[0]) == in_window(p_rep, inter, 14, 100, 50) and ctx.get_merge()[1] == len(p_front) and p_rep[0] == 50
    assert ctx.pair_split() == (len(p_front) + len(pa), 50 - p_rep[2])
    # with the pair split: of the rest alone, its boundary lies behind the merged part
    ra, rb = split(rest)
    ctx.set_pair_split(True)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), front + ra + rb, "split")
    assert ctx.pair_split() == (len(front) + len(ra), PAIRS - rep[2]) and ctx.get_merge()[1] == len(front)
    # with each pick: of either part, the boundaries are those of the picked result
    for what in PICKS:
        ctx.set_pick(what)
        pf = picked(front, what)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), pf + picked(ra, what) + picked(rb, what), "split and picked %d" % what)
        assert ctx.pair_split() == (len(pf) + len(picked(ra, what)), PAIRS - rep[2]) and ctx.get_merge()[1] == len(pf)
        assert ctx.get_pick() == (what, len(front) + len(rest), PAIRS + PAIRS - rep[2])
    ctx.set_pair_split(False)
    for what in PICKS:
        ctx.set_pick(what)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(front, what) + picked(rest, what), "picked %d" % what)
        assert ctx.get_merge()[1] == len(picked(front, what)) and ctx.pair_split() is None
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 50, out_cap=cap)
    assert (first, second) == (picked(p_front, what) + picked(pa, what), picked(pb, what))
    assert ctx.get_merge()[1] == len(picked(p_front, what))
    ctx.set_pick(0)
    # a trim in front: the merge sees the trimmed mates
    t = Trim(tail=2)
    t_text = trimmed(inter, t)[0]
    t_front, t_rest, t_rep = parts(t_text, m)
    assert t_front != front
    ctx.set_trim(t)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), t_front + t_rest, "behind the trim")
    assert fields(ctx.get_merge()[0]) == t_rep
    ctx.set_trim(None)
    # a selection of pairs in front: it judges the mates
    s = Select(motif=b"ACGT", pairs=capi.SELECT_EITHER)
    kept = keep(inter, s)
    assert 0 < len(kept) < len(inter)
    s_front, s_rest, s_rep = parts(kept, m)
    ctx.set_select(s)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), s_front + s_rest, "behind a selection")
    assert fields(ctx.get_merge()[0]) == s_rep and ctx.get_select().kept_bytes == len(kept)
    k_front, k_rest, k_rep = parts(keep(b"".join(records(inter)[200:300]), s), m)
    ka, kb = split(k_rest)
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 50, out_cap=cap)
    assert (first, second) == (k_front + ka, kb) and fields(ctx.get_merge()[0]) == k_rep
    ctx.set_select(Select(min_len=1000, pairs=capi.SELECT_BOTH))      # ... one that keeps nothing: nothing is left to merge
    assert ctx.decode_host(enc, level=3, out_cap=cap) == b"" and ctx.get_merge() is None
    # refused at the decode call: a selection of single records, the overlap switch as well, a range under the pair window
    ctx.set_select(Select(min_len=10))
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG and "merged mates:" in str(e.value)
    ctx.set_select(None)
    ctx.set_overlap(Overlap(min_overlap=12))
    for call in (lambda: ctx.decode_host(enc, level=3, out_cap=cap), lambda: ctx.decode_range_host(enc, 1, 3, level=3, out_cap=cap),
                 lambda: ctx.decode_pair_range_host(enc, 100, 50, out_cap=cap)):
        with pytest.raises(capi.SfqError) as e:
            call()
        assert e.value.code == E_ARG and "merged mates:" in str(e.value)
    ctx.set_overlap(None)
    for bad in (Merge(first_record=2, min_overlap=12), Merge(n_records=100, min_overlap=12)):
        ctx.set_merge(bad)
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_pair_range_host(enc, 100, 50, out_cap=cap)
        assert e.value.code == E_ARG
    got = ctx.decode_host(enc, level=3, out_cap=cap)                   # ... while the other decoders take it: what lies outside is dropped
    assert got == merged(inter, Merge(n_records=100, min_overlap=12))[0] and len(got) < len(inter) // 4
    with pytest.raises(capi.SfqError) as e:
        ctx.set_merge(Merge(qual_base=32))
    assert e.value.code == E_ARG
    # off again: today's bytes
    ctx.set_merge(None)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == inter and ctx.get_merge() is None
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 50, out_cap=cap)
    assert (first, second) == split(b"".join(records(inter)[200:300])) and ctx.get_merge() is None


def test_a_window_whose_first_pair_is_an_odd_record_of_its_blocks(mctx):
    ctx = mctx
    enc, inter = encoded(ctx, "mixed", 15)
    cap = len(inter) + 4096
    m = Merge(min_overlap=12)
    rs = records(inter)
    ctx.set_merge(m)
    for first_pair, n in ((8, 7), (8, 40), (23, 1)):                   # records 16, 46: the second records of blocks 1 and 3
        assert (2 * first_pair) % 15 % 2 == 1
        front, rest, rep = parts(b"".join(rs[2 * first_pair:2 * (first_pair + n)]), m)
        ra, rb = split(rest)
        first, second, _ = ctx.decode_pair_range_host(enc, first_pair, n, out_cap=cap)
        first_difference(first, front + ra, "pairs %d..+%d, the merged part and the first mates" % (first_pair, n))
        first_difference(second, rb, "pairs %d..+%d, second mates" % (first_pair, n))
        assert fields(ctx.get_merge()[0]) == in_window(rep, inter, 15, first_pair, n) and ctx.get_merge()[1] == len(front) and rep[0] == n
    # a window of blocks that begins at an odd record: the range says where the pairs begin, the records outside it are dropped
    ctx.set_merge(Merge(first_record=1, n_records=28, min_overlap=12))
    got, _ = ctx.decode_range_host(enc, 1, 2, level=3, out_cap=cap)
    assert got == merged(b"".join(rs[16:44]), m)[0]


@pytest.mark.parametrize("kind", ["all", "none"])
def test_an_empty_part_is_skipped_by_the_split_and_the_pick(mctx, kind):
    ctx = mctx
    enc, inter = encoded(ctx, kind, 64)
    cap = len(inter) + 4096
    m = Merge(min_overlap=20)
    front, rest, rep = parts(inter, m)
    assert rep[2] == (PAIRS if kind == "all" else 0) and (rest == b"" if kind == "all" else (front == b"" and rest == inter))
    ra, rb = split(rest) if rest else (b"", b"")
    ctx.set_merge(m)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), front + rest, "alone")
    assert ctx.get_merge()[1] == len(front)
    ctx.set_pair_split(True)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), front + ra + rb, "split")
    assert ctx.pair_split() == (len(front) + len(ra), PAIRS - rep[2])
    first, second, _ = ctx.decode_pair_range_host(enc, 10, 20, out_cap=cap)
    w_front, w_rest, _ = parts(b"".join(records(inter)[20:60]), m)
    wa, wb = split(w_rest) if w_rest else (b"", b"")
    assert (first, second) == (w_front + wa, wb)
    ctx.set_pick(capi.PICK_BASES)
    want = picked(front, capi.PICK_BASES) + picked(ra, capi.PICK_BASES) + picked(rb, capi.PICK_BASES)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), want, "split and picked")
    assert ctx.get_merge()[1] == len(picked(front, capi.PICK_BASES))
    assert ctx.pair_split() == (len(picked(front, capi.PICK_BASES)) + len(picked(ra, capi.PICK_BASES)), PAIRS - rep[2])

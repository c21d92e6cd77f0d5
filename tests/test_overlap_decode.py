"""The overlap switch (sfq_ctx_set_overlap) behind every host decoder: a small paired archive comes back with the read-through cut by
the Python rule of test_overlap.py, behind the trim (test_trim.py's rule) and in front of the selection, the pair split, the pair
window and the picks (test_select.py's rules); installed checksums stay those of the decoded text.  Every comparison is exact byte
equality."""
import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Overlap, Select, Trim
from test_overlap import bases, bases_of, fields, mates, overlapped, rec
from test_pairs import records, first_difference
from test_select import MODES, keep, picked
from test_trim import trimmed

pytestmark = pytest.mark.gpu
E_ARG = -1
PAIRS = 600


@pytest.fixture
def octx(ctx):
    """The session's context; afterwards no overlap, no trim, no selection, no pick, no split, checksums off."""
    try:
        yield ctx
    finally:
        ctx.set_overlap(None)
        ctx.set_trim(None)
        ctx.set_select(None)
        ctx.set_pick(0)
        ctx.set_pair_split(False)
        ctx.set_checksums(False)


_files = {}


def files():
    """two files of 600 reads of 60 bases, the inserts uniform in [15, 140]: a third cut, a third overlapping, a third apart"""
    if not _files:
        rng = np.random.default_rng(31)
        genome = bases(rng, 20000)
        a, b = [], []
        for i in range(PAIRS):
            ins = int(rng.integers(15, 141))
            at = int(rng.integers(0, len(genome) - ins))
            x, y = mates(rng, genome[at:at + ins], 60, 60)
            a.append(rec(x, hdr=b"@p%d/1" % i))
            b.append(rec(y, hdr=b"@p%d/2" % i))
        _files["a"], _files["b"] = b"".join(a), b"".join(b)
    return _files["a"], _files["b"]


def split(fq):
    rs = records(fq)
    return b"".join(rs[0::2]), b"".join(rs[1::2])


def test_the_switch_behind_every_host_decoder(octx):
    ctx = octx
    a, b = files()
    inter = b"".join(x + y for x, y in zip(records(a), records(b)))
    ctx.set_checksums(True)                                           # the blocks' CRCs are installed: those of the uncut text
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=14, **MODES["frozen"])
    ctx.set_checksums(False)
    cap = len(inter) + 4096
    assert ctx.decode_host(enc, level=3, out_cap=cap) == inter and ctx.get_overlap() is None
    o = Overlap(min_overlap=12)
    want, rep, wins = overlapped(inter, o)
    assert rep[0] == PAIRS and min(rep[3], rep[2] - rep[3], rep[9][0]) > PAIRS // 6 and len(want) < len(inter)
    # alone
    ctx.set_overlap(o)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), want, "alone")
    assert fields(ctx.get_overlap()) == rep
    window = b"".join(records(inter)[14:56])
    w_want, w_rep, _ = overlapped(window, o)
    got, _ = ctx.decode_range_host(enc, 1, 3, level=3, out_cap=cap)
    first_difference(got, w_want, "blocks 1..+3")
    assert fields(ctx.get_overlap()) == w_rep
    wa, wb = split(b"".join(records(want)[200:300]))
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 50, out_cap=cap)
    first_difference(first, wa, "a window of pairs, first mates")
    first_difference(second, wb, "a window of pairs, second mates")
    got = ctx.get_overlap()
    assert got.n_pairs == 50 and got.n_cut == sum(w is not None and w[0] < 0 for w in wins[100:150])
    # counted only: the text stays, the report is the cutting run's but for the two sizes
    ctx.set_overlap(Overlap(min_overlap=12, cut=0))
    assert ctx.decode_host(enc, level=3, out_cap=cap) == inter
    got = fields(ctx.get_overlap())
    assert got[:5] == rep[:5] and got[5:8] == (len(inter), rep[6], rep[6]) and got[8:] == rep[8:]
    ctx.set_overlap(o)
    # behind a trim and in front of a selection on the length: a pair cut below the bound is dropped
    t = Trim(tail=2)
    trimmed_text = trimmed(inter, t)[0]
    t_want, t_rep, _ = overlapped(trimmed_text, o)
    s = Select(min_len=40, pairs=capi.SELECT_BOTH)
    kept = keep(t_want, s)
    assert 0 < len(kept) < len(t_want) and keep(trimmed_text, s) == trimmed_text and t_want != want
    ctx.set_trim(t)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), t_want, "behind the trim")
    assert fields(ctx.get_overlap()) == t_rep
    ctx.set_select(s)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), kept, "behind the trim, in front of the selection")
    assert ctx.get_select().text_bytes == len(t_want)
    ka, kb = split(kept)
    ctx.set_pair_split(True)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), ka + kb, "trimmed, cut, selected and split")
    ctx.set_select(None)
    ctx.set_trim(None)
    # with the pair split, with a pick
    xa, xb = split(want)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), xa + xb, "split")
    assert ctx.pair_split() == (len(xa), PAIRS)
    ctx.set_pick(capi.PICK_BASES)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(xa, capi.PICK_BASES) + picked(xb, capi.PICK_BASES), "split and picked")
    ctx.set_pair_split(False)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(want, capi.PICK_BASES), "the cut base lines")
    ctx.set_pick(capi.PICK_FASTA)
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 50, out_cap=cap)
    assert (first, second) == (picked(wa, capi.PICK_FASTA), picked(wb, capi.PICK_FASTA))
    ctx.set_pick(0)
    # a window of pairs is the range: a rule with a range of its own is refused
    for bad in (Overlap(first_record=2, min_overlap=12), Overlap(n_records=100, min_overlap=12)):
        ctx.set_overlap(bad)
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_pair_range_host(enc, 100, 50, out_cap=cap)
        assert e.value.code == E_ARG
    got = ctx.decode_host(enc, level=3, out_cap=cap)                   # ... while the other decoders take it
    assert got == overlapped(inter, Overlap(n_records=100, min_overlap=12))[0]
    with pytest.raises(capi.SfqError) as e:
        ctx.set_overlap(Overlap(min_overlap=0))
    assert e.value.code == E_ARG
    # off again: today's bytes
    ctx.set_overlap(None)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == inter and ctx.get_overlap() is None
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 50, out_cap=cap)
    assert (first, second) == split(b"".join(records(inter)[200:300])) and ctx.get_overlap() is None


def test_a_window_whose_first_pair_is_an_odd_record_of_its_blocks(octx):
    ctx = octx
    a, b = files()
    inter = b"".join(x + y for x, y in zip(records(a), records(b)))
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=15, **MODES["frozen"])
    cap = len(inter) + 4096
    o = Overlap(min_overlap=12)
    want = records(overlapped(inter, o)[0])
    ctx.set_overlap(o)
    for first_pair, n in ((8, 7), (8, 40), (23, 1)):                   # records 16, 46: the second records of blocks 1 and 3
        assert (2 * first_pair) % 15 % 2 == 1
        wa, wb = split(b"".join(want[2 * first_pair:2 * (first_pair + n)]))
        first, second, _ = ctx.decode_pair_range_host(enc, first_pair, n, out_cap=cap)
        first_difference(first, wa, "pairs %d..+%d, first mates" % (first_pair, n))
        first_difference(second, wb, "pairs %d..+%d, second mates" % (first_pair, n))
        assert ctx.get_overlap().n_pairs == n
    # a window of blocks that begins at an odd record: the range says where the pairs begin
    got_plain, _ = ctx.decode_range_host(enc, 1, 2, level=3, out_cap=cap)
    ctx.set_overlap(Overlap(first_record=1, n_records=28, min_overlap=12))
    got, _ = ctx.decode_range_host(enc, 1, 2, level=3, out_cap=cap)
    assert got == b"".join(records(inter)[15:16] + want[16:44] + records(inter)[44:45]) and got != got_plain

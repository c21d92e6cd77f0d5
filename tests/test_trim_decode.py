"""The trim switch (sfq_ctx_set_trim) behind every host decoder: the text comes back trimmed by the Python rule of test_trim.py, in
front of the selection, the pair split, the pair window and the picks, whose Python rules (test_select.py) are composed behind it;
installed checksums stay those of the decoded text.  Every comparison is exact byte equality."""
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Select, Trim
from test_pairs import records, reads, first_difference
from test_select import MODES, keep, picked
from test_trim import ADAPTER, bases_of, fields, trimmed

pytestmark = pytest.mark.gpu
E_ARG, E_FORMAT = -1, -4
RULE = dict(head=3, tail=2, lead_q=35, trail_q=15, win_len=5, win_q_x100=2600, adapter=ADAPTER[:13], adapter_mm=1, adapter_min=3)


@pytest.fixture
def tctx(ctx):
    """The session's context; afterwards no trim, no selection, no pick, no split, checksums off."""
    try:
        yield ctx
    finally:
        ctx.set_trim(None)
        ctx.set_select(None)
        ctx.set_pick(0)
        ctx.set_pair_split(False)
        ctx.set_checksums(False)


FORMATS = dict(MODES, format6=dict(block_reads=0))


@pytest.mark.parametrize("mode", sorted(FORMATS))
def test_the_switch_behind_decode_host(tctx, mode):
    ctx = tctx
    fq = capi.synth_fastq(300 if mode == "format6" else 1500, 100, seed=41)
    ctx.set_checksums(True)                                           # decode_host installs the blocks' CRCs: those of the untrimmed text
    enc = ctx.encode_host(fq, **dict(dict(level=3, block_reads=256), **FORMATS[mode]))
    ctx.set_checksums(False)
    assert len(enc.crcs) == len(enc.blocks)
    cap = len(fq) + 4096
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_trim() is None
    t = Trim(**RULE)
    want, rep = trimmed(fq, t)
    assert 0 < rep[1] and 0 < len(want) < len(fq) and all(rep[7])
    ctx.set_trim(t)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), want, mode)
    assert fields(ctx.get_trim()) == rep
    # the selection judges the trimmed length: a bound between the two lengths
    lens = sorted(len(b) for b in bases_of(want))
    bound = lens[len(lens) // 2] + 1
    assert lens[0] < bound <= lens[-1] < 100
    s = Select(min_len=bound, max_n=2)
    ctx.set_select(s)
    kept = keep(want, s)
    assert 0 < len(kept) < len(want) and keep(fq, s) != kept
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), kept, mode + ", selected")
    assert ctx.get_select().text_bytes == len(want) and fields(ctx.get_trim()) == rep
    for w in (capi.PICK_FASTA, capi.PICK_NAMES, capi.PICK_BASES, capi.PICK_QUALS):
        ctx.set_pick(w)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(kept, w), "%s, selected, pick %d" % (mode, w))
    ctx.set_select(None)
    ctx.set_pick(capi.PICK_BASES)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(want, capi.PICK_BASES), mode + ", the trimmed base lines")
    assert ctx.get_pick() == (capi.PICK_BASES, len(want), rep[0])
    ctx.set_pick(0)
    # everything cut to nothing: the records keep their lines, and a selection on the length drops them all
    ctx.set_trim(Trim(max_len=0))
    got = ctx.decode_host(enc, level=3, out_cap=cap)
    assert got == trimmed(fq, Trim(max_len=0))[0] and got.count(b"\n") == fq.count(b"\n")
    ctx.set_select(Select(min_len=1))
    assert ctx.decode_host(enc, level=3, out_cap=cap) == b"" and ctx.get_select().n_kept == 0
    ctx.set_select(None)
    with pytest.raises(capi.SfqError) as e:
        ctx.set_trim(Trim(win_len=40))
    assert e.value.code == E_ARG
    ctx.set_trim(None)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_trim() is None


def test_a_damaged_checksum_is_found_in_front_of_the_trim(tctx):
    ctx = tctx
    fq = capi.synth_fastq(600, 100, seed=42)
    ctx.set_checksums(True)
    enc = ctx.encode_host(fq, level=3, block_reads=256, **MODES["frozen"])
    ctx.set_checksums(False)
    ctx.set_trim(Trim(**RULE))
    enc.crcs[1] ^= 1
    with pytest.raises(capi.SfqError):
        ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096)
    enc.crcs[1] ^= 1
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == trimmed(fq, Trim(**RULE))[0]


def test_the_switch_behind_a_window_of_blocks(tctx):
    ctx = tctx
    fq = capi.synth_fastq(1500, 100, seed=43)
    rs = records(fq)
    ctx.set_checksums(True)
    enc = ctx.encode_host(fq, level=3, block_reads=256, **MODES["frozen"])
    ctx.set_checksums(False)
    cap = len(fq) + 4096
    window = b"".join(rs[256:1024])
    t = Trim(**RULE)
    want, rep = trimmed(window, t)
    ctx.set_trim(t)
    got, _ = ctx.decode_range_host(enc, 1, 3, level=3, out_cap=cap)
    first_difference(got, want, "blocks 1..+3")
    assert fields(ctx.get_trim()) == rep
    s = Select(first_record=10, n_records=700, min_len=60, index_base=256, sample=0xC0000000, sample_seed=3)
    ctx.set_select(s)
    got, _ = ctx.decode_range_host(enc, 1, 3, level=3, out_cap=cap)
    first_difference(got, keep(want, s), "blocks 1..+3, a range of records selected")
    ctx.set_select(None)
    ctx.set_trim(None)
    assert ctx.decode_range_host(enc, 1, 3, level=3, out_cap=cap)[0] == window and ctx.get_trim() is None


def test_the_switch_with_pairs(tctx):
    ctx = tctx
    a, b = reads(900, 30, 60, seed=21), reads(900, 30, 60, seed=22)
    ra, rb = records(a), records(b)
    inter = b"".join(x + y for x, y in zip(ra, rb))
    ctx.set_checksums(True)
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=14, **MODES["frozen"])
    ctx.set_checksums(False)
    cap = len(inter) + 4096
    t = Trim(head=1, trail_q=40, win_len=4, win_q_x100=3000, adapter=ADAPTER[:13])
    ta, tb, ti = trimmed(a, t)[0], trimmed(b, t)[0], trimmed(inter, t)[0]
    assert len(ti) < len(inter)
    ctx.set_trim(t)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), ti, "interleaved")
    ctx.set_pair_split(True)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), ta + tb, "split")
    assert ctx.pair_split() == (len(ta), 900)
    ctx.set_pick(capi.PICK_QUALS)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(ta, capi.PICK_QUALS) + picked(tb, capi.PICK_QUALS), "split and picked")
    ctx.set_pick(0)
    # a selection of pairs on the trimmed lengths, then the split
    s = Select(min_len=20, pairs=capi.SELECT_BOTH)
    ctx.set_select(s)
    kept = records(keep(ti, s))
    assert 0 < len(kept) < 1800
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), b"".join(kept[0::2]) + b"".join(kept[1::2]), "selected and split")
    ctx.set_select(None)
    ctx.set_pair_split(False)
    # a window of pairs: trimmed, then cut to the pairs and split
    wa, wb = trimmed(b"".join(ra[300:500]), t)[0], trimmed(b"".join(rb[300:500]), t)[0]
    first, second, _ = ctx.decode_pair_range_host(enc, 300, 200, out_cap=cap)
    first_difference(first, wa, "a window of pairs, first mates")
    first_difference(second, wb, "a window of pairs, second mates")
    assert ctx.pair_split() == (len(wa), 200) and ctx.get_trim().n_records >= 400
    ctx.set_pick(capi.PICK_FASTA)
    first, second, _ = ctx.decode_pair_range_host(enc, 300, 200, out_cap=cap)
    assert (first, second) == (picked(wa, capi.PICK_FASTA), picked(wb, capi.PICK_FASTA))
    ctx.set_pick(0)
    ctx.set_trim(None)
    first, second, _ = ctx.decode_pair_range_host(enc, 300, 200, out_cap=cap)
    assert (first, second) == (b"".join(ra[300:500]), b"".join(rb[300:500])) and ctx.get_trim() is None

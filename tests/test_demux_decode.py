"""The demux switch (sfq_ctx_set_demux) behind the host decoders: a small archive comes back partitioned by sample, by the Python rule of
demux_rule.py applied to the decoded text; alone, behind the trim, the selection and the dedup, as the call's last pass; the refusals
at the decode call; sfq_get_demux before and after.  Every comparison is exact byte equality."""
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Dedup, Demux, DemuxPart, Merge, Select, Trim, DEMUX_BASES as B
from demux_rule import demux
from test_dedup_decode import dd, planted
from test_pairs import records, first_difference
from test_select import MODES, keep
from test_trim import trimmed

pytestmark = pytest.mark.gpu
E_ARG = -1
ROWS = [b"ACG", b"TTA", b"GGC", b"CAT", b"AAA"]


@pytest.fixture
def xctx(ctx):
    """The session's context; afterwards no demux, no dedup, no merge, no trim, no selection, no pick, no split."""
    try:
        yield ctx
    finally:
        ctx.set_demux(None)
        ctx.set_dedup(None)
        ctx.set_merge(None)
        ctx.set_trim(None)
        ctx.set_select(None)
        ctx.set_pick(0)
        ctx.set_pair_split(False)


def rule_of(max_mm=0, **kw):
    return Demux([DemuxPart(B, 0, 0, 1, 3)], n_samples=len(ROWS), max_mm=max_mm, **kw)


def same(ctx, got, text, rule, what):
    """the bytes handed back and sfq_get_demux against the rule applied to text"""
    parts, units, c = demux(text, rule, ROWS)
    first_difference(got, b"".join(parts), what)
    rep, off, got_units = ctx.get_demux()
    assert off == [sum(len(p) for p in parts[:i]) for i in range(len(parts) + 1)], what
    assert got_units == units, what
    assert (rep.n_in_range, rep.n_units, rep.n_assigned, rep.n_perfect, rep.n_short, rep.n_far, rep.n_ambiguous, rep.text_bytes, rep.out_bytes,
            rep.bases_clipped) == (c["n_in_range"], c["n_units"], c["n_assigned"], c["n_perfect"], c["n_short"], c["n_far"], c["n_ambiguous"],
                                   len(text), c["out_bytes"], c["bases_clipped"]), what
    return c


def test_records_behind_the_host_decoders(xctx):
    ctx = xctx
    fq = planted()[2]
    rs = records(fq)
    enc = ctx.encode_host(fq, level=3, block_reads=100, **MODES["frozen"])
    cap = len(fq) + 4096
    before = ctx.decode_host(enc, level=3, out_cap=cap)
    assert before == fq and ctx.get_demux() is None
    for rule in (rule_of(), rule_of(clip=1), rule_of(max_mm=1), rule_of(first_record=50, n_records=1000)):
        ctx.set_demux(rule, ROWS)
        c = same(ctx, ctx.decode_host(enc, level=3, out_cap=cap), fq, rule, "alone")
        assert 0 < c["n_assigned"] < c["n_units"]
    # a window of blocks; the rule's range inside it
    window = b"".join(rs[200:700])
    for rule in (rule_of(), rule_of(first_record=50, n_records=300, clip=1)):
        ctx.set_demux(rule, ROWS)
        got, _ = ctx.decode_range_host(enc, 2, 5, level=3, out_cap=cap)
        same(ctx, got, window, rule, "blocks 2..+5")
    # THE ORDER: the trim, the selection, the dedup, the demux: it sorts the trimmed records that the selection and the dedup kept
    t, s = Trim(head=1), Select(motif=b"ACG", min_len=58)
    chain = dd(keep(trimmed(fq, t)[0], s))
    assert 0 < len(chain) < len(fq)
    ctx.set_trim(t)
    ctx.set_select(s)
    ctx.set_dedup(Dedup())
    rule = Demux([DemuxPart(B, 0, 0, 0, 3)], n_samples=len(ROWS), max_mm=0)          # the trim took the first base
    ctx.set_demux(rule, ROWS)
    same(ctx, ctx.decode_host(enc, level=3, out_cap=cap), chain, rule, "behind the trim, the selection and the dedup")
    assert ctx.get_demux()[0].text_bytes == ctx.get_dedup().kept_bytes
    # a selection that keeps nothing: nothing is left to sort
    ctx.set_select(Select(min_len=1000))
    assert ctx.decode_host(enc, level=3, out_cap=cap) == b"" and ctx.get_demux() is None
    ctx.set_select(None)
    ctx.set_trim(None)
    ctx.set_dedup(None)
    # refused: the pick
    ctx.set_demux(rule_of(), ROWS)
    ctx.set_pick(capi.PICK_FASTA)
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG and "demultiplexed records:" in str(e.value) and "pick" in str(e.value)
    ctx.set_pick(0)
    # a rule that the check refuses: the setting stays
    with pytest.raises(capi.SfqError) as e:
        ctx.set_demux(rule_of(pairs=2), ROWS)
    assert e.value.code == E_ARG
    same(ctx, ctx.decode_host(enc, level=3, out_cap=cap), fq, rule_of(), "the setting stays")
    # off again: the bytes handed back before
    ctx.set_demux(None)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == before and ctx.get_demux() is None


def test_pairs_behind_the_host_decoders(xctx):
    ctx = xctx
    a, b, inter = planted()
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=14, **MODES["frozen"])
    cap = len(inter) + 4096
    p = [DemuxPart(B, 0, 0, 1, 2), DemuxPart(B, 1, 0, 0, 1)]
    for split in (0, 1):
        rule = Demux(p, n_samples=len(ROWS), max_mm=0, pairs=1, split_mates=split, clip=split)
        ctx.set_demux(rule, ROWS)
        c = same(ctx, ctx.decode_host(enc, level=3, out_cap=cap), inter, rule, "pairs, split %d" % split)
        assert 0 < c["n_assigned"] < c["n_units"]
    # behind a dedup of pairs
    ctx.set_dedup(Dedup(pairs=1))
    same(ctx, ctx.decode_host(enc, level=3, out_cap=cap), dd(inter, Dedup(pairs=1)), rule, "behind the dedup of pairs")
    # refused: pairs out of step with a pass in front, either way round
    ctx.set_dedup(Dedup())
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG and "demultiplexed records:" in str(e.value) and "dedup" in str(e.value)
    ctx.set_dedup(None)
    ctx.set_select(Select(motif=b"ACGT"))
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG and "selection" in str(e.value)
    ctx.set_select(Select(motif=b"ACGT", pairs=capi.SELECT_EITHER))
    ctx.set_demux(rule_of(), ROWS)
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG and "selection" in str(e.value)
    ctx.set_select(None)
    # refused: the merge, the pair split, a window of pairs
    ctx.set_demux(rule, ROWS)
    ctx.set_merge(Merge(min_overlap=12))
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG and "demultiplexed records:" in str(e.value) and "merge" in str(e.value)
    ctx.set_merge(None)
    ctx.set_pair_split(True)
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG and "pair split" in str(e.value) and "split_mates" in str(e.value)
    ctx.set_pair_split(False)
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_pair_range_host(enc, 100, 400, out_cap=cap)
    assert e.value.code == E_ARG and "window of pairs" in str(e.value)
    # off again: the bytes handed back before
    ctx.set_demux(None)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == inter and ctx.get_demux() is None

"""The BGZF switch (sfq_ctx_set_bgzf) behind the host decoders: a small archive comes back as BGZF bytes that inflate to what the plain
call returns -- one text, the pair split and a pair window (two parts at the split), the pick, the merge, the demultiplexing (every
part inflates to the plain call's part), a selection that keeps nothing; the switch off again; sfq_get_bgzf before and after."""
import gzip
import os

import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Demux, DemuxPart, Merge, Select, DEMUX_BASES as B
import bgzf_check
from test_pairs import reads, records
from test_select import MODES

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROWS = [b"ACG", b"TTA", b"GGC", b"CAT", b"AAA"]


@pytest.fixture
def zctx(ctx):
    try:
        yield ctx
    finally:
        ctx.set_bgzf(False)
        ctx.set_demux(None)
        ctx.set_merge(None)
        ctx.set_select(None)
        ctx.set_pick(0)
        ctx.set_pair_split(False)


def parts_of(ctx, got, plain_parts):
    """got as BGZF whose parts inflate to plain_parts; sfq_get_bgzf agrees"""
    rep, off, text = ctx.get_bgzf()
    assert len(off) == len(plain_parts) + 1 and off[0] == 0 and off[-1] == len(got) == rep.out_bytes
    assert text == [len(p) for p in plain_parts] and rep.text_bytes == sum(text)
    assert bgzf_check.check(got, off) == b"".join(plain_parts)
    for i, p in enumerate(plain_parts):
        assert bgzf_check.check(got[off[i]:off[i + 1]]) == p, "part %d" % i
    return off


def test_one_text(zctx):
    ctx = zctx
    fq = gzip.open(os.path.join(GOLDEN, "small.fq.gz")).read()
    enc = ctx.encode_host(fq, level=3, block_reads=100, **MODES["frozen"])
    cap = len(fq) + 4096
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_bgzf() is None
    ctx.set_bgzf(True)
    got = ctx.decode_host(enc, level=3, out_cap=cap)
    assert len(got) < len(fq) / 2
    parts_of(ctx, got, [fq])
    win, _ = ctx.decode_range_host(enc, 1, 2, level=3, out_cap=cap)
    parts_of(ctx, win, [b"".join(records(fq)[100:300])])
    # the pick
    ctx.set_pick(capi.PICK_BASES)
    got = ctx.decode_host(enc, level=3, out_cap=cap)
    parts_of(ctx, got, [b"".join(r.split(b"\n")[1] + b"\n" for r in records(fq))])
    ctx.set_pick(0)
    # a selection that keeps nothing
    ctx.set_select(Select(min_len=100000))
    assert ctx.decode_host(enc, level=3, out_cap=cap) == b"" and ctx.get_bgzf() is None
    ctx.set_select(None)
    # off again: today's bytes
    ctx.set_bgzf(False)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_bgzf() is None


def test_pairs(zctx):
    ctx = zctx
    a, b = reads(600, 60, 150, 21), reads(600, 60, 150, 22)
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=100, **MODES["frozen"])
    cap = len(a) + len(b) + 4096
    ctx.set_pair_split(True)
    plain = ctx.decode_host(enc, level=3, out_cap=cap)
    first, pairs = ctx.pair_split()
    assert plain == a + b and first == len(a)
    ctx.set_bgzf(True)
    got = ctx.decode_host(enc, level=3, out_cap=cap)
    off = parts_of(ctx, got, [a, b])
    assert ctx.pair_split() == (off[1], pairs)
    # with the pick behind the split
    ctx.set_pick(capi.PICK_NAMES)
    got = ctx.decode_host(enc, level=3, out_cap=cap)
    names = [b"".join(r.split(b"\n")[0][1:] + b"\n" for r in records(x)) for x in (a, b)]
    off = parts_of(ctx, got, names)
    assert ctx.pair_split()[0] == off[1]
    ctx.set_pick(0)
    ctx.set_pair_split(False)
    # a window of pairs: two parts at *split
    ra, rb = records(a), records(b)
    x, y, _ = ctx.decode_pair_range_host(enc, 130, 200, level=3, out_cap=cap)
    parts_of(ctx, x + y, [b"".join(ra[130:330]), b"".join(rb[130:330])])
    assert bgzf_check.check(x) == b"".join(ra[130:330]) and bgzf_check.check(y) == b"".join(rb[130:330])


def test_merge(zctx):
    ctx = zctx
    from test_merge_decode import files
    a, b = files("mixed")
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=100, **MODES["frozen"])
    cap = len(a) + len(b) + 4096
    ctx.set_merge(Merge())
    plain = ctx.decode_host(enc, level=3, out_cap=cap)
    rep, m = ctx.get_merge()
    assert 0 < m < len(plain)
    ctx.set_bgzf(True)
    got = ctx.decode_host(enc, level=3, out_cap=cap)
    off = parts_of(ctx, got, [plain[:m], plain[m:]])
    assert ctx.get_merge()[1] == off[1]
    ctx.set_bgzf(False)
    ctx.set_pair_split(True)
    plain = ctx.decode_host(enc, level=3, out_cap=cap)
    m, first = ctx.get_merge()[1], ctx.pair_split()[0]
    ctx.set_bgzf(True)
    got = ctx.decode_host(enc, level=3, out_cap=cap)
    off = parts_of(ctx, got, [plain[:m], plain[m:first], plain[first:]])
    assert ctx.get_merge()[1] == off[1] and ctx.pair_split()[0] == off[2]


def test_demux(zctx):
    ctx = zctx
    from test_dedup_decode import planted
    fq = planted()[2]
    enc = ctx.encode_host(fq, level=3, block_reads=100, **MODES["frozen"])
    cap = len(fq) + 4096
    ctx.set_demux(Demux([DemuxPart(B, 0, 0, 1, 3)], n_samples=len(ROWS), max_mm=0), ROWS)
    plain = ctx.decode_host(enc, level=3, out_cap=cap)
    _, poff, units = ctx.get_demux()
    ctx.set_bgzf(True)
    got = ctx.decode_host(enc, level=3, out_cap=cap)
    off = parts_of(ctx, got, [plain[poff[i]:poff[i + 1]] for i in range(len(poff) - 1)])
    rep, zoff, zunits = ctx.get_demux()
    assert zoff == off and zunits == units


def test_result_larger_than_out_cap(zctx):
    """out_cap sizes the decoded text; a result that does not fit it is E_OVERFLOW with the size needed.  One short record: its member
    carries 26 bytes of header and trailer and cannot be smaller than the text."""
    ctx = zctx
    fq = reads(1, 10, 10, 9)
    assert len(fq) < 40
    enc = ctx.encode_host(fq, level=3, block_reads=100, **MODES["frozen"])
    ctx.set_bgzf(True)
    got = ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096)
    assert bgzf_check.check(got) == fq and len(got) > len(fq)
    assert ctx.get_bgzf()[0].out_bytes == len(got)
    for cap in (len(fq), len(got) - 1):
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_host(enc, level=3, out_cap=cap)
        assert e.value.code == -5 and ("needs %d bytes" % len(got)) in str(e.value), str(e.value)
        assert ctx.get_bgzf() is None                                   # a refused call has not deflated
    assert ctx.decode_host(enc, level=3, out_cap=len(got)) == got

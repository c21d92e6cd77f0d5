"""The screen switch (sfq_ctx_set_screen) behind the three host decoders: a small archive comes back without the reads that share
k-mers with a reference -- or with those alone -- by the Python rule of screen_rule.py applied to the decoded text; behind the trim
and the selection, IN FRONT OF THE DEDUP (a matched read never enters the dedup's set), the merge, the split, the pair window and
the picks; the refusals at the decode call.  Every comparison is exact byte equality."""
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Dedup, Merge, Screen, Select, Trim
from screen_rule import kmer_set, screen
from test_dedup_decode import dd, planted
from test_merge_decode import parts, split
from test_pairs import records, first_difference
from test_select import MODES, keep, picked
from test_trim import trimmed

pytestmark = pytest.mark.gpu
E_ARG = -1
K = 21


@pytest.fixture
def gctx(ctx):
    """The session's context; afterwards no screen, no sets, no dedup, no merge, no trim, no selection, no pick, no split."""
    ctx.screen_set_destroy()
    try:
        yield ctx
    finally:
        ctx.set_screen(None)
        ctx.screen_set_destroy()
        ctx.set_dedup(None)
        ctx.dedup_set_destroy()
        ctx.set_merge(None)
        ctx.set_trim(None)
        ctx.set_select(None)
        ctx.set_pick(0)
        ctx.set_pair_split(False)
        ctx.set_checksums(False)


def reference(inter):
    """a sequence text that a part of the reads come from: the base lines of every 7th record, either strand"""
    rs = records(inter)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    lines = [r.split(b"\n")[1] for r in rs[::7]]
    return b"\n".join(l if i % 2 else l.translate(comp)[::-1] for i, l in enumerate(lines))


def scr(fq, rule, kset):
    """(the text the rule keeps, the report's first six fields)"""
    kept, units, nm, sw, sh = screen(fq, rule, K, kset)
    rs = records(fq)
    G = 2 if rule.pairs else 1
    return b"".join(rs[r] for r in kept), (units * G, units, len(kept) // G, nm, sw, sh)


def fields(rep):
    return (rep.n_in_range, rep.n_units, rep.n_kept, rep.n_matched_records, rep.n_windows, rep.n_hits)


def test_records_behind_every_host_decoder(gctx):
    ctx = gctx
    fq = planted()[2]                                                 # the interleaved text, coded as records that stand alone
    rs = records(fq)
    ref = reference(fq)
    kset = kmer_set(K, ref)
    enc = ctx.encode_host(fq, level=3, block_reads=100, **MODES["frozen"])
    cap = len(fq) + 4096
    ctx.set_screen(Screen())
    with pytest.raises(capi.SfqError) as e:                           # no set
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG and "screened records:" in str(e.value)
    ctx.screen_set_create(K, len(ref))
    ctx.screen_set_add(ref)
    assert ctx.screen_set_info() == (K, len(kset), len(ref))
    for rule in (Screen(), Screen(keep_matched=True), Screen(min_hits=5, min_pct=60), Screen(first_record=50, n_records=1000)):
        want, rep = scr(fq, rule, kset)
        assert 0 < len(want) < len(fq)
        ctx.set_screen(rule)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), want, "alone")
        got = ctx.get_screen()
        assert fields(got) == rep and (got.text_bytes, got.kept_bytes, got.set_kmers) == (len(fq), len(want), len(kset))
    ctx.set_screen(Screen())
    want = scr(fq, Screen(), kset)[0]
    # checksums on: they are those of the decoded text
    ctx.set_checksums(True)
    enc2 = ctx.encode_host(fq, level=3, block_reads=100, **MODES["frozen"])
    first_difference(ctx.decode_host(enc2, level=3, out_cap=cap), want, "with checksums")
    assert ctx.checksums() == (enc2.crcs, enc2.text_crc)
    ctx.set_checksums(False)
    # a window of blocks; the rule's range inside it
    window = b"".join(rs[200:700])
    got, _ = ctx.decode_range_host(enc, 2, 5, level=3, out_cap=cap)
    first_difference(got, scr(window, Screen(), kset)[0], "blocks 2..+5")
    g = Screen(first_record=50, n_records=300, keep_matched=True)
    ctx.set_screen(g)
    got, _ = ctx.decode_range_host(enc, 2, 5, level=3, out_cap=cap)
    first_difference(got, scr(window, g, kset)[0], "records 50..+300 of blocks 2..+5")
    assert fields(ctx.get_screen()) == scr(window, g, kset)[1]
    # the picks behind
    ctx.set_screen(Screen())
    for w in (capi.PICK_FASTA, capi.PICK_BASES):
        ctx.set_pick(w)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(want, w), "pick %d" % w)
    ctx.set_pick(0)
    # THE ORDER: the trim, the selection, the screen, the dedup: the screen judges the trimmed lines of the records the selection kept
    # (a record's verdict is a function of its key, so the order of screen and dedup shows in the dedup's SET, below, not in the text)
    t, s = Trim(tail=2), Select(motif=b"ACG", min_len=58)
    t_text = trimmed(fq, t)[0]
    chain = dd(scr(keep(t_text, s), Screen(), kset)[0])
    assert 0 < len(chain) < len(dd(keep(t_text, s)))
    ctx.set_trim(t)
    ctx.set_select(s)
    ctx.set_dedup(Dedup())
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), chain, "behind the trim and the selection, in front of the dedup")
    assert ctx.get_screen().text_bytes == ctx.get_select().kept_bytes and ctx.get_dedup().text_bytes == ctx.get_screen().kept_bytes
    ctx.set_trim(None)
    ctx.set_select(None)
    # ... observed through the dedup's set: only what the screen kept is in it
    ctx.dedup_set_create(len(rs), len(fq), 0)
    ctx.set_dedup(Dedup(use_set=True))
    seen = {}
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), dd(want, Dedup(use_set=True), seen), "into the dedup's set")
    assert ctx.dedup_set_info()[0] == len(seen) == ctx.get_dedup().n_kept
    matched = scr(fq, Screen(keep_matched=True), kset)[0]
    ctx.set_screen(Screen(keep_matched=True))                         # now the matched reads alone: none of them is known to the set
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), dd(matched, Dedup(use_set=True), seen), "the matched reads are new to the set")
    assert ctx.get_dedup().n_dup_set == 0
    ctx.set_dedup(None)
    ctx.dedup_set_destroy()
    # a selection that keeps nothing: nothing is left to screen; a screen that keeps nothing: the passes behind are skipped
    ctx.set_select(Select(min_len=1000))
    assert ctx.decode_host(enc, level=3, out_cap=cap) == b"" and ctx.get_screen() is None
    ctx.set_select(None)
    ctx.set_screen(Screen(min_hits=1000, keep_matched=True))
    ctx.set_dedup(Dedup())
    assert ctx.decode_host(enc, level=3, out_cap=cap) == b"" and ctx.get_screen().n_kept == 0 and ctx.get_dedup() is None
    ctx.set_dedup(None)
    with pytest.raises(capi.SfqError) as e:
        ctx.set_screen(Screen(min_hits=0))
    assert e.value.code == E_ARG
    # off again: today's bytes
    ctx.set_screen(None)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_screen() is None


def test_pairs_behind_every_host_decoder(gctx):
    ctx = gctx
    a, b, inter = planted()
    rs = records(inter)
    ref = reference(inter)
    kset = kmer_set(K, ref)
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=14, **MODES["frozen"])
    cap = len(inter) + 4096
    ctx.screen_set_create(K, len(ref))
    ctx.screen_set_add(ref)
    either, both = Screen(pairs=1), Screen(pairs=2)
    w1, w2 = scr(inter, either, kset)[0], scr(inter, both, kset)[0]
    assert 0 < len(w1) < len(w2) < len(inter)
    for rule, want in ((either, w1), (both, w2), (Screen(pairs=2, keep_matched=True), scr(inter, Screen(pairs=2, keep_matched=True), kset)[0])):
        ctx.set_screen(rule)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), want, "interleaved")
        assert fields(ctx.get_screen()) == scr(inter, rule, kset)[1]
        wa, wb = split(want)
        ctx.set_pair_split(True)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), wa + wb, "split")
        ctx.set_pair_split(False)
    # a window of pairs: the entry supplies the range
    ctx.set_screen(either)
    for first_pair, n in ((100, 400), (101, 30), (0, 1200)):
        part = b"".join(rs[2 * first_pair:2 * (first_pair + n)])
        win = scr(part, either, kset)[0]
        first, second, _ = ctx.decode_pair_range_host(enc, first_pair, n, out_cap=cap)
        assert (first, second) == split(win), "pairs %d..+%d" % (first_pair, n)
        assert fields(ctx.get_screen()) == scr(part, either, kset)[1]
    # ... behind a selection of pairs, which has cut to the window, and in front of the dedup of pairs
    s = Select(motif=b"ACGT", pairs=capi.SELECT_EITHER)
    ctx.set_select(s)
    ctx.set_dedup(Dedup(pairs=1))
    win = dd(scr(keep(b"".join(rs[200:1000]), s), either, kset)[0], Dedup(pairs=1))
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 400, out_cap=cap)
    assert (first, second) == split(win) and 0 < len(win)
    ctx.set_select(None)
    win = dd(scr(b"".join(rs[200:1000]), either, kset)[0], Dedup(pairs=1))
    first, second, _ = ctx.decode_pair_range_host(enc, 100, 400, out_cap=cap)
    assert (first, second) == split(win) and 0 < len(win)
    ctx.set_dedup(None)
    # the merge behind: it sees the pairs that are left
    m = Merge(min_overlap=12)
    front, rest, rep = parts(w1, m)
    assert 0 < len(front) and 0 < len(rest)
    ctx.set_merge(m)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), front + rest, "merged")
    # refused at the decode call: by record where mates must stay in step; a range under the pair window
    ctx.set_screen(Screen())
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)                    # the merge is on
    assert e.value.code == E_ARG and "screened records:" in str(e.value)
    ctx.set_merge(None)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), scr(inter, Screen(), kset)[0], "by record: no pass behind that wants pairs")
    ctx.set_pair_split(True)
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(enc, level=3, out_cap=cap)
    assert e.value.code == E_ARG and "screened records:" in str(e.value)
    ctx.set_pair_split(False)
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_pair_range_host(enc, 100, 400, out_cap=cap)
    assert e.value.code == E_ARG and "screened records:" in str(e.value)
    for bad in (Screen(pairs=1, first_record=2), Screen(pairs=2, n_records=100)):
        ctx.set_screen(bad)
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_pair_range_host(enc, 100, 400, out_cap=cap)
        assert e.value.code == E_ARG
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), scr(inter, Screen(pairs=2, n_records=100), kset)[0], "the other decoders take a range")
    # off again: today's bytes
    ctx.set_screen(None)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == inter and ctx.get_screen() is None

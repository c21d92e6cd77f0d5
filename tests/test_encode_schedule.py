"""GPU: the encode call's schedule (api.cpp encode_body).  Under the match model the verdict's passes fork in FRONT of the
quality sample's histogram (EE_BLOCKS_READY), the chains' size lists are cleared on side streams that reach their writers, the blocks' first headers
come home with the head, and the "chn.idx" bytes and the block descriptors' copy run beside the packing.  None of that may change a byte.

A wrong wait shows as bytes that differ from run to run, from a context with another history, or as a text that does not come back.  Every
case therefore codes its text three times on the session's context with calls of other sizes in between, once on a fresh context, and
compares ALL of what a call leaves -- the packed streams, index(), first_headers(), prior(), chains(), rec_prior(), the result's counts,
sizes and offsets (checksums and statistics where they are on) --, decodes, and where the suite has a host oracle for the block's bytes
(test_frozen_tables.check_against_oracle, test_match_walk.encoded_as_the_oracle_says) holds the first run to it.

The cases are the smallest texts that take each path the schedule touches, in blocks of 64 records:
  no model          bases with nothing to learn: 129 records are three blocks, the fewest for which gen_bounds gives three generations (the
                    verdict's passes run and turn the model down); 128 are two, and gm_begin returns before it queues anything
  match model       match_mint's texts: the verdict turns the model on, the base chains get a size list of their own (gm_csz) and "chn.idx"
                    is made from the joined lists (gm_idx)
  one record / one block
  segments          match_mint's segment text (SFQ_CHAIN_SEGMENT), and a few long reads that take segments by themselves: the host waits
                    for the segment counts in the middle of the head, and the size lists are sized by what it learns
  long headers      all over 127 bytes: the general header kernel
  first headers     every block's first header 1 / 255 / 256 / 300 bytes: the blob's guessed part is 256 bytes a block, so the last one
                    comes home in the second copy, behind the final synchronise
  given / counts    SFQ_PRIOR_GIVEN; sfq_count_priors and then SFQ_PRIOR_COUNTS
  checksums + statistics on together (two more streams beside the head)
  models            qualities alone, headers alone, bases alone: no wait may name a stream that never ran
  kernel = 2        round 4's generation tables: the schedule of before (nothing forks early, nothing runs beside the packing)"""
import zlib

import numpy as np
import pytest
import torch

import match_mint as M
import util
from slimfastq_amd import capi
from test_frozen_tables import check_against_oracle
from test_match_walk import call as match_call, encoded_as_the_oracle_says

pytestmark = pytest.mark.gpu
BR, CR = 64, 16
FROZEN = dict(level=3, block_reads=BR, prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=CR)


def records(n, seed, read_len=100, header=None):
    """n records of random bases (nothing to learn) and qualities; header(i) -> the header's text"""
    rng = np.random.default_rng(seed)
    acgt, q = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"#5:?FI", np.uint8)
    out = []
    for i in range(n):
        L = read_len if isinstance(read_len, int) else int(rng.integers(*read_len))
        h = header(i) if header else b"run7:%d:%d" % (i // 50, 1000 + i)
        out.append(b"@%s\n%s\n+\n%s\n" % (h, acgt[rng.integers(0, 4, L)].tobytes(), q[rng.integers(0, 6, L)].tobytes()))
    return b"".join(out)


_OTHERS = {}


def other_text(k):
    """The calls in between: a smaller and a larger one, of other block and chain geometry"""
    if k not in _OTHERS:
        _OTHERS[k] = records(37, 90, 60) if k == 0 else records(1500, 91, (20, 180))
    return _OTHERS[k]


def left_behind(enc):
    """Everything a call leaves, as comparable values"""
    r = enc.res
    d = dict(data=bytes(enc.data), index=bytes(enc.blocks), first_headers=bytes(enc.first_hdrs), prior=bytes(enc.prior), chains=bytes(enc.chains),
             rec_prior=bytes(enc.rec_prior), counts=(r.n_records, r.n_blocks, r.n_chains, r.first_hdr_bytes, r.total_bytes),
             stream_bytes=list(r.stream_bytes), stream_offset=list(r.stream_offset), crcs=enc.crcs, text_crc=enc.text_crc,
             stats=None if enc.stats is None else bytes(enc.stats))
    return d


def same(a, b, what):
    for k in a:
        if k in ("data", "first_headers", "chains", "index") and a[k] != b[k]:
            util.first_difference(b[k], a[k], "%s: %s" % (what, k))
        assert a[k] == b[k], (what, k)


def scheduled(ctx, fq, kw=FROZEN, before=None, oracle=None, both=None, decodes=True):
    """The text three times on the session's context, other calls in between; once on a fresh context; all alike, and the text comes back.
    before(c): what a call needs installed in context c first; oracle(enc): the host's word on the first run; both(c, on): a switch of the
    context, on for the text's calls alone; decodes: the call codes every model, so its streams are an archive"""
    def code(c):
        if both:
            both(c, True)
        try:
            if before:
                before(c)
            return c.encode_host(fq, **kw)
        finally:
            if both:
                both(c, False)
    first = code(ctx)
    runs = [left_behind(first)]
    for k in (0, 1):
        o = other_text(k)
        assert ctx.decode_host(ctx.encode_host(o, level=3, block_reads=(500, 96)[k], prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN), level=3, out_cap=len(o) + 4096) == o
        runs.append(left_behind(code(ctx)))
    fresh = capi.Context(0, table_budget=4 << 30)
    try:
        runs.append(left_behind(code(fresh)))
    finally:
        fresh.close()
    for i, r in enumerate(runs[1:]):
        same(runs[0], r, ("second run", "third run", "fresh context")[i])
    nb = first.res.n_blocks
    assert first.res.n_records == fq.count(b"\n") // 4 and nb == len(first.blocks) and first.res.first_hdr_bytes == len(first.first_hdrs)
    # the index and the blob say where every block's first header is
    chunks = util.split_records(fq, kw["block_reads"]) if kw["block_reads"] not in (0, capi.BLOCK_AUTO) else None
    if chunks:
        assert nb == len(chunks)
        for b, chunk in enumerate(chunks):
            o, n = first.blocks[b].first_hdr_off, first.blocks[b].first_hdr_len
            assert first.first_hdrs[o:o + n] == chunk[1:chunk.index(b"\n")], b
    if decodes:
        assert ctx.decode_host(first, level=kw["level"], out_cap=len(fq) + 4096) == fq
    if oracle:
        oracle(first)
    return first


def by_the_oracle(fq, kw=FROZEN):
    return lambda enc: check_against_oracle(None, fq, kw["level"], kw["block_reads"], kw["chain_reads"], kw["prior_step"], enc=enc)


@pytest.mark.parametrize("nrec", [2 * BR + 1, 2 * BR])
def test_bases_with_nothing_to_learn(ctx, nrec):
    """Three blocks: the verdict's passes run beside the histogram and turn the model down.  Two: there is no verdict to wait for."""
    fq = records(nrec, 1)
    enc = scheduled(ctx, fq, oracle=by_the_oracle(fq))
    assert not util.unpack_chains(enc.chains)["flags"] & 1


@pytest.mark.parametrize("name", ["generations", "unequal"])
def test_bases_that_repeat_take_the_match_model(ctx, name):
    t = M.text(name)
    scheduled(ctx, t["fq"], kw=match_call(t), oracle=lambda enc: encoded_as_the_oracle_says(t, enc))


@pytest.mark.parametrize("nrec", [1, BR])
def test_a_single_record_and_a_single_block(ctx, nrec):
    fq = records(nrec, 2)
    scheduled(ctx, fq, oracle=by_the_oracle(fq) if nrec >= CR else None)          # (the oracle helper wants a whole chain of records)


def test_segments_on_request(ctx):
    t = M.text("segments")
    enc = scheduled(ctx, t["fq"], kw=match_call(t), oracle=lambda enc: encoded_as_the_oracle_says(t, enc))
    assert util.unpack_chains(enc.chains, len(enc.blocks))["flags"] & 8


def test_a_few_long_reads_take_segments_by_themselves(ctx):
    fq = capi.synth_fastq(12, 150, seed=3, kind=1)                           # 10-50 kb a read
    enc = scheduled(ctx, fq, kw=dict(level=3, block_reads=capi.BLOCK_AUTO, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN))
    assert util.unpack_chains(enc.chains, len(enc.blocks))["flags"] & 8


def test_headers_over_127_bytes(ctx):
    fq = records(3 * BR + 5, 3, 80, header=lambda i: b"instrument-%d:flowcell-%s:%d:%d %s" % (i % 3, b"ABCDEFGH" * 4, i // 7, 20000 + 13 * i, b"x" * (90 + i % 40)))
    assert min(len(ln) for ln in fq.split(b"\n")[0::4] if ln) > 128
    scheduled(ctx, fq, oracle=by_the_oracle(fq))


@pytest.mark.parametrize("first_len", [1, 255, 256, 300])
def test_block_first_headers_of(ctx, first_len):
    """256 bytes a block come home before the blob's size is known: 300 a block takes the second copy as well"""
    def header(i):
        if i % BR:
            return b"r:%d:%d" % (i // 9, i)
        return (b"%d" % (i // BR % 10)) if first_len == 1 else (b"first.%d." % i).ljust(first_len, b"z")
    fq = records(4 * BR + 7, 4 + first_len, 70, header=header)
    enc = scheduled(ctx, fq, oracle=by_the_oracle(fq))
    assert [b.first_hdr_len for b in enc.blocks] == [first_len] * 5 and len(enc.first_hdrs) == 5 * first_len


def test_priors_that_are_given(ctx):
    fq = records(5 * BR, 5)
    made = ctx.encode_host(records(5 * BR, 6), **FROZEN)
    enc = scheduled(ctx, fq, kw=dict(FROZEN, prior_step=capi.PRIOR_GIVEN), before=lambda c: c.set_priors(made.prior, made.rec_prior))
    assert enc.prior == made.prior and enc.rec_prior == made.rec_prior


def test_counts_and_then_the_encode_from_them(ctx):
    fq = records(5 * BR, 7)
    d = torch.frombuffer(bytearray(fq), dtype=torch.uint8).cuda()

    def count(c):
        c.count_priors(d.data_ptr(), len(fq), level=3, block_reads=BR, prior_step=1, tables=capi.TABLES_FROZEN)
    plain = ctx.encode_host(fq, **FROZEN)
    enc = scheduled(ctx, fq, kw=dict(FROZEN, prior_step=capi.PRIOR_COUNTS), before=count)
    same(left_behind(plain), left_behind(enc), "counted first against sampled in the call")     # (the same sample either way)


def test_checksums_and_statistics_on_together(ctx):
    fq = records(3 * BR + 9, 8)

    def both(c, on):
        c.set_checksums(on)
        c.set_stats(on)
    enc = scheduled(ctx, fq, both=both, oracle=by_the_oracle(fq))
    assert enc.crcs == [zlib.crc32(c) for c in util.split_records(fq, BR)] and enc.text_crc == zlib.crc32(fq)
    assert enc.stats is not None and enc.stats.n_records == 3 * BR + 9
    same({k: v for k, v in left_behind(ctx.encode_host(fq, **FROZEN)).items() if k not in ("crcs", "text_crc", "stats")},
         left_behind(enc), "with the two passes beside the head")


@pytest.mark.parametrize("models", [capi.M_QLT, capi.M_REC, capi.M_GEN, capi.M_QLT | capi.M_USR])
def test_models_limited_to(ctx, models):
    """A stream whose model is off still forks and joins: nothing waits for an event that was not recorded in this call"""
    fq = records(3 * BR + 1, 9)
    whole = ctx.encode_host(fq, **FROZEN)
    part = scheduled(ctx, fq, kw=dict(FROZEN, models=models), decodes=False)
    for name, m in (("qlt", capi.M_QLT), ("rec", capi.M_REC), ("gen", capi.M_GEN)):
        assert part.stream(name) == (whole.stream(name) if models & m else b""), name


def test_round_4_generation_tables_keep_their_schedule(ctx):
    fq = records(3 * BR + 1, 10)
    scheduled(ctx, fq, kw=dict(FROZEN, kernel=2))
    t = M.text("generations")
    scheduled(ctx, t["fq"], kw=dict(match_call(t), kernel=2))


def test_adaptive_tables_and_format_6(ctx):
    fq = records(3 * BR + 1, 11)
    scheduled(ctx, fq, kw=dict(level=3, block_reads=BR, prior_step=0, tables=capi.TABLES_ADAPTIVE))
    scheduled(ctx, fq, kw=dict(level=3, block_reads=0, prior_step=0, tables=capi.TABLES_ADAPTIVE))

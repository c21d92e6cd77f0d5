"""GPU: every hand-written copy of the range coder through its interval clamp (coder.hpp:76-77; dev_coder.h RcEnc / RcDec, dev_wavepw.h,
dev_multicoder.h, dev_chain.h LaneEnc / LaneEncB and the lane decoders, and the kernels built on them).  The line runs once in 2^32
renormalisations, so ordinary text never reaches it; the texts of clamp_mint.py do, dozens to thousands of times each (test_clamp_inputs.py
holds them to that on the CPU).  Every case encodes legal FASTQ through the C ABI, compares every stream -- chain by chain where there are chains --
with the oracle's bytes, decodes on the GPU and compares with the text.  No GPU decoder is handed bytes that an encoder did not write.

Not reached: the frozen mode's header chains (k_rec_code and its decoders) -- minting headers means steering the token model."""
import numpy as np
import pytest

import clamp_mint as M
import util
from oracle import oracle as O
from slimfastq_amd import capi
from test_frozen_tables import SEG, base_chains_oracle
from test_gpu_parity import assert_streams_equal

pytestmark = pytest.mark.gpu


def assert_chains_equal(got, got_sizes, want, want_sizes, what=""):
    """Chain by chain, so that a failure names the first chain that differs."""
    assert len(got_sizes) == len(want_sizes), what
    g = w = 0
    for c, (gs, ws) in enumerate(zip(got_sizes, want_sizes)):
        gs, ws = int(gs), int(ws)
        assert got[g:g + gs] == want[w:w + ws], "%s chain %d of %d: got %d bytes, want %d" % (what, c, len(want_sizes), gs, ws)
        g += gs; w += ws
    assert g == len(got) and w == len(want), what


def clamping(fn, *a, **k):
    """fn's result -- and the oracle must have clamped at least MIN_CLAMPS times while it made it (else the case checks nothing)."""
    out, n = M.clamps_of(fn, *a, **k)
    assert n >= M.MIN_CLAMPS, n
    return out


@pytest.mark.parametrize("lds_rows", (0, capi.LDS_ROWS_NONE))
@pytest.mark.parametrize("name", sorted(M.FROZEN_QLT))
def test_frozen_quality_chains_through_the_clamp(ctx, name, lds_rows):
    """LaneEncB in k_qlt_encode_c (branch-free, its fix masked per lane behind a wave-wide test) and k_qlt_decode_c's decoders, lds_rows
    automatic and none.  (Under a given prior, and with fewer than 150 000 chains, the encoder stages no rows in LDS either way -- api.cpp
    want_hot --, so its LDS instantiation runs the same LaneEncB but is not reached here; the decoder takes lds_rows as given.)  all-lanes: every chain of a wavefront is minted; lane0 / lane31 / lane63: one minted chain among 63 ordinary ones that
    renormalise without straddling, or not at all, while it takes the fix; unequal-lengths: chain c's lines are 20 + 2 c symbols long, so the
    short chains' lanes have finished when the long ones clamp; segments: the chains are pieces of 75 symbols of one record."""
    t = M.frozen_qlt(*M.FROZEN_QLT[name])
    fq, level = t["fq"], t["level"]
    want, sizes, extra = clamping(M.frozen_qlt_streams, t)
    ctx.set_priors(t["prior"], t["rec_prior"])
    try:
        enc = ctx.encode_host(fq, level=level, block_reads=t["br"], prior_step=capi.PRIOR_GIVEN, tables=capi.TABLES_FROZEN,
                              chain_reads=SEG | t["seg"] if t["seg"] else t["cr"], lds_rows=lds_rows)
        assert enc.prior == t["prior"] and len(enc.blocks) == 1
        ci = util.unpack_chains(enc.chains, 1)
        assert bool(ci["flags"] & 8) == bool(t["seg"]) and ci["chain_reads"] == (1 if t["seg"] else t["cr"])
        assert_chains_equal(enc.stream("qlt"), ci["qlt"], want, sizes, name)
        assert sum(b.extra_hi for b in enc.blocks) == extra == 0
        assert ctx.decode_host(enc, level=level, out_cap=len(fq) + 4096, lds_rows=lds_rows) == fq
    finally:
        ctx.set_priors(b"", b"")


@pytest.mark.parametrize("kernel", (0, 1))
@pytest.mark.parametrize("level", sorted(M.FORMAT6))
def test_format_6_streams_through_the_clamp(ctx, level, kernel):
    """One block, the reference's own streams (RcEnc / RcDec in the lane-per-block kernels, the wave coder in the default ones): the quality
    stream and the base stream (the level's gen_bits) both minted."""
    t = M.adaptive(*M.FORMAT6[level])
    fq = t["fq"]
    clamping(M.adaptive_qlt_streams, t); clamping(M.adaptive_gen_streams, t)
    enc = ctx.encode_host(fq, level=level, block_reads=0, kernel=kernel)
    assert enc.res.n_blocks == 1 and enc.blocks[0].gen_bits == t["gen_bits"]
    assert_streams_equal(enc, O.compress(fq, level).streams, ctxmsg="level %d kernel %d" % (level, kernel))
    assert ctx.decode_host(enc, level=level, out_cap=len(fq) + 4096, kernel=kernel) == fq


@pytest.mark.parametrize("kernel", (0, 1))
@pytest.mark.parametrize("name", sorted(M.BLOCKS))
def test_adaptive_blocks_through_the_clamp(ctx, name, kernel):
    """The block format with adaptive tables, 64 blocks of 16 or 32 records (dev_wavepw.h, dev_multicoder.h, decode_w.hip; kernel = 1: the
    lane-per-block kernels): cold rows (prior_step 0) with qualities and bases minted; a prior counted over the text itself (prior_step 1) with
    the bases minted -- that prior is a function of the text, so no quality line can be minted under it --; and the same warm start from a GIVEN
    prior, under which the qualities are minted -- after showing that a counted prior and the same prior given are coded from alike."""
    args, step = M.BLOCKS[name]
    t = M.adaptive(*args)
    fq, level, br = t["fq"], t["level"], t["br"]
    starts, lens = util.line_table(fq)
    qoff, qlen = starts[3::4], lens[3::4]
    gens = clamping(M.adaptive_gen_streams, t)
    rows = t["rows66"]
    if step == 1:
        rows = O.qlt_prior_rows(O.qlt_histogram(fq, qoff, np.minimum(qlen, M.PRIOR_SYMBOLS), level, 0, 1))
        want, sizes = O.qlt_encode_blocks(fq, qoff, qlen, level, br, rows)
    else:
        want, sizes = clamping(M.adaptive_qlt_streams, t)
    if step == capi.PRIOR_GIVEN:
        # The prior this case is given is, byte for byte, the one a prior_step = 1 call counts over the ordinary text, and that call's quality
        # blocks are the blocks a call GIVEN it writes: the two differ in how the rows get to the device (api.cpp: launch_prior_rows there,
        # upload_prior here), not in the kernels that code from them (ctx->prior_on, fill_model_args).
        plain = t["plain"]
        counted = ctx.encode_host(plain, level=level, block_reads=br, gen_bits=t["gen_bits"], kernel=kernel, prior_step=1)
        assert counted.prior == t["prior"]
        ctx.set_priors(t["prior"], b"")
        try:
            given = ctx.encode_host(plain, level=level, block_reads=br, gen_bits=t["gen_bits"], kernel=kernel, prior_step=step)
        finally:
            ctx.set_priors(b"", b"")
        assert given.prior == counted.prior and given.stream("qlt") == counted.stream("qlt")
        assert [b.size[2] for b in given.blocks] == [b.size[2] for b in counted.blocks]
    ctx.set_priors(t["prior"], b"")
    try:
        enc = ctx.encode_host(fq, level=level, block_reads=br, gen_bits=t["gen_bits"], kernel=kernel, prior_step=step)
        chunks = util.split_records(fq, br)
        assert enc.res.n_blocks == len(chunks) == len(sizes)
        if rows is not None:
            assert np.array_equal(util.unpack_prior(enc.prior, M.q_rows(level)), rows)
        assert_chains_equal(enc.stream("qlt"), [b.size[2] for b in enc.blocks], want, sizes, name + " qlt block")
        assert_chains_equal(enc.stream("gen"), [b.size[1] for b in enc.blocks], b"".join(gens), [len(g) for g in gens], name + " gen block")
        for b in (0, len(chunks) // 2, len(chunks) - 1):                         # the other streams: the reference's for a file holding the block
            ref = util.block_reference(chunks[b], level, gen_bits=t["gen_bits"]).streams
            for s in capi.STREAM_NAMES:
                if s != "qlt":
                    assert enc.stream(s, b) == ref.get(s, b""), (name, s, b)
        assert ctx.decode_host(enc, level=level, out_cap=len(fq) + 4096, kernel=kernel) == fq
    finally:
        ctx.set_priors(b"", b"")


def test_match_model_base_chains_through_the_clamp(ctx):
    """Frozen tables, the bases under the match model (k_gm_code, k_gm_decode_c): the last generation's chains minted."""
    t = M.frozen_bases(*M.FROZEN_BASES["gm"])
    fq = t["fq"]
    clamping(M.frozen_bases_streams, t)
    enc = ctx.encode_host(fq, level=3, block_reads=t["br"], prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=t["cr"])
    ci = util.unpack_chains(enc.chains)
    assert ci["flags"] & 32 and ci["flags"] & 1 and ci["gm_table_bits"] == t["tb"]
    starts, lens = util.line_table(fq)
    want, sizes, on = base_chains_oracle(fq, starts[1::4], lens[1::4], ci, t["br"], t["cr"])
    assert on == 1 and ci["gen_chain_reads"] == t["cr"]                          # the chains the text was minted for
    assert_chains_equal(enc.stream("gen"), ci["gen"], want, sizes, "gm")
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq


def test_generation_table_base_chains_through_the_clamp(ctx):
    """Frozen tables with kernel = 2: the bases under generation tables of Base2 rows (k_gen_encode_c, k_gen_decode_c), the last generation's
    chains minted."""
    t = M.frozen_bases(*M.FROZEN_BASES["tables"])
    fq = t["fq"]
    want, sizes, on = clamping(M.frozen_bases_streams, t)
    enc = ctx.encode_host(fq, level=3, block_reads=t["br"], gen_bits=t["gen_bits"], prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=t["cr"], kernel=2)
    ci = util.unpack_chains(enc.chains)
    assert ci["flags"] & 1 and not ci["flags"] & 32 and enc.blocks[0].gen_bits == t["gen_bits"] and ci["gen_chain_reads"] == t["cr"]
    assert on == 1
    assert_chains_equal(enc.stream("gen"), ci["gen"], want, sizes, "generation tables")
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq

"""The quality chains' kernel (chains.hip k_qlt_encode_c) has the model's level as a template parameter -- levels 1-2 and levels 3-4 are two
kernels, each in a 256-lane form that reads its rows from the table and a 1024-lane form that stages the hottest rows in LDS -- and its
coder (dev_chain.h LaneEncB) runs the second and later renormalisation rounds of a symbol in a block of its own.  Neither may move a
byte: every instantiation at every level, and texts whose symbols nearly all need a second round, must give the oracle's "qlt" stream and
chain sizes (O.qlt_histogram -> O.qlt_prior_rows -> O.qlt_frozen_rows -> O.qlt_encode_chains, as test_frozen_tables.check_against_oracle
does for its calls) and decode back to the text."""
import numpy as np
import pytest

from slimfastq_amd import capi
from oracle import oracle as O
import util

pytestmark = pytest.mark.gpu
PRIOR_SYMBOLS = 4096
KERNELS = (capi.LDS_ROWS_NONE, 64)            # rows from the table (256 lanes); 64 rows staged: the 1024-lane image kernel at any size
_reference = {}                               # (text, level, ...) -> what the oracle says, computed once and shared by both kernels


def _kernel_id(lds):
    return "table" if lds == capi.LDS_ROWS_NONE else "lds%d" % lds


def quality_reference(key, fq, level, br, cr, step, solid):
    if key not in _reference:
        starts, lens = util.line_table(fq)
        qoff, qlen = starts[3::4] + solid, lens[3::4] - solid
        rows66 = O.qlt_prior_rows(O.qlt_histogram(fq, qoff, np.minimum(qlen, PRIOR_SYMBOLS), level, 0, step))
        want, sizes, extra = O.qlt_encode_chains(fq, qoff, qlen, level, br, min(cr, br), O.qlt_frozen_rows(rows66))
        rows66.setflags(write=False); sizes.setflags(write=False)
        _reference[key] = (rows66, want, sizes, extra)
    return _reference[key]


def check_quality_chains(ctx, key, fq, level, br, cr, step, lds):
    enc = ctx.encode_host(fq, level=level, block_reads=br, prior_step=step, tables=capi.TABLES_FROZEN, chain_reads=cr, lds_rows=lds)
    rows66, want, sizes, extra = quality_reference(key, fq, level, br, cr, step, enc.blocks[0].solid)
    ci = util.unpack_chains(enc.chains)
    assert ci["chain_reads"] == min(cr, br)
    assert np.array_equal(util.unpack_prior(enc.prior, 4096 if level == 1 else 65536), rows66), key
    assert list(ci["qlt"]) == list(sizes), key
    got = enc.stream("qlt")
    assert got == want, (key, util.first_difference(got, want, "qlt"))
    assert sum(b.extra_hi for b in enc.blocks) == extra, key
    assert ctx.decode_host(enc, level=level, out_cap=len(fq) + 4096, lds_rows=lds) == fq, key
    return want


def hostile_fastq(nrec, n, seed=17):
    """Equal-length records.  Every fourth record -- the ones a prior of step 4 samples -- has all-'I' qualities; the others are 'I' with
    every third quality drawn uniformly from '!' .. '~', the escapes (over '!' + 62) included.  The frozen rows know 'I' alone, so a drawn
    symbol and the 'I' after it cost 2.3-3.6 stream bytes: nearly every one takes a second renormalisation round, many an escape with
    rounds of its own.  -> (text, number of drawn symbols)"""
    rng = np.random.default_rng(seed + n)
    out = bytearray()
    drawn = 0
    for r in range(nrec):
        q = np.full(n, ord("I"), np.uint8)
        if r % 4:
            at = np.arange(0, n, 3)
            q[at] = rng.integers(ord("!"), ord("~") + 1, len(at))
            drawn += len(at)
        out += b"@h.%d\n" % r + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n)) + b"\n+\n" + bytes(q) + b"\n"
    return bytes(out), drawn


_texts = {}                                   # a text is made once


def _text(name, n=0):
    if (name, n) not in _texts:
        _texts[(name, n)] = capi.synth_fastq(4000, 150) if name == "synth" else hostile_fastq(2048, n)
    return _texts[(name, n)]


@pytest.mark.parametrize("lds", KERNELS, ids=_kernel_id)
@pytest.mark.parametrize("level", (1, 2, 3, 4))
def test_every_instantiation_at_every_level(ctx, level, lds):
    fq = _text("synth")
    check_quality_chains(ctx, ("synth", level), fq, level, br=500, cr=25, step=1, lds=lds)


@pytest.mark.parametrize("lds", KERNELS, ids=_kernel_id)
@pytest.mark.parametrize("level", (1, 2, 3, 4))
@pytest.mark.parametrize("n", (6, 22, 150))
def test_second_and_third_rounds_in_every_lane(ctx, n, level, lds):
    fq, drawn = _text("hostile", n)
    want = check_quality_chains(ctx, ("hostile", n, level), fq, level, br=256, cr=4, step=4, lds=lds)
    # the text is what it is meant to be: more than two stream bytes a drawn symbol (a symbol that leaves a byte or none takes no second round)
    assert len(want) > 2 * drawn, (len(want), drawn)

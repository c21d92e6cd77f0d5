"""GPU: the quality prior's chain of kernels against the rule it must equal (oracle/sfq_oracle.c: sfqo_qlt_histogram, sfqo_qlt_prior_rows,
frozen_row), on the inputs of prior_mint.py (test_prior_inputs.py holds them to their claims on the CPU):

  1. counts      sfq_count_priors + sfq_get_prior_counts of every histogram text, levels 1 .. 4, steps 1 and 3, sample_scale 1 and 2: the count
                 table equals O.qlt_histogram's, word for word (k_qlt_hist and its bytewise tail, k_qlt_hist_w, every arm of hist_add).  The
                 text lies in device memory exactly as long as it is, between guards of 0xFF (util.Placed); the tail texts also 13 bytes behind a
                 sixteen-byte boundary with FASTQ going on behind them.  The crowded and the hot texts three times over.
  2. rows        chosen count tables through sfq_set_prior_counts: "qlt.pri" holds O.qlt_prior_rows of them (k_prior_rows, k_prior_flags /
                 k_prior_slots / k_prior_gather, pack_prior), the frozen chains are the oracle's under O.qlt_frozen_rows of those rows, the
                 text decodes; and through adaptive tables, both kernels (the lane and the wave layout k_prior_rows also writes).
  3. families    chosen prior rows through sfq_set_qlt_prior + SFQ_PRIOR_GIVEN (unpack_prior, k_prior_scatter, k_qlt_frozen_rows): the
                 quality chains are the oracle's chain by chain, and the decoder (qdec_store, k_qlt_decode_c with and without its LDS image)
                 returns the text -- through rows whose neighbouring cums differ by 1, under every symbol.
  4. wave call   a text of long records through the whole call at levels 1 and 4, in segments of 1000 and with automatic parameters.

No tolerances: every comparison is of integers or bytes.  No GPU decoder is handed bytes that an encoder did not write: the blob of case 3 is
a well-formed prior, which the parser accepts by design, and the streams are the encoder's own.

What case 3 found.  k_qlt_frozen_rows took x << 16 in 32 bits with x = f + 1 up to 65 536, under a comment that said "no overflow": for a
frequency of 65 535 -- the most unpack_prior accepts; the encoder's own rows stop at 32 000 -- the product was 0, all 64 symbols got g = 1
and symbol 0 the remainder, where the rule (frozen_row: a 64-bit product) gives that symbol 65 473.  Encoder and decoder share the kernel, so
a round trip hid it.  With the parent's kernel test_row_families[1] fails at "level 1 chain 0 of 750: got 338 bytes, want 334" (the first byte
that differs is byte 58) and test_row_families[3] at "level 3 chain 0 of 750: got 353 bytes, want 351" (byte 21); the other 156 cases pass.
The product is now taken in 64 bits.  Every other row here has x <= 32 001 and agreed before and after.

Not reached here: the encoder's LDS image (api.cpp want_hot is 0 under a given prior; test_quality_constants.py and
test_frozen_tables.py::test_frozen_quality_rows_staged_in_lds_do_not_change_a_byte hold it); k_prior_slots for a table of other than 4096 or
65 536 rows (one workgroup takes either; no level has another); counts that add up past 2^32 in one context (the all-reduce's business,
no kernel's); hist_add's count carrying into its key (768 adds would have to land between a lane's read and its own add).

Wall time on one MI355X.  This module alone, 158 cases: 17.9 s and 18.1 s as a machine's first process (10.8 s and 11.1 s of them the
first case: the process's first use of torch on the device), 9.5 - 10.9 s in the twenty processes behind one; no other case takes more
than 0.3 s.  The whole suite (CPU and GPU tests, one process): 629 s (1897 passed, 1 skipped) with this module and test_prior_inputs.py, 625 s (1690 passed, 1 skipped) without
the two; inside the suite no case of this module is among the 30 slowest (all over 4 s).

Checked on scratch copies of prior.hip and chains.hip, one predicate or constant changed at a time, this whole module run against each
(counts = test_counts_equal_the_oracles, rows = test_rows_of_installed_counts, families = test_row_families, call = test_wave_histogram_...):
  caught
    hist_add: the harvest's test HIST_HARVEST - 1u -> - 2u       counts: hot (4 levels), lens (4), wave-drops-8 (4), wave-walk-5 (levels 3, 4): the
                                                                 256 taken off a count of 255 borrow from the key
    k_qlt_hist_w: `if (i == 0) ctx = 0` removed                  counts: all 8 wave texts at levels 3 and 4; call: level 4.  (Levels 1 and 2 do not
                                                                 run the statement.)
    k_qlt_hist_w: dsum + incl - t -> dsum + incl                 the same 16 + 2 cases
    k_qlt_hist_w: c1 = rl(b, 63) -> rl(b, 62)                    counts: all 32 wave cases; call: all 4
    k_qlt_hist_w: b < 63u ? b : 63u -> b & 63u                   counts: wave-uniform-9 / 8 / 5 and wave-colour-5 at every level (16); call: all 4.  The
                                                                 walk and the drops texts hold no symbol of 63 or more.
    k_qlt_hist: pos < skip -> pos <= skip                        counts: all 116 cases of the lane texts
    k_qlt_hist: the tail's bytes dropped (wd[k] = 0)             counts: hot, lens, colour and the 12 tail texts whose last dword is a part of one with a
                                                                 symbol in it ((k + L + 1) % 4 >= 2), at every level (60); none of the other 12
    k_prior_rows: > 32000 -> >= 32000                            rows: all 4 levels, at the row "max:42667" (6 * 42 667 >> 3 = 32 000 itself)
    k_prior_rows: the sort key's `| lane` dropped                rows: all 4; call: all 4
    k_qlt_frozen_rows: 63u - lane -> lane in `best`              rows: all 4; families: both; call: all 4
    k_qlt_frozen_rows: `g ? g : 1u` dropped                      families: both (the triples' 61 floors of 0); nothing else has a floor of 0
    k_qlt_frozen_rows: the parent's 32-bit product               families: both (above)
    k_qlt_decode_c: t4 <= -> <                                   families: both; call: all 4
    k_qlt_decode_c: t2 <= -> <, t1 <= -> <                       families: both, each
    k_qlt_decode_c: u4 <= -> <                                   families: both; call: level 1, segments of 1000
    k_qlt_decode_c: u2 <= -> <, u1 <= -> <                       rows: all 4; families: both; call: all 4, each
    k_qlt_decode_c: `& 0xffffu` on the frequency dropped         families: both; call: all 4 (symbol 63, whose next cum is the total, stored as 0)
  changes no count and no byte, and cannot be caught
    hist_add: the probe limit 128 -> 16                          a key that gives up its search is added to the same counter in memory that its slot
                                                                 would be flushed to.  The crowded texts hold 27 000 keys and more a workgroup
                                                                 against 16 384 slots: they run that arm under either limit, and their counts are
                                                                 the oracle's under both
    hist_add: >= 768u -> >= 1024u                                the count's field is ten bits (HIST_CMASK 1023): the test is then never true and every
                                                                 add goes through the slot, which the harvest keeps below 1024 unless 768 adds land
                                                                 between one lane's add and its subtraction -- no text makes that happen on demand
    qdec_store: `row[8 + 63] = 0` dropped                        the word is then never written, and a buffer fresh from the allocator reads 0 there:
                                                                 the run passed all 158 cases.  It shows only in a reused buffer that held something else.
Every case fails under one of these changes or more: the counts of the lane texts under `pos <= skip`, those of the wave texts under
rl(b, 62), the rows, the families and the call under `best`.
"""
import functools

import numpy as np
import pytest

import prior_mint as M
import util
from oracle import oracle as O
from slimfastq_amd import capi
from test_clamp_gpu import assert_chains_equal
from test_frozen_tables import SEG
from util import Placed

pytestmark = pytest.mark.gpu
FROZEN, ADAPTIVE = capi.TABLES_FROZEN, capi.TABLES_ADAPTIVE


@functools.lru_cache(maxsize=8)
def want_counts(name, level, step):
    return M.histogram(M.text(name), level, step)


def counted(ctx, src, n, level, br, step, scale):
    """The quality counts sfq_count_priors leaves for the text at src"""
    import torch
    nq, nr = capi.Context.prior_counts_words(level)
    assert nq == M.q_rows(level) * 64
    q = torch.empty(nq, dtype=torch.int32, device="cuda"); r = torch.empty(nr, dtype=torch.int32, device="cuda")
    ctx.count_priors(src.ptr, n, level=level, block_reads=br, prior_step=step, tables=FROZEN, sample_scale=scale)
    ctx.get_prior_counts(level, q.data_ptr(), r.data_ptr())
    torch.cuda.synchronize()
    return q.cpu().numpy().view(np.uint32)


def first_count_that_differs(got, want, what):
    bad = np.flatnonzero(got != want)
    assert not len(bad), "%s: %d of %d counts differ (the table's sum %d, want %d); the first: context %#x symbol %d, got %d, want %d" % (
        what, len(bad), len(want), int(got.sum(dtype=np.uint64)), int(want.sum(dtype=np.uint64)), bad[0] >> 6, bad[0] & 63, got[bad[0]], want[bad[0]])


# ---- 1. counts, count for count ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", (1, 2, 3, 4))
@pytest.mark.parametrize("name", M.TEXTS)
def test_counts_equal_the_oracles(ctx, name, level):
    t = M.text(name)
    fq = t["fq"]
    places = ((0, "ff"), (13, "fastq")) if name in M.TAILS else ((0, "ff"),)
    for off, fill in places:
        src = Placed(len(fq), off, fill, fq)
        for step in M.STEPS:
            for scale in M.SCALES:
                want = want_counts(name, level, step * scale)
                for again in range(3 if name in M.REPEATED else 1):
                    what = "%s, level %d, step %d x %d, text at +%d ('%s'), run %d" % (name, level, step, scale, off, fill, again)
                    first_count_that_differs(counted(ctx, src, len(fq), level, t["br"], step, scale), want, what)
        assert src.back(name + ": the text") == fq


# ---- 2. rows from installed counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", (1, 2, 3, 4))
def test_rows_of_installed_counts(ctx, level):
    import torch
    tb = M.table(level)
    t = M.ordinary()
    fq, br, cr = t["fq"], 64, 8
    qoff, qlen = M.lines(t)
    nq, nr = capi.Context.prior_counts_words(level)
    d = torch.from_numpy(np.frombuffer(fq, np.uint8).copy()).cuda()
    own = torch.empty(nq, dtype=torch.int32, device="cuda"); r = torch.empty(nr, dtype=torch.int32, device="cuda")
    ctx.count_priors(d.data_ptr(), len(fq), level=level, block_reads=br, prior_step=1, tables=FROZEN)       # (the header sample's counts)
    ctx.get_prior_counts(level, own.data_ptr(), r.data_ptr())
    q = torch.from_numpy(tb["counts"].view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    rows = O.qlt_prior_rows(tb["counts"])
    # frozen tables
    ctx.set_prior_counts(level, q.data_ptr(), r.data_ptr())
    enc = ctx.encode_host(fq, level=level, block_reads=br, prior_step=capi.PRIOR_COUNTS, tables=FROZEN, chain_reads=cr)
    got = util.unpack_prior(enc.prior, M.q_rows(level))
    for c in np.flatnonzero((got != rows).any(axis=1)):
        raise AssertionError("level %d: the row of context %#x (%s) differs: got %s total %d iend %d, want %s total %d iend %d" % (
            level, c, tb["kinds"].get(int(c), "the text's own"), ["%d:%d" % (s >> 16, s & 0xffff) for s in got[c, :64] if s], got[c, 64], got[c, 65],
            ["%d:%d" % (s >> 16, s & 0xffff) for s in rows[c, :64] if s], rows[c, 64], rows[c, 65]))
    want, sizes, extra = O.qlt_encode_chains(fq, qoff, qlen, level, br, cr, O.qlt_frozen_rows(rows))
    ci = util.unpack_chains(enc.chains)
    assert ci["chain_reads"] == cr
    assert_chains_equal(enc.stream("qlt"), ci["qlt"], want, sizes, "level %d frozen" % level)
    assert sum(b.extra_hi for b in enc.blocks) == extra
    assert ctx.decode_host(enc, level=level, out_cap=len(fq) + 4096) == fq
    # adaptive tables: the rows as a block's warm start, in the wave layout (60 + 4 slots) and the lane-per-block layout
    want, sizes = O.qlt_encode_blocks(fq, qoff, qlen, level, br, rows)
    for kernel in (0, 1):
        ctx.set_prior_counts(level, q.data_ptr(), r.data_ptr())
        enc = ctx.encode_host(fq, level=level, block_reads=br, prior_step=capi.PRIOR_COUNTS, tables=ADAPTIVE, kernel=kernel)
        assert np.array_equal(util.unpack_prior(enc.prior, M.q_rows(level)), rows), kernel
        assert_chains_equal(enc.stream("qlt"), [b.size[2] for b in enc.blocks], want, sizes, "level %d adaptive, kernel %d, block" % (level, kernel))
        assert ctx.decode_host(enc, level=level, out_cap=len(fq) + 4096, kernel=kernel) == fq


# ---- 3. rows of every family, given ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", (1, 3))
def test_row_families(ctx, level):
    f = M.family(level)
    fq, br, cr = f["fq"], f["br"], f["cr"]
    qoff, qlen = M.lines(f)
    want, sizes, extra = O.qlt_encode_chains(fq, qoff, qlen, level, br, cr, f["frozen"])
    ctx.set_priors(f["prior"], f["rec_prior"])
    try:
        enc = ctx.encode_host(fq, level=level, block_reads=br, prior_step=capi.PRIOR_GIVEN, tables=FROZEN, chain_reads=cr)
        assert enc.prior == f["prior"] and len(enc.blocks) == 10
        ci = util.unpack_chains(enc.chains)
        assert ci["chain_reads"] == cr and not ci["flags"] & 8
        assert_chains_equal(enc.stream("qlt"), ci["qlt"], want, sizes, "level %d" % level)
        assert sum(b.extra_hi for b in enc.blocks) == extra > 0
        for lds_rows in (capi.LDS_ROWS_NONE, 1, 300, 6000):                           # k_qlt_decode_c<256, false>; <1024, true> with one list, some, as many as fit
            back = ctx.decode_host(enc, level=level, out_cap=len(fq) + 4096, lds_rows=lds_rows)
            util.first_difference(back, fq, "level %d, decoded with lds_rows %#x" % (level, lds_rows))
    finally:
        ctx.set_priors(b"", b"")


# ---- 4. the wave histogram into a whole call ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto", (False, True))
@pytest.mark.parametrize("level", (1, 4))
def test_wave_histogram_into_a_whole_call(ctx, level, auto):
    t = M.text("wave-uniform-9")
    fq = t["fq"]
    qoff, qlen = M.lines(t)
    glen = qlen
    if auto:
        enc = ctx.encode_host(fq, level=level, block_reads=capi.BLOCK_AUTO, prior_step=capi.PRIOR_AUTO, tables=FROZEN)
    else:
        enc = ctx.encode_host(fq, level=level, block_reads=t["br"], prior_step=1, tables=FROZEN, chain_reads=SEG | 1000)
    ci = util.unpack_chains(enc.chains, len(enc.blocks))
    assert ci["flags"] & 8 and ci["chain_reads"] == 1 and (auto or ci["seg_len"] == 1000)
    seg = ci["seg_len"]
    rows = O.qlt_prior_rows(want_counts(t["name"], level, 1))                        # (nine records: the automatic step is 1)
    assert np.array_equal(util.unpack_prior(enc.prior, M.q_rows(level)), rows)
    want, sizes, extra = O.qlt_encode_segs(fq, qoff, qlen, glen, level, seg, O.qlt_frozen_rows(rows))
    assert enc.res.n_chains == int(O.seg_counts(qlen, glen, seg).sum())
    assert_chains_equal(enc.stream("qlt"), ci["qlt"], want, sizes, "level %d, segments of %d" % (level, seg))
    assert sum(b.extra_hi for b in enc.blocks) == extra > 0
    assert ctx.decode_host(enc, level=level, out_cap=len(fq) + 4096) == fq

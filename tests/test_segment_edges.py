"""GPU: chains that are SEGMENTS of one record where a record's two lines have unequal lengths, on the texts of seg_mint.py
(test_segment_inputs.py holds the texts to their claims on the CPU).  The rule -- n = ceil(max(bases, qualities) / seg_len) chains of
L = ceil(M / n) symbols, the shorter line's late chains EMPTY -- is restated in dev_walk.h (seg_count_of, seg_range, LineWalk::bounds), gm.hip
(k_gm_plan, k_gm_decode_c) and chains.hip (k_gen_pack_raw, k_qlt_decode_c, k_gen_decode_c, k_seg_count_dec); every restatement runs here.

test_segments_equal_the_oracle: every text x level 1, 3 x block_reads 4, 7, 64, SFQ_CHAIN_SEGMENT(seg), prior_step 1: the chain index's shape
(flag bit 3, seg_len, chain_reads 1, every block's share, n_chains), the quality chains and the base chains (match model or two bits a base) against
the oracle chain by chain, the three exception lists and the N byte of EVERY block against the oracle's Rice lists, and the way back into a
buffer of exactly the text's size.  The near-capacity text (seg_mint.capacity_text: two records of 1 base, 4096 ordinary qualities and 600 escapes
the prior's sample never saw; the fullest quality chain holds 115 of its region's 124 bytes, ratio 0.9274 at level 1, 0.9194 at level 3) is one of
the texts: the library takes it, writes the oracle's bytes and reads them back.
test_round_4_generation_tables_take_segments: sfq_params.kernel = 2 does take segments (api.cpp refuses nothing): k_gen_encode_c / k_gen_decode_c.
test_automatic_choice_at_the_segment_length: api.cpp's rule (a call whose chains would be single records, fewer than 204 800 of them, takes
segments where its longest BASE line exceeds the wanted length) at that length and one symbol over it.
test_untrusted_index_*: a share below the block's record count, a sum that is not the stored total, another seg_len.

Wall time on one MI355X, same machine and run: the GPU suite with this module 432 s (788 tests), without it 431 s (725 tests: the suite at the parent
commit); this module's 63 tests take 1.0 s of it (1.6 s alone), 0.05 s the slowest: a four-hundredth, where a tenth was allowed.

Checked on scratch copies of the sources, one rule changed at a time, each library run ONCE over this module and over the earlier tests that code
segments (-k "segment or long_re" over test_frozen_tables, test_gen_pack, test_gen_pack_groups, test_match_walk, test_clamp_gpu, test_placement,
test_checksums, test_text_stats: 21 earlier tests):
(the texts of that run had the 300-segment records wherever they fell; the two-symbol records that now put their empty chains on a multiple of 256
were added afterwards, and the whole GPU suite passed on the texts as they are)
  caught
    seg_range: L = M / nseg (a floor)            new: 62 of 63 -- every text x level x block size at the first quality chain compared (a WRONG BYTE: the chains
                                                 differ from the oracle's), kernel = 2, the index cases, the automatic choice with one record (the text comes
                                                 back short).  earlier: 12 fail as well (test_long_records_are_cut_into_segments x 3, test_long_reads_take_
                                                 segments_by_themselves, test_gen_pack / _groups x 4, test_placement x 3, test_checksums[segments]): their random
                                                 lengths do expose a floor.
    seg_range: sub_lo = seg * seg_len            new: 63 of 63, wrong bytes as above.  earlier: 14 fail (the 12 above and both match-model segment tests).
    k_seg_count_dec: slen alone                  new: 61 of 63 (all but the automatic choice, whose lines are equal), an ERROR RETURN: the encoder's bytes are the
                                                 oracle's, decode_host ends in SFQ_E_CORRUPT "chain index: block N's segments disagree with its records' line
                                                 lengths".  earlier: NONE fails.
    k_gm_decode_c: seg_range(cp, n_next)         new: 21 -- match-64, match-75, colour-64 at every level and block size, the three index cases of match-64 --, an
                                                 ERROR RETURN: SFQ_E_CORRUPT from the chain decoder.  earlier: NONE fails.
  judged from the code, not run (a lane would read and write outside its record's stage)
    k_gm_plan: lo = cp.sub_lo without the clamp  len - lo wraps where the base line ends before the segment starts, n becomes sub_len, and the lane plans L
                                                 bases at soff[r] + lo: the records behind it, or -- the call's last records -- what lies behind the stage.
                                                 match-64, match-75 and colour-64 hold such chains by the hundred (empty>=260:q, short=1:q, short<L:q), also in
                                                 the call's last block; the tokens of the records behind would be written twice.
  change no byte and cannot be caught
    LineWalk::bounds: b0 = lo without the min    b0 lands behind b1, the second line leaves b1 where it is, and next() reads `if (end < pos) end = pos`: no piece.
    k_gen_pack_raw's copy of it                  the same: `if (b1 < b0) b1 = b0` stands behind the copy, len = 0.
  not reachable
    the quality chains' mark by chain            k_qlt_encode_c<.., MARK = true> is launched only with a.exc_flag set, which no caller does (launch_qlt_encode_c).
"""
import numpy as np
import pytest

import seg_mint as S
import util
from oracle import oracle as O
from slimfastq_amd import capi
from test_clamp_gpu import assert_chains_equal
from test_frozen_tables import GEN_STEP, PRIOR_SYMBOLS, SEG, base_chains_oracle

pytestmark = pytest.mark.gpu
assert PRIOR_SYMBOLS == S.PRIOR_SYMBOLS
ALL = S.TEXTS + ["capacity"]


def encode(ctx, t, level, br, **kw):
    return ctx.encode_host(t["fq"], level=level, block_reads=br, prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=SEG | t["seg"], **kw)


def index_as_the_oracle_says(t, enc, br):
    """"chn.idx": segments of the text's length, one record a chain, every block's share and their sum"""
    _, _, glen, _, qlen = S.lines(t)
    nrec = len(glen)
    nblocks = -(-nrec // br)
    ci = util.unpack_chains(enc.chains, nblocks)
    assert ci["flags"] & 8 and ci["seg_len"] == t["seg"] and ci["chain_reads"] == 1 and len(enc.blocks) == nblocks
    nseg = O.seg_counts(glen, qlen, t["seg"])
    assert [int(nseg[b * br:(b + 1) * br].sum()) for b in range(nblocks)] == list(ci["seg_blocks"])
    assert enc.res.n_chains == int(nseg.sum()) == S.seg_table(t)[2][-1]
    return ci


@pytest.mark.parametrize("br", S.BRS)
@pytest.mark.parametrize("level", S.LEVELS)
@pytest.mark.parametrize("name", ALL)
def test_segments_equal_the_oracle(ctx, name, level, br):
    t = S.text(name)
    fq, solid = t["fq"], int(t["solid"])
    what = "%s level %d blocks of %d" % (name, level, br)
    enc = encode(ctx, t, level, br)
    assert enc.blocks[0].solid == solid
    ci = index_as_the_oracle_says(t, enc, br)
    _, goff, glen, qoff, qlen = S.lines(t)
    # qualities
    want, sizes, extra, _ = S.quality_oracle(name, level)
    assert_chains_equal(enc.stream("qlt"), ci["qlt"], want, sizes, what + ": qlt")
    assert sum(b.extra_hi for b in enc.blocks) == extra
    # bases: the match model, or two bits a base
    want, sizes, on = base_chains_oracle(fq, goff, glen, ci, br, 1, t["seg"], qlen)
    assert on == int(t["match"]) and (on or ci["flags"] & 128)
    assert_chains_equal(enc.stream("gen"), ci["gen"], want, sizes, what + ": gen")
    # the exception lists and the N byte of every block
    assert ci["flags"] & 16
    for b, chunk in enumerate(util.split_records(fq, br)):
        starts, lens = util.line_table(chunk)
        ns, nn, lc, n_byte = O.exc_rice_block(chunk, starts[1::4] + solid, lens[1::4] - solid, starts[3::4] + solid, lens[3::4] - solid)
        assert dict(zip(("gen.Ns", "gen.Nn", "gen.lc"), (ns, nn, lc))) == util.exc_rice_reference(chunk, solid=solid)
        for s, ref in (("gen.Ns", ns), ("gen.Nn", nn), ("gen.lc", lc)):
            assert enc.stream(s, b) == ref, (what, s, b)
        assert enc.blocks[b].n_byte == n_byte, (what, b, enc.blocks[b].n_byte, n_byte)
    assert ctx.decode_host(enc, level=level, out_cap=len(fq)) == fq, what


def test_round_4_generation_tables_take_segments(ctx):
    """sfq_params.kernel = 2 (round 4's generation tables of Base2 rows, the reference's exception coding) with chains that are segments: the entry
    does not refuse the combination, so the base chains are held to O.gen_encode_segs, and the archive decodes."""
    t = S.text("match-64")
    fq, br = t["fq"], 64
    enc = encode(ctx, t, 3, br, kernel=2)
    ci = index_as_the_oracle_says(t, enc, br)
    assert not ci["flags"] & 32 and not ci["flags"] & 16
    _, goff, glen, qoff, qlen = S.lines(t)
    want, sizes, on = O.gen_encode_segs(fq, goff, glen, qlen, enc.blocks[0].gen_bits, br, t["seg"], GEN_STEP)
    assert (ci["flags"] & 1) == on
    assert_chains_equal(enc.stream("gen"), ci["gen"], want, sizes, "generation tables over segments")
    want, sizes, extra, _ = S.quality_oracle("match-64", 3)
    assert_chains_equal(enc.stream("qlt"), ci["qlt"], want, sizes, "kernel = 2: qlt")
    assert ctx.decode_host(enc, level=3, out_cap=len(fq)) == fq


# ---- the automatic choice (api.cpp, restated) ----------------------------------------------------------------------------------------------------
CHAINS_WANT = 262144


def default_chain_reads(nrec, nbytes):
    per = max(1, nbytes // max(1, nrec))
    return min(max(1, -(-nrec // CHAINS_WANT), -(-4096 // per)), 4096)


def wanted_segment(nrec, nbytes):
    return min(max(4096, nbytes // 2 // (CHAINS_WANT - 8192 - min(nrec // 2, 100000))), 1 << 20)


def _records(lens, seed):
    rng = np.random.default_rng(seed)
    return b"".join(b"@a%d\n%s\n+\n%s\n" % (i, S._ACGT[rng.integers(0, 4, n)].tobytes(), S._QS[rng.integers(0, len(S._QS), n)].tobytes())
                    for i, n in enumerate(lens))


@pytest.mark.parametrize("nrec", (1, 3))
def test_automatic_choice_at_the_segment_length(ctx, nrec):
    """chain_reads = 0: a call whose default chains are single records (default_chain_reads gives 1: a record of 4 KiB of text or more -- ONE record
    is the smallest count at which it does) and that has fewer than 204 800 of them takes segments of wanted_segment() symbols where its longest BASE
    line is longer than that.  A longest line of exactly 4096 stays with whole records; one base (and its quality) more takes segments of 4096."""
    kw = dict(level=3, block_reads=capi.BLOCK_AUTO, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN)
    for extra in (0, 1):
        fq = _records([4096 + extra] + [4096 - 7 * i for i in range(1, nrec)], 5)
        assert default_chain_reads(nrec, len(fq)) == 1 and nrec < 204800
        want = wanted_segment(nrec, len(fq))
        assert want == 4096 and (max(util.line_table(fq)[1][1::4]) > want) == bool(extra)
        enc = ctx.encode_host(fq, **kw)
        ci = util.unpack_chains(enc.chains, len(enc.blocks))
        assert bool(ci["flags"] & 8) == bool(extra) and ci["chain_reads"] == 1
        if extra:
            assert ci["seg_len"] == want and enc.res.n_chains == nrec + 1
        else:
            assert enc.res.n_chains == nrec
        assert ctx.decode_host(enc, level=3, out_cap=len(fq)) == fq


# ---- the untrusted index ---------------------------------------------------------------------------------------------------------------------------
def _index_fields(ci_blob):
    """(the blob's integers, the place of the chain count): [chain_reads, flags, (match model: bits, records, chains,) n, seg_len, shares ...]"""
    v = util._vints(ci_blob)
    return v, 2 + (3 if v[1] & 32 else 0)


def _repacked(v):
    out = bytearray()
    for x in v:
        util.put_v(out, x)
    return bytes(out)


@pytest.mark.parametrize("name", ("flat-16", "match-64"))
@pytest.mark.parametrize("how", ("share-below-records", "sum-not-total", "other-seg-len"))
def test_untrusted_index_that_contradicts_itself_is_refused(ctx, name, how):
    """The decoder rebuilds the geometry from the line lengths it decodes and takes the blocks' shares from "chn.idx": a block's share below its record
    count (every record has a chain or more; the difference moved to the next block, so the sum stays), shares whose sum is not the stored chain
    count, and a segment length under which the records have another number of segments each end in an SfqError; the intact archive decodes after."""
    t = S.text(name)
    fq, br = t["fq"], 64
    enc = encode(ctx, t, 3, br)
    v, p = _index_fields(enc.chains)
    _, _, glen, _, qlen = S.lines(t)
    nseg = O.seg_counts(glen, qlen, t["seg"])
    assert v[p] == int(nseg.sum()) and v[p + 1] == t["seg"] and v[p + 2] == int(nseg[:br].sum()) and v[p + 3] == int(nseg[br:2 * br].sum())
    bad = list(v)
    if how == "share-below-records":
        assert all(k == 1 for k in nseg[2 * br:3 * br])      # block 2 holds one-segment records only: its share IS the bound
        bad[p + 2 + 2] -= 1; bad[p + 2 + 3] += 1
    elif how == "sum-not-total":
        bad[p + 2] += 1
    else:
        bad[p + 1] -= 1
        assert int(O.seg_counts(glen, qlen, t["seg"] - 1).sum()) != int(nseg.sum())
    forged = enc.clone()
    forged.chains = _repacked(bad)
    with pytest.raises(capi.SfqError):
        ctx.decode_host(forged, level=3, out_cap=len(fq) + 4096)
    assert ctx.decode_host(enc, level=3, out_cap=len(fq)) == fq

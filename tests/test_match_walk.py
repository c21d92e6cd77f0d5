"""GPU: the match model's walk (gm.hip gm_predict / gm_update -- one branch-free state machine in k_gm_plan, k_gm_price and k_gm_decode_c)
against the rule it must equal (sfq_oracle.c gm_walk), on the texts of match_mint.py: every transition of the walk at a chosen offset of the
pointer's window, a chosen base of the line and a chosen lane of a wavefront (test_match_inputs.py holds the texts to that on the CPU).
Every case encodes through the C ABI with frozen tables and the text's geometry, requires the match model and the oracle's index bits and chain
records in "chn.idx", compares the base chains with the oracle's chain by chain, decodes on the GPU and compares with the text.  The stage-end
and the lane texts also go through sfq_encode_blocks / sfq_decode_blocks with the text at an odd offset between guards.  No GPU decoder is
handed bytes that an encoder did not write.

Not reached here: the walk's instantiations for a stage of 4 GiB or more (gm_plan_line<false, u64>, k_gm_decode_c<TH, u64>) -- no oracle codes
a stage of that size in seconds; test_large_texts.py::test_match_model_walk_of_a_4_gib_stage takes them through a round trip, without a reference
for the coded bytes -- and gm_ld16's held address: no walk loads at or behind `cap` (match_mint.stage_end_lines says why).

Wall time on one MI355X, same machine and run: the GPU suite with this module 428 s (662 tests); this module alone 13.2 s (63 tests), 11.6 s of
them the first device-entry case (the process's first use of torch on the device).  An encode, the comparison and a decode take 0.01 - 0.07 s a
text, the segment text 0.01 s; inside the suite no case of this module is among the 25 slowest (all under 2.9 s).

Checked on scratch copies of gm.hip, one predicate or constant changed at a time, the encode half of every text against the oracle:
  caught
    W.m < GM_DROP -> <=                    drops, alphabet, colour (first at chain 52: keep:m=8 becomes a drop); no other text
    i + 1u + GM_D < n -> i + 2u + GM_D     short, long (lookup-last-eligible), all-lanes
    the limit's predicate always true      every text with a later generation but short (35 of 36): generations, segments (own record) ...
    the prefetch at o == 0                 all 36: the first shifted window is one that was never loaded (run:16 and beyond)
    the shift at o > 16                    all 36
    gm_level's m < 8 -> m <= 8             drops, alphabet, colour, runs, long, short, generations, all-lanes, unequal (a hit at m = 8 behind a kept miss)
    a pointer's first m = GM_K - 1         all 36
  changes no byte and cannot be caught
    the prefetch at o == 9                 a pointer starts at offset GM_D = 1 and moves one byte a base, on a kept miss too: it passes 9 as it
                                           passes 8, before the shift at 16.  The window arrives a base later; no text differs.
    gm_newline_ahead keeping byte 0 only   byte 0 is p itself, which is never a sentinel (gm_insert: i + 1 < len); a pointer taken with the sentinel
                                           at p + 1 stands on it at its first base, and gm_predict drops it there before the base is coded: the oracle's
                                           "refused" and "dropped at the sentinel" write the same bytes (ends: refused, 18 times, no text differs).
    i + 1u + GM_D < n -> <=                the lookup behind base n - 2 sets pend_at = n, a base the line does not have (none-one-later, no text differs).
    (W.ent >> 24) < lim -> <=              p == lim does not occur: p is sixteen bases or more into a line, lim is a line's first position.
    GM_MCAP 30                             m is compared with 4, 8, 16 and GM_DROP only: 30 and 31 are one state.
"""
import numpy as np
import pytest

import match_mint as M
import util
from slimfastq_amd import capi
from test_clamp_gpu import assert_chains_equal
from test_frozen_tables import SEG, base_chains_oracle
from test_placement import decode_placed, encode_placed

pytestmark = pytest.mark.gpu
PLACE, FILL = (13, 8), "fastq"                               # the text 13 bytes behind a sixteen-byte boundary, FASTQ going on around it


def encoded_as_the_oracle_says(t, enc):
    """The call took the match model with the oracle's index bits and chain records; its base chains are the oracle's, chain by chain"""
    fq, br = t["fq"], t["br"]
    goff, glen, other, nrec, tb, gcr = M.geometry(t)
    ci = util.unpack_chains(enc.chains, -(-nrec // br) if t["seg"] else None)
    assert ci["flags"] & 32 and ci["flags"] & 1 and bool(ci["flags"] & 8) == bool(t["seg"])
    want, sizes, on = base_chains_oracle(fq, goff, glen, ci, br, 1 if t["seg"] else min(t["cr"], br), t["seg"], other)
    assert on == 1 and ci["gm_table_bits"] == tb and ci["gen_chain_reads"] == gcr
    assert_chains_equal(enc.stream("gen"), ci["gen"], want, sizes, t["name"])


def call(t):
    return dict(level=3, block_reads=t["br"], prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=SEG | t["seg"] if t["seg"] else t["cr"])


@pytest.mark.parametrize("name", M.TEXTS)
def test_walk_equals_the_oracle_on_minted_text(ctx, name):
    t = M.text(name)
    fq = t["fq"]
    enc = ctx.encode_host(fq, **call(t))
    assert bool(enc.blocks[0].solid) == t["solid"]
    encoded_as_the_oracle_says(t, enc)
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq


@pytest.mark.parametrize("name", M.PLACED)
def test_walk_on_text_placed_at_an_odd_offset(ctx, name):
    """The same through the device entries: the text, the streams and the outputs 13 and 8 bytes behind a sixteen-byte boundary, exactly
    as long as they must be, between guards of FASTQ that must come back as they were (test_placement.py)."""
    t = M.text(name)
    fq = t["fq"]
    enc = encode_placed(ctx, fq, PLACE, FILL, name + ": sfq_encode_blocks", **call(t))
    encoded_as_the_oracle_says(t, enc)
    decode_placed(ctx, enc, fq, PLACE, FILL, name + ": sfq_decode_blocks", 3)

"""CPU: the texts of match_mint.py are what test_match_walk.py takes them for.  By the oracle's own trace of its walk (O.gm_trace: the function
that codes fills it), every text's verdict is "on", every class it claims occurs MIN times or more -- a class placed in a lane, in that lane --, and the
oracle decodes the chains it wrote back to the text's bases.  Over all texts together every event of the walk, a hit and a miss at each of
the four Fo levels, and every offset of the pointer in its window occur.  These are conditions on the inputs, not measurements."""
import numpy as np
import pytest

import match_mint as M
from oracle import oracle as O


@pytest.mark.parametrize("name", M.TEXTS)
def test_text_holds_what_it_claims(name):
    t = M.text(name)
    w = M.walk(name)
    assert w["on"] == 1
    got = M.classes(name)
    for cls in M.CLAIMS[name]:
        assert got[cls] >= M.MIN_OF.get(cls, M.MIN), (name, cls, got[cls])
    # a kept miss leaves m at 0: the base behind it, if the line has one, is predicted at level 0
    kept = np.flatnonzero(w["miss"] & ((w["ev"] & O.GMT_DROP_MISS) == 0))
    nxt = kept[w["have"][kept + 1]]
    assert (w["m"][nxt + 1] == 0).all() and ((w["tok"][nxt + 1] >> 2) & 3 == 0).all()
    if not t["seg"]:                                         # (the oracle's way back takes whole-record chains)
        goff, glen, other, nrec, tb, gcr = M.geometry(t)
        streams, sizes, on = O.gm_encode_chains(t["fq"], goff, glen, tb, t["br"], gcr)
        assert on == 1
        back = O.gm_decode_chains(streams, sizes, glen, tb, t["br"], gcr)
        assert np.array_equal(back, w["b"][~w["sent"]])


def test_stage_end_texts_end_in_one_record_that_copies_the_tail_before_it():
    for n in M.STAGE_END:
        lines = M.text("stage-end-%d" % n)["fq"].split(b"\n")[1::4]
        assert len(lines) == 129 and len(lines[-1]) == n and lines[-2].endswith(lines[-1])
        w = M.walk("stage-end-%d" % n)
        last = slice(int(w["soff"][128]), int(w["soff"][129]) - 1)
        assert (w["ptr"][last][w["have"][last]] >= w["soff"][127]).all()          # the pointer walks the record before it


def test_all_texts_together_reach_every_transition():
    seen = set()
    for name in M.TEXTS:
        seen |= M.coverage(name)
    assert seen >= M.COVERAGE, sorted(M.COVERAGE - seen)
    assert len(M.PLACED) == len(M.STAGE_END) + 5

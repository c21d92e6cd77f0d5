"""CPU: the texts of seg_mint.py are what test_segment_edges.py takes them for, and the oracle's segment geometry (sfq_oracle.c seg_geometry)
equals a second statement of the rule that shares no code with it.  Every text holds every class it claims, MIN times or more, counted by
seg_mint.classes() from the line lengths and letters alone; the match model's verdict is what the variant says, for every block size the GPU
test uses.  Every quality line is cut in plain Python (seg_mint.cut / piece) and every slice coded as a chain of one record of its own
(O.qlt_encode_chains: a segment starts as a line does): back to back these are the bytes and sizes of O.qlt_encode_segs, an empty slice is
0 bytes.  The flat texts' base slices, packed two bits a base in numpy, are O.gm_encode_segs' chains.  The oracle decodes its quality chains
back to the text.  No chain of any text fills its output region (chain_region, restated in seg_mint.regions); the near-capacity text's
fullest chain reaches seg_mint.CAPACITY_RATIO of it.  These are conditions on the inputs, measured on the oracle, not on the GPU."""
import numpy as np
import pytest

import seg_mint as S
from oracle import oracle as O

ALL = S.TEXTS + ["capacity"]


@pytest.mark.parametrize("name", S.TEXTS)
def test_text_holds_what_it_claims(name):
    t = S.text(name)
    got = S.classes(name)
    for cls in S.claims(name):
        assert got.get(cls, 0) >= S.MIN_OF.get(cls, S.MIN), (name, cls, got.get(cls, 0))
    assert len(t["fq"]) < 256 << 10                          # (four records of 300 segments of 75 symbols are 90 KB of it)
    if t["solid"]:                                           # every block says "colour space" by its first record (usrs.cpp:239-257)
        bases = t["fq"].split(b"\n")[1::4]
        assert all(bases[r][1:2] in (b"0", b"1", b"2", b"3") for br in t["brs"] for r in range(0, len(bases), br))
    nrec = len(S.seg_table(t)[0])
    for br in t["brs"]:
        assert nrec % br and S.base_oracle(name, br)[2] == int(t["match"]), (name, br)


def test_every_line_length_class_is_in_every_variant():
    for variant in ("match", "flat", "colour"):
        for cls in S.LENGTH_CLASSES:
            assert any(S.classes(n).get(cls, 0) >= S.MIN for n in S.TEXTS if n.startswith(variant)), (variant, cls)
    assert {S.text(n)["seg"] for n in S.TEXTS} == set(S.SEGS)
    ends = {k for n in S.TEXTS for k in S.classes(n) if k.startswith("last:")}
    assert ends == {"last:long", "last:short"}


@pytest.mark.parametrize("name", ALL)
def test_segment_counts_equal_the_second_statement(name):
    t = S.text(name)
    _, _, glen, _, qlen = S.lines(t)
    n, L, off = S.seg_table(t)
    assert list(O.seg_counts(glen, qlen, t["seg"])) == n
    for g, q, k, l in zip(glen.tolist(), qlen.tolist(), n, L):        # the segments cover both lines, and the last one is not empty in the longer
        M = max(g, q)
        assert S.piece(M, k - 1, l)[1] == M and S.piece(M, k - 1, l)[0] < M and S.piece(M, 0, l)[0] == 0


@pytest.mark.parametrize("level", S.LEVELS)
@pytest.mark.parametrize("name", ALL)
def test_quality_slices_coded_alone_are_the_oracles_segments(name, level):
    t = S.text(name)
    fq = t["fq"]
    _, _, glen, qoff, qlen = S.lines(t)
    want, sizes, extra, rows = S.quality_oracle(name, level)
    n, L, off = S.seg_table(t)
    offs, cnts = [], []
    for r, (k, l) in enumerate(zip(n, L)):
        for s in range(k):
            lo, hi = S.piece(int(qlen[r]), s, l)
            offs.append(int(qoff[r]) + lo); cnts.append(hi - lo)
    got, gsz, gextra = O.qlt_encode_chains(fq, np.array(offs, np.uint64), np.array(cnts, np.uint32), level, 1, 1, rows)
    assert list(gsz) == list(sizes) and got == want and gextra == extra
    assert all(sz == 0 for sz, c in zip(sizes, cnts) if c == 0) and (cnts.count(0) >= 2 or name == "capacity")
    assert all(sz > 0 for sz, c in zip(sizes, cnts) if c)
    # and the way back
    back = O.qlt_decode_segs(want, sizes, qoff, qlen, glen, level, t["seg"], rows)
    for o, ln in zip(qoff.tolist(), qlen.tolist()):
        assert back[o:o + ln] == fq[o:o + ln]


@pytest.mark.parametrize("name", [n for n in ALL if not S.text(n)["match"]])
def test_flat_base_slices_packed_alone_are_the_oracles_segments(name):
    """two bits a base, four a byte, the first in the low bits, the last byte padded with zeros; an N-like base codes as 0"""
    t = S.text(name)
    a = np.frombuffer(t["fq"], np.uint8)
    _, goff, glen, _, qlen = S.lines(t)
    code = np.zeros(256, np.uint8)
    for ch, v in zip("ACGTacgt0123", [0, 1, 2, 3] * 3):
        code[ord(ch)] = v
    n, L, off = S.seg_table(t)
    want = bytearray(); sizes = []
    for r, (k, l) in enumerate(zip(n, L)):
        for s in range(k):
            lo, hi = S.piece(int(glen[r]), s, l)
            c = code[a[int(goff[r]) + lo:int(goff[r]) + hi]]
            c = np.concatenate([c, np.zeros(-len(c) % 4, np.uint8)]).reshape(-1, 4)
            by = (c[:, 0] | c[:, 1] << 2 | c[:, 2] << 4 | c[:, 3] << 6).astype(np.uint8)
            want += by.tobytes(); sizes.append(len(by))
    for br in t["brs"]:
        got, gsz, on = S.base_oracle(name, br)
        assert on == 0 and list(gsz) == sizes and got == bytes(want)
    assert sizes.count(0) >= 2


@pytest.mark.parametrize("name", ALL)
def test_no_chain_fills_its_region(name):
    t = S.text(name)
    for br in t["brs"]:
        assert S.fill_ratio(S.base_oracle(name, br)[1], S.regions(t, br, 3, 4)) < 1
        for level in S.LEVELS:
            assert S.fill_ratio(S.quality_oracle(name, level)[1], S.regions(t, br, 2, 1)) < 1


def test_near_capacity_text_is_near_capacity():
    top = max(S.capacity_ratio(level, br) for level in S.LEVELS for br in S.BRS)
    print("near-capacity text: the fullest quality chain holds %.4f of its region" % top)
    assert 0.7 <= top < 1
    assert abs(top - S.CAPACITY_RATIO) < 0.001
    t = S.text("capacity")
    _, _, glen, _, qlen = S.lines(t)
    assert sum(1 for g, q in zip(glen, qlen) if g == 1 and q > 4000) == len(S.CAPACITY["at"])

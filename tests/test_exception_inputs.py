"""exc_mint.py held to its word, on the CPU: the Python statement of the base-exception lists (positions, rice_encode, rice_decode) against the
oracle's C (sfqo_exc_rice_block, sfqo_exc_rice_decode) on every block of every minted text, and every edge a text claims to reach asserted from
rice_encode's report, marked() and queue_peaks().  A text that stops reaching its edge fails here, before the GPU sees it.

The two far texts go through O.exc_rice_block as well: one pass over 34.6 M bases in C, 0.3 s of host time -- within "a few seconds", so the comparison
is on the oracle's own bytes, not only on what its decoder makes of the Python bytes."""
import numpy as np
import pytest

import exc_mint as M
import util
from oracle import oracle as O
from test_frozen_tables import gm_chain_reads, gm_table_bits


def _pairs():
    return [(name, br) for name in M.SMALL for br, _ in M.text(name)["geos"]]


@pytest.mark.parametrize("name,br", _pairs())
def test_the_python_rule_writes_the_oracles_lists_in_every_block(name, br):
    t = M.text(name)
    for b, (chunk, (want, n_byte, nbases)) in enumerate(zip(M.block_chunks(t, br), M.lists(name, br))):
        starts, lens = util.line_table(chunk)
        s = t["solid"]
        ref = O.exc_rice_block(chunk, starts[1::4] + s, lens[1::4] - s, starts[3::4] + s, lens[3::4] - s)
        assert n_byte == ref[3], (name, b)
        pos = M.positions(chunk, s)
        for i, ln in enumerate(M.NAMES):
            util.first_difference(want[ln][0], ref[i], "%s block %d %s" % (name, b, ln))
            assert np.array_equal(O.exc_rice_decode(want[ln][0]), pos[ln].astype(np.uint64)), (name, b, ln)
            assert np.cumsum(M.rice_decode(ref[i])).tolist() == pos[ln].tolist(), (name, b, ln)
            assert M.verdict(ref[i], nbases) == "ok"


@pytest.mark.parametrize("name", ("far-20", "far-25"))
def test_far_gaps_against_the_oracle(name):
    t = M.text(name)
    (want, n_byte, nbases), = M.lists(name, t["nrec"])
    starts, lens = util.line_table(t["fq"])
    ref = O.exc_rice_block(t["fq"], starts[1::4], lens[1::4], starts[3::4], lens[3::4])
    assert n_byte == ref[3] == ord("N") and nbases == t["nrec"] * M.EDGE_LEN
    for i, ln in enumerate(M.NAMES):
        assert want[ln][0] == ref[i], (name, ln)
        pos = t["claims"][ln]
        assert np.cumsum(M.rice_decode(ref[i])).tolist() == pos.tolist()
        assert O.exc_rice_decode(want[ln][0]).tolist() == pos.tolist()
    for ln in M.NAMES:
        assert [v for v, _, _ in want[ln][1]["steps"]] == list(M.FAR[name]["lists"][ln])
    first = {ln: want[ln][1]["steps"][0] for ln in M.NAMES}
    if name == "far-20":
        # 2^20 - 1 fills the escape's low field and leaves the upper one 0; 2^20 is the upper field's first bit; 2^21 + 3 has bits in both
        assert first == {"gen.Ns": ((1 << 20) - 1, 8, 4095), "gen.Nn": (1 << 20, 8, 4096), "gen.lc": ((1 << 21) + 3, 8, 8192)}
        assert [want[ln][1]["upper"] for ln in M.NAMES] == [False, True, True] and all(want[ln][1]["escapes"] == 1 for ln in M.NAMES)
    else:
        # the first event lies more than 2^25 bases in: behind it A = 256 + 2^25 + 5 and N = 2, so the rule asks for k = 25 and the code clamps
        rep = want["gen.Ns"][1]
        A, N = M.RICE_A0 + rep["steps"][0][0], 2
        assert rep["steps"][0][0] > 1 << 25 and M.rice_k(A, N, kmax=99) == 25 and rep["upper"] and rep["escapes"] == 1
        assert all([k for _, k, _ in want[ln][1]["steps"]] == [8, 24, 24] for ln in M.NAMES)


def test_the_clamp_is_the_oracles():
    """One list that needs k = 25 unclamped (far-25's): a coder that lets k reach 25 writes other bytes, the clamped bytes are the oracle's."""
    t = M.text("far-25")
    gaps = list(M.FAR["far-25"]["lists"]["gen.Ns"])
    starts, lens = util.line_table(t["fq"])
    ref = O.exc_rice_block(t["fq"], starts[1::4], lens[1::4], starts[3::4], lens[3::4])[0]
    assert M.rice_encode(gaps)[0] == ref
    loose = _encode_with_kmax(gaps, 25)[0]
    assert loose != ref and O.exc_rice_decode(loose).tolist() != np.cumsum(gaps).tolist()


def _encode_with_kmax(gaps, kmax):
    """rice_encode with another clamp (its rice_k takes the clamp as a default argument: patched for the call)"""
    keep = M.rice_k.__defaults__
    M.rice_k.__defaults__ = (kmax,)
    try:
        return M.rice_encode(gaps)
    finally:
        M.rice_k.__defaults__ = keep


def test_edges_reaches_what_it_claims():
    t = M.text("edges")
    br = t["geos"][0][0]
    L = M.lists("edges", br)
    assert len(L) == len(t["plan"]) and all(nb == M.EDGE_B for _, _, nb in L)
    for b, lists in enumerate(t["plan"]):                     # every block holds the lists it was planned with
        pos = M.positions(M.block_chunks(t, br)[b], 0)
        for ln in M.NAMES:
            assert pos[ln].tolist() == np.asarray(lists[ln], np.int64).tolist(), (b, ln)
    rep = lambda claim: L[t["claims"][claim][0]][0][t["claims"][claim][1]][1]
    blob = lambda claim: L[t["claims"][claim][0]][0][t["claims"][claim][1]][0]
    assert rep("first gap 8191: q = 31 at k = 8, no escape")["steps"] == [(8191, 8, 31)] and rep("first gap 8191: q = 31 at k = 8, no escape")["q31"]
    assert rep("first gap 8192: escape at k = 8")["steps"] == [(8192, 8, 32)] and rep("first gap 8192: escape at k = 8")["escapes"] == 1
    assert len(blob("first gap 8192: escape at k = 8")) == 11                         # 32 + 40 bits, then the end mark: a zero bit and thirteen more
    r = rep("gap 31 at k = 0: q = 31")
    assert r["steps"][-1] == (31, 0, 31) and r["escapes"] == 0 and [v for v, _, _ in r["steps"][:-1]] == [1] * M.K0_RUN
    assert [k for _, k, _ in r["steps"]].index(0) <= 143                               # 143 unit gaps bring k down to 0
    r = rep("gap 32 at k = 0: escape")
    assert r["steps"][-1] == (32, 0, 32) and r["escapes"] == 1 and not r["upper"]
    assert t["claims"]["gap 31 at k = 0: q = 31"][0] != t["claims"]["gap 32 at k = 0: escape"][0]
    for n in (1, 31, 32, 33):                                 # N reaches 32 with the 31st entry: both halved there
        assert len(rep("%d entr%s" % (n, "y" if n == 1 else "ies"))["steps"]) == n
    assert rep("bits = 0 mod 8")["bits"] % 8 == 0 and rep("bits = 0 mod 8")["bits"] > 0
    assert rep("bits = 0 mod 32")["bits"] % 32 == 0 and rep("bits = 0 mod 32")["bits"] > 32
    assert rep("bits = 31 mod 32")["bits"] % 32 == 31
    assert sum(1 for b in L for ln in M.NAMES if b[0][ln][1]["bits"] % 32 == 31) >= 2
    for claim in ("dense Nn", "dense lc"):
        assert [v for v, _, _ in rep(claim)["steps"]] == [1] * M.EDGE_B and 0 in rep(claim)["ks"]
    same = [blob("same list as " + k) for k in ("Ns", "Nn", "lc")]
    assert same[0] == same[1] == same[2] and len(same[0]) > 40
    b = t["claims"]["n in two lists"][0]
    pos = M.positions(M.block_chunks(t, br)[b], 0)
    assert set(pos["gen.Ns"]) <= set(pos["gen.lc"]) and len(pos["gen.Ns"]) == 2 and pos["n_byte"] == ord("N")
    b = t["claims"]["no event"][0]
    assert all(L[b][0][ln][0] == b"" for ln in M.NAMES) and L[b][1] == 0
    assert {0, 8} <= set().union(*(x[0][ln][1]["ks"] for x in L for ln in M.NAMES))


@pytest.mark.parametrize("name", M.QUEUES)
def test_queue_blocks_hold_the_marked_records_they_claim(name):
    t = M.text(name)
    flags = M.marked(t["fq"])
    c = t["claims"]
    if name == "queue-colour":
        assert flags.all()                                    # the quality line's leading '!'
        flags = c["marked"]                                   # ... the records WITH an event are still laid out as the plan says
    else:
        assert np.array_equal(flags, c["marked"])
    br = t["geos"][0][0]
    per = [flags[i:i + br] for i in range(0, len(flags), br)]
    assert [int(p.sum()) for p in per] == M.QUEUE_MARKED
    assert [M.queue_peaks(p)[0] for p in per] == M.QUEUE_PEAK and max(M.QUEUE_PEAK) == 127          # 63 waiting, 64 more: the fullest the queue gets
    assert M.queue_peaks(per[8]) == (127, [64, 64, 63])
    sizes = {len(p) % 64 for p in per} | {len(flags[i:i + g]) % 64 for g, _ in t["geos"][1:] for i in range(0, len(flags), g)}
    assert {0, 1, 63} <= sizes
    assert per[M.QUEUE_ALL].all() and per[-1].all() and len(per[-1]) == 65
    # the record kinds, counted from the text
    lines = t["fq"].split(b"\n")
    s = t["solid"]
    seen = set()
    for r, kind in c["kinds"].items():
        head, g, q = lines[4 * r], lines[4 * r + 1][s:], lines[4 * r + 3][s:]
        n = M.event_count(g, q)
        seen.add(kind)
        assert r // br == M.QUEUE_ALL and r % br < 192
        if kind in ("8 events", "9 events", "90 events"):
            assert n == int(kind.split()[0]) and len(g) <= 1024
        elif kind.startswith("ninth"):
            ev = [i for i in range(len(g)) if M.event_count(g[i:i + 1], q[i:i + 1])]
            assert n == 9 and ev[8] >= 16 * ((len(g) - 1) // 16) > ev[7]
        elif kind in ("1024 bases", "1025 bases"):
            assert len(g) == int(kind.split()[0]) and 0 < n <= 8
        elif kind.startswith("no event"):
            assert n == 0 and len(q) > len(g) and b"!" in q[len(g):] and b"!" not in q[:len(g)]
        elif kind == "short quality line":
            nxt = lines[4 * r + 4]
            beyond = (q + b"\n" + nxt)[len(q):len(g)]          # what lies where the missing qualities would
            assert len(q) < len(g) and beyond.count(b"!") >= 8 and c["kinds"][r + 1] == "header of '!'"
            assert any(ch in b"Nn." for ch in g[len(q):]) and (s or any(ch >= 0x61 for ch in g[len(q):]))
    assert seen == set(M.QUEUE_KINDS.values())
    assert any(c["kinds"].get(r + 1) == "1025 bases" and r % br // 64 == (r + 1) % br // 64 for r, v in c["kinds"].items() if v == "9 events")
    want = ord("N") if name == "queue" else ord(".")
    assert {nb for _, nb, _ in M.lists(name, br)} == {0, want}
    if name == "queue":
        assert b"n" in b"".join(lines[1::4])


@pytest.mark.parametrize("name", ("ragged-flat", "ragged-match"))
def test_ragged_blocks_put_events_where_they_claim(name):
    t = M.text(name)
    br = t["geos"][0][0]
    starts, lens = util.line_table(t["fq"])
    glen = lens[1::4].astype(np.int64)
    assert glen[0] == glen[2 * br - 1] == M.RAGGED_GIANT < 65534 and len(glen) == 3 * br and glen[1:2 * br - 1].max() <= 5 and glen[1:2 * br - 1].min() == 1
    assert (glen[1 + M.RAGGED_ONES[0]:1 + M.RAGGED_ONES[1]] == 1).all()
    L = M.lists(name, br)
    every = [set(np.concatenate([np.cumsum(M.rice_decode(L[b][0][ln][0])) for ln in M.NAMES]).astype(np.int64).tolist()) for b in (0, 1)]
    lc = [set(np.cumsum(M.rice_decode(L[b][0]["gen.lc"][0])).tolist()) for b in (0, 1)]
    for what, places in t["claims"]["where"].items():
        assert {b for b, _ in places} == {0, 1}, what
        for b, p in places:
            assert p in lc[b] and 1 <= p <= L[b][2], (what, b, p)
    w = t["claims"]["where"]
    assert (0, 1) in w["block's first base"] and (1, 1) in w["block's first base"]
    assert (0, L[0][2]) in w["block's last base"] and (1, L[1][2]) in w["block's last base"]
    assert (0, M.RAGGED_GIANT) in w["giant's last base"] and (0, M.RAGGED_GIANT + 1) in w["neighbour's first base"]
    assert (1, L[1][2] - M.RAGGED_GIANT + 1) in w["giant's first base"] and (1, L[1][2] - M.RAGGED_GIANT) in w["neighbour's last base"]
    for b in (0, 1):
        assert all(len(L[b][0][ln][1]["steps"]) >= 5 for ln in M.NAMES), b        # all three lists carry positions
    # the record a position lies in is far from the guess by the block's mean line length, on either side (exc.hip rec_of)
    for b in (0, 1):
        g = glen[b * br:(b + 1) * br]
        first = np.cumsum(g) - g
        off = [int(np.searchsorted(first, p - 1, side="right") - 1) - (p - 1) * br // int(g.sum()) for p in sorted(every[b])]
        assert (min(off) < -1000) if b == 0 else (max(off) > 1000), (b, min(off), max(off))
    # which stage the decoder will use: the match model's verdict, by the oracle
    goff = starts[1::4]
    fq = t["fq"]
    gcr = gm_chain_reads(len(fq), len(goff), br, t["geos"][0][1])
    on = O.gm_encode_chains(fq, goff, lens[1::4], gm_table_bits(len(fq)), br, gcr)[2]
    assert bool(on) == t["claims"]["match"]


def test_rice_python_coder_and_decoder_agree_on_random_lists():
    """A few thousand lists whose gaps mix scales from 1 to 2^30, so that k moves both ways, through rice_encode and rice_decode -- and, every
    eighth list, through the oracle's decoder."""
    rng = np.random.default_rng(2024)
    ks, esc, upper = set(), 0, 0
    for i in range(3000):
        n = int(rng.integers(1, 80)) if i % 10 else int(rng.integers(150, 400))
        scale = rng.choice([0, 3, 8, 14, 20, 25, 30], n if i % 3 else 1)
        gaps = (1 + (rng.integers(0, 1 << 62, n) >> (62 - np.resize(scale, n)).astype(np.int64))).tolist()
        blob, rep = M.rice_encode(gaps)
        assert M.rice_decode(blob) == gaps
        assert (rep["bits"] + 7) // 8 <= len(blob) <= (rep["bits"] + 25 + 7) // 8
        ks |= rep["ks"]; esc += rep["escapes"]; upper += rep["upper"]
        if i % 8 == 0:
            assert O.exc_rice_decode(blob).tolist() == np.cumsum(gaps).tolist()
    assert {0, 8, 24} <= ks and len(ks) >= 20 and esc > 500 and upper > 100
    assert M.rice_encode([]) == (b"", dict(ks=set(), escapes=0, upper=False, q31=False, bits=0, steps=[])) and M.rice_decode(b"") == []
    # the gaps the issue names, against the oracle's decoder
    for g in (8191, 8192, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 25) + 5):
        for tail in ([], [1], [g]):
            blob, _ = M.rice_encode([g] + tail)
            assert O.exc_rice_decode(blob).tolist() == np.cumsum([g] + tail).tolist()


def test_damaged_lists_as_the_python_decoder_reads_them():
    """What test_exception_lists.py's damaged archives hold, decided here: a list overwritten with 0xFF is an escape to a position of 2^40 - 1;
    a list whose end mark and padding are ones runs out of its stream."""
    blob, rep = M.rice_encode([5, 1000, 70])
    assert M.verdict(b"\xff" * 9, 10 ** 7) == "position beyond the block" and next(M.rice_gaps(b"\xff" * 9)) == (1 << 40) - 1
    bad = int.from_bytes(blob, "little") | (((1 << (8 * len(blob) - rep["bits"])) - 1) << rep["bits"])
    assert M.verdict(bad.to_bytes(len(blob), "little"), 10 ** 7) == "end outside the stream"
    with pytest.raises(M.RiceError):
        M.rice_decode(bad.to_bytes(len(blob), "little"))

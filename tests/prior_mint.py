"""Inputs that take the quality prior's chain of kernels to its edges AT CHOSEN PLACES: built, not drawn.  The chain: a sample histogram
(prior.hip k_qlt_hist, a lane per record; k_qlt_hist_w, a wave per record, where the mean record is over 4000 bytes), the prior's rows
(k_prior_rows), the blob "qlt.pri" and the way back (k_prior_flags / k_prior_slots / k_prior_gather, pack_prior / unpack_prior,
k_prior_scatter), the frozen rows and the decoder's form of them (chains.hip k_qlt_frozen_rows, qdec_store), and the quality decoder's two
sixteen-byte searches over that form (k_qlt_decode_c).  Four kinds of input, each a function of its name and of fixed seeds, cached:

  text(name)      FASTQ for the histograms: dict(name, fq, br, solid).  LANE_TEXTS have a mean record of 4000 bytes or less, WAVE_TEXTS more.
  table(level)    count tables for sfq_set_prior_counts: dict(counts, kinds: context -> kind of row, shifts: context -> the scaling shift).
  family(level)   prior rows of chosen shapes (rows66, packed with clamp_mint.pack_prior), the text coded under them, and its header prior.
  claims(name) / classes(name)   what an input is meant to reach, counted from the oracle's own results (O.qlt_histogram, O.qlt_prior_rows,
                  O.qlt_frozen_rows); test_prior_inputs.py holds every input to its claims on the CPU, test_prior_edges.py runs them on the GPU.

The classes:
  crowded:L            at level L every workgroup of HIST_T = 256 sampled records holds more than HIST_S = 16 384 distinct (context, symbol)
                       keys: hist_add's probes run out and the key is counted straight in memory
  hot:L                some key occurs 768 times or more among one workgroup's records: the harvest at 256 and the "count in memory" arm
  workgroups:N         the sample at step 1 is N workgroups of the kernel that takes the text
  last-wg-one-record   the last workgroup holds one record
  tail:K:L             the last record's quality line starts K bytes behind a four-byte boundary of the text, is L symbols long, and that
                       record is sampled at every step the tests use (1, 2, 3, 6)
  len:L                a quality line of L symbols
  escapes              symbols of 63 and more (the counted symbol is clamped to 63, the context takes the raw value)
  mean-over-4000 / mean-at-most-4000   which kernel launch_qlt_hist picks
  d3-early / d3-late   level 3's delta saturates (d3 = 7) inside a line's first 64 symbols / only behind them (the wave kernel's carried sum)
  solid                colour space: every quality line's first symbol belongs to the primer base and is not counted
"""
import functools

import numpy as np

import util
from oracle import oracle as O
from clamp_mint import PRIOR_SYMBOLS, is_legal, pack_prior, pack_rec_prior, q_rows, rec_sample

HIST_T, HIST_S = 256, 16384                                  # prior.hip: records a workgroup of k_qlt_hist, slots of its table
WAVE_WG = 4                                                  # records a workgroup of k_qlt_hist_w
STEPS, SCALES = (1, 3), (1, 2)                               # prior_step x sample_scale of the count cases
MIN = 16                                                     # times a (family member, symbol) must occur (match_mint.MIN)
TAIL_LENS = (1, 2, 3, 5, 16, 17)
LANE_LENS = (1, 2, 3, 15, 16, 17, 4095, 4096, 4097, 6000)
WAVE_LENS = (1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8192)
_ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---- texts -------------------------------------------------------------------------------------------------------------------------------------
def _record(name, i, bases, quals, solid=False, pad=0):
    if solid:
        bases, quals = b"T" + bytes(b"0123"[c & 3] for c in bases), b"!" + quals
    return b"@%s.%d%s\n%s\n+\n%s\n" % (name.encode(), i, b"x" * pad, bases, quals)


def _assemble(name, quals, br, seed, solid=False, pads=None):
    """quals: the quality lines (bytes, without a colour-space primer's symbol) -> dict(name, fq, br, solid)"""
    rng = np.random.default_rng(seed)
    recs = []
    for i, q in enumerate(quals):
        b = _ACGT[rng.integers(0, 4, len(q))].tobytes()
        recs.append(_record(name, i, b, q, solid, pads[i] if pads else 0))
    return dict(name=name, fq=b"".join(recs), br=br, solid=solid)


def uniform(rng, n, lo=33, hi=126):
    return rng.integers(lo, hi + 1, n, dtype=np.uint8).tobytes()


def walk(rng, n):
    """a random walk clipped to '"' .. ']' (what the suite's long reads have)"""
    return (np.clip(np.cumsum(rng.integers(-2, 3, n)) + 20, 1, 60) + 33).astype(np.uint8).tobytes()


def binned(rng, n):
    """four quality values, one of them seven symbols in ten"""
    return np.frombuffer(b"F:,#", np.uint8)[rng.choice(4, n, p=(0.7, 0.15, 0.1, 0.05))].tobytes()


def drops(rng, n, at):
    """a quiet walk with falls of 30 and more at the places `at`: level 3's delta grows by each fall"""
    q = np.clip(np.cumsum(rng.integers(0, 2, n)) % 3 + 70, 34, 126)
    for a in at:
        if a + 1 < n:
            q[a], q[a + 1] = 75, 36
    # (the walk itself falls by 2 once in about six symbols: some 20 in a line's first 64, short of the 51 that saturate d3)
    return q.astype(np.uint8).tobytes()


def _tail_text(name, k, L):
    """13 records (the last is record 12: sampled at steps 1, 2, 3 and 6); an earlier header padded until the last quality line starts k
    bytes behind a four-byte boundary"""
    rng = np.random.default_rng(1000 + 10 * k + L)
    quals = [uniform(rng, 20 + i) for i in range(12)] + [uniform(rng, L, 34, 90)]     # (no escape in the last line: a byte read as 0 counts as one)
    for pad in range(4):
        t = _assemble(name, quals, 8, 7, pads=[pad if i == 5 else 0 for i in range(13)])
        starts, _ = util.line_table(t["fq"])
        if int(starts[-1]) % 4 == k:
            return t
    raise AssertionError(name)


# the wave texts' line lengths: the special ones among records of 5 000 .. 9 000 symbols that keep the mean over 4000 bytes
_WAVE_SHAPES = {
    9: (8192, 63, 64, 9000, 65, 127, 7000, 128, 1),
    8: (129, 4095, 9000, 4096, 4097, 8000, 6000, 5000),
    5: (1, 64, 8192, 5000, 9000),
}


def _build(name):
    seed = sum(name.encode()) * 1009 + len(name)
    rng = np.random.default_rng(seed)
    if name in ("crowded", "crowded+1"):                     # two workgroups; a further record makes three, the last holding one record
        return _assemble(name, [uniform(rng, 150) for _ in range(512 + (name == "crowded+1"))], 256, 1)
    if name == "hot":
        return _assemble(name, [binned(rng, 150) for _ in range(2048)], 256, 2)
    if name.startswith("tail-"):
        _, k, L = name.split("-")
        return _tail_text(name, int(k), int(L))
    if name == "lens":
        quals = []
        for rep in range(2):
            quals += [uniform(rng, L) if rep else walk(rng, L) for L in LANE_LENS]
            quals += [uniform(rng, 150) for _ in range(10)]
        return _assemble(name, quals, 16, 3)
    if name == "colour":
        return _assemble(name, [uniform(rng, 1 + (i * 7) % 120) for i in range(300)], 64, 4, solid=True)
    if name.startswith("wave-"):
        _, kind, n = name.split("-")
        shape = _WAVE_SHAPES[int(n)]
        if kind == "uniform":
            quals = [uniform(rng, L) for L in shape]
        elif kind == "walk":
            quals = [walk(rng, L) for L in shape]
        elif kind == "drops":                                # falls inside the first 64 symbols and again later; or only behind symbol 64
            quals = [drops(rng, L, (5, 20, 40, 300, 1000, 4000) if i % 2 == 0 else (70, 100, 131, 200, 2000)) for i, L in enumerate(shape)]
        elif kind == "colour":
            return _assemble(name, [uniform(rng, L) for L in shape], 4, 5, solid=True)
        else:
            raise KeyError(name)
        return _assemble(name, quals, 4, 5)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def text(name):
    return _build(name)


TAILS = ["tail-%d-%d" % (k, L) for k in range(4) for L in TAIL_LENS]
LANE_TEXTS = ["crowded", "crowded+1", "hot", "lens", "colour"] + TAILS
WAVE_TEXTS = ["wave-uniform-9", "wave-uniform-8", "wave-uniform-5", "wave-walk-9", "wave-walk-8", "wave-walk-5", "wave-drops-8", "wave-colour-5"]
TEXTS = LANE_TEXTS + WAVE_TEXTS
REPEATED = ("crowded", "crowded+1", "hot")                   # counted three times over: the atomics' order must not show

CLAIMS = {
    "crowded": ["crowded:%d" % l for l in (1, 2, 3, 4)] + ["workgroups:2", "escapes", "mean-at-most-4000"],
    "crowded+1": ["crowded:%d" % l for l in (1, 2, 3, 4)] + ["workgroups:3", "last-wg-one-record", "mean-at-most-4000"],
    "hot": ["hot:%d" % l for l in (1, 2, 3, 4)] + ["workgroups:8", "mean-at-most-4000"],
    "lens": ["len:%d" % L for L in LANE_LENS] + ["escapes", "mean-at-most-4000"],
    "colour": ["solid", "escapes", "mean-at-most-4000"],
    "wave-uniform-9": ["len:%d" % L for L in _WAVE_SHAPES[9]] + ["workgroups:3", "last-wg-one-record", "escapes", "mean-over-4000"],
    "wave-uniform-8": ["len:%d" % L for L in _WAVE_SHAPES[8]] + ["workgroups:2", "escapes", "mean-over-4000"],
    "wave-uniform-5": ["len:%d" % L for L in _WAVE_SHAPES[5]] + ["workgroups:2", "last-wg-one-record", "escapes", "mean-over-4000"],
    "wave-walk-9": ["len:%d" % L for L in _WAVE_SHAPES[9]] + ["mean-over-4000"],
    "wave-walk-8": ["len:%d" % L for L in _WAVE_SHAPES[8]] + ["mean-over-4000"],
    "wave-walk-5": ["len:%d" % L for L in _WAVE_SHAPES[5]] + ["mean-over-4000"],
    "wave-drops-8": ["d3-early", "d3-late", "mean-over-4000"],
    "wave-colour-5": ["solid", "escapes", "mean-over-4000"],
}
for _n in TAILS:
    CLAIMS[_n] = ["tail:%s:%s" % tuple(_n.split("-")[1:]), "mean-at-most-4000"]


def lines(t):
    """(qoff, qlen) of the counted part of every quality line: without a colour-space primer's symbol"""
    starts, lens = util.line_table(t["fq"])
    s = int(t["solid"])
    return starts[3::4] + np.uint64(s), lens[3::4] - np.uint32(s)


def histogram(t, level, step=1, first=0, cap=PRIOR_SYMBOLS):
    qoff, qlen = lines(t)
    return O.qlt_histogram(t["fq"], qoff, np.minimum(qlen, cap), level, first, step)


def is_wave(t):
    """launch_qlt_hist's choice"""
    return len(t["fq"]) // (t["fq"].count(b"\n") // 4) > 4000


def classes(name):
    """class -> the times it occurs (or 1 / 0), by the oracle's counts"""
    t = text(name)
    fq = t["fq"]
    qoff, qlen = lines(t)
    nrec = len(qoff)
    per = WAVE_WG if is_wave(t) else HIST_T
    c = {"mean-over-4000": int(is_wave(t)), "mean-at-most-4000": int(not is_wave(t)), "solid": int(t["solid"])}
    c["workgroups:%d" % -(-nrec // per)] = 1
    c["last-wg-one-record"] = int(nrec % per == 1)
    for L in set(LANE_LENS + WAVE_LENS + tuple(sum(_WAVE_SHAPES.values(), ()))):
        c["len:%d" % L] = int((qlen == L).sum())
    c["escapes"] = int(histogram(t, 1).reshape(-1, 64)[:, 63].sum())
    if name in REPEATED:
        for level in (1, 2, 3, 4):
            crowded, hot = True, 0
            for w in range(-(-nrec // per)):
                r = slice(w * per, min(nrec, (w + 1) * per))
                h = O.qlt_histogram(fq, qoff[r], np.minimum(qlen[r], PRIOR_SYMBOLS), level, 0, 1)
                full = r.stop - r.start == per
                crowded &= (not full) or int(np.count_nonzero(h)) > HIST_S
                hot = max(hot, int(h.max()))
            c["crowded:%d" % level] = int(crowded)
            c["hot:%d" % level] = int(hot >= 768)
    if name.startswith("tail-"):
        starts, _ = util.line_table(fq)
        ok = all((nrec - 1) % (s * k) == 0 for s in STEPS for k in SCALES) and int(starts[-1]) + int(qlen[-1]) + 1 == len(fq)
        c["tail:%d:%d" % (int(starts[-1]) % 4, int(qlen[-1]))] = int(ok)
    if "drops" in name:
        early = late = 0
        for r in range(nrec):
            d3 = lambda cap: (np.flatnonzero(O.qlt_histogram(fq, qoff[r:r + 1], np.minimum(qlen[r:r + 1], cap), 3, 0, 1).reshape(-1, 64).sum(axis=1)) >> 13).max()
            head, whole = d3(64), d3(PRIOR_SYMBOLS)
            early += head == 7
            late += head < 7 and whole == 7
        c["d3-early"], c["d3-late"] = int(early), int(late)
    return c


def claims(name):
    return CLAIMS[name]


# ---- count tables --------------------------------------------------------------------------------------------------------------------------------
ORDINARY_RECORDS = 300                                       # the small ordinary text the tables' rows are coded over


@functools.lru_cache(maxsize=None)
def ordinary():
    rng = np.random.default_rng(77)
    return _assemble("ord", [walk(rng, 30 + (i * 13) % 90) for i in range(ORDINARY_RECORDS)], 64, 6)


def _row(kind):
    """64 counts of the kind, and the shift the rule must apply to them (None: whatever it is)"""
    r = np.zeros(64, np.uint64)
    small = np.array([3, 7, 40, 41, 62])
    if kind.startswith("max:"):                              # a largest count on either side of a scaling border: 6 * max against 32 000
        # (42 667: 6 * max >> 3 is 32 000 itself, the largest frequency the encoder writes -- and not above the border)
        mx = int(kind[4:])
        r[small] = (1, 2, mx // 2, mx // 3, 5)
        r[20] = mx
        sh = 0
        while (mx * 6) >> sh > 32000:
            sh += 1
        return r, sh
    if kind == "all-equal":
        r[:] = 100
        return r, 0
    if kind == "two-largest":
        r[small] = (9, 9, 9, 1, 1); r[[11, 50]] = 4000
        return r, 0
    if kind == "three-largest":
        r[small] = (1, 1, 2, 2, 2); r[[0, 33, 63]] = 20000
        return r, 2
    if kind == "zero-tail":                                  # counts that scale to frequency 0, the highest seen symbol among them
        r[3] = 1 << 20; r[[10, 40]] = 1; r[5] = 1 << 8
        return r, 8
    if kind == "only-0":
        r[0] = 17
        return r, 0
    if kind == "only-63":
        r[63] = 17
        return r, 0
    if kind == "near-2^32":
        r[30] = (1 << 32) - 1; r[small] = (1, 2, 3, 1 << 31, 1 << 20)
        return r, 20
    raise KeyError(kind)


# (the second border lies between 10 666 and 10 667 -- 6 * 10 667 >> 1 is 32 001 --: both sides of it, and 10 668)
KINDS = ["max:5333", "max:5334", "max:10666", "max:10667", "max:10668", "max:42667", "all-equal", "two-largest", "three-largest", "zero-tail", "only-0", "only-63", "near-2^32"]


def table_contexts(level):
    """context 0, the last one, and the borders of k_prior_slots' threads and waves: multiples of 1024 -- and, where a wave of its threads
    covers 256 contexts (4096 rows), of 256 -- and the contexts on either side"""
    n = q_rows(level)
    ms = [256 * k for k in range(1, 16)] if n == 4096 else [1024 * k for k in (1, 2, 3, 4, 5, 8, 16, 31, 32, 33, 60, 63)]
    return [0] + [m + d for m in ms for d in (-1, 0, 1)] + [n - 1]


@functools.lru_cache(maxsize=None)
def table(level):
    """The ordinary text's own counts with rows of every kind written over them at table_contexts: a table as several ranks' sum would be"""
    t = ordinary()
    counts = histogram(t, level).astype(np.uint64).reshape(-1, 64)
    kinds, shifts = {}, {}
    for i, c in enumerate(table_contexts(level)):
        kind = KINDS[i % len(KINDS)]
        counts[c], shifts[c] = _row(kind)
        kinds[c] = kind
    assert counts.max() < 1 << 32
    return dict(level=level, counts=counts.astype(np.uint32).reshape(-1), kinds=kinds, shifts=shifts)


# ---- row families ----------------------------------------------------------------------------------------------------------------------------------
SPIKES = (0, 7, 8, 31, 32, 55, 56, 62, 63)
TRIPLES = ((0, 8, 56), (7, 31, 63), (32, 55, 62), (3, 40, 63))
MEMBERS = ["spike:%d" % p for p in SPIKES] + ["triple:%d:%d:%d" % t for t in TRIPLES] + ["all-32000", "only-0", "48-at-1", "49-at-1", "limit:5", "limit:63"]
UNLISTED_EVERY = 17                                          # one context in 17 is left out of the blob: the uniform row


def member_row(kind):
    """A prior row in the canonical form unpack_prior rebuilds: the non-zero head (frequency descending, symbol ascending), then the unused
    symbols below iend ascending; total, iend"""
    f, iend = {}, 64
    if kind.startswith("spike:"):
        f = {int(kind[6:]): 32000}
    elif kind.startswith("triple:"):
        f = {int(s): 32000 for s in kind.split(":")[1:]}
    elif kind == "all-32000":
        f = {s: 32000 for s in range(64)}
    elif kind == "only-0":
        f, iend = {0: 1}, 1
    elif kind in ("48-at-1", "49-at-1"):
        iend = int(kind[:2]); f = {s: 1 for s in range(iend)}
    elif kind.startswith("limit:"):                          # the largest frequency the parser accepts
        f = {int(kind[6:]): 65535}
    else:
        raise KeyError(kind)
    r = np.zeros(66, np.uint32)
    head = sorted(f, key=lambda s: (-f[s], s))
    for j, s in enumerate(head + [s for s in range(iend) if s not in f]):
        r[j] = f.get(s, 0) | (s << 16)
    r[64], r[65] = sum(f.values()), iend
    return r


def member_of(ctx):
    """the family member context ctx is given (None: unlisted)"""
    return None if ctx % UNLISTED_EVERY == UNLISTED_EVERY - 1 else MEMBERS[ctx % len(MEMBERS)]


@functools.lru_cache(maxsize=None)
def family_text():
    """6000 records of 1 .. 40 qualities drawn uniformly from '"' .. '~' ('!' would also mark its base): every context of level 1, and so
    every family member, meets every symbol"""
    rng = np.random.default_rng(4242)
    t = _assemble("fam", [uniform(rng, 1 + int(rng.integers(0, 40)), 34, 126) for _ in range(6000)], 600, 8)
    return dict(t, cr=8)


@functools.lru_cache(maxsize=None)
def family(level):
    """Level 1: every context a member by ctx % n.  Level 3: the contexts the text visits, alike.  -> dict(fq, br, cr, rows66, prior, rec_prior, frozen)"""
    t = family_text()
    fq = t["fq"]
    n = q_rows(level)
    rows66 = np.zeros((n, 66), np.uint32)
    visited = range(n) if level == 1 else np.flatnonzero(histogram(t, level, cap=1 << 30).reshape(-1, 64).sum(axis=1))
    made = {k: member_row(k) for k in MEMBERS}
    for c in visited:
        k = member_of(int(c))
        if k is not None:
            rows66[c] = made[k]
    starts, ll = util.line_table(fq)
    hoff, hlen = starts[0::4] + 1, ll[0::4] - 1
    f = O.rec_prior_freqs(O.rec_count(fq, hoff, hlen, *rec_sample(len(hoff))))
    return dict(t, level=level, rows66=rows66, prior=pack_prior(rows66), rec_prior=pack_rec_prior(f), frozen=O.qlt_frozen_rows(rows66))


def family_uses(level):
    """[member, symbol]: the times the text codes the symbol under a row of the member (the last row of the result: unlisted contexts)"""
    h = histogram(family_text(), level, cap=1 << 30).reshape(-1, 64)
    out = np.zeros((len(MEMBERS) + 1, 64), np.int64)
    for c in np.flatnonzero(h.sum(axis=1)):
        k = member_of(int(c))
        out[MEMBERS.index(k) if k is not None else len(MEMBERS)] += h[c]
    return out


def legal(t):
    """Legal FASTQ for the block format: four lines a record, '@' and '+', base and quality lines of one length and not empty, qualities
    '!' .. '~'; colour space: a primer base, digits, and a quality line that starts with '!'"""
    fq = t["fq"]
    if not t["solid"]:
        return is_legal(fq)
    ls = fq.split(b"\n")
    if ls[-1] != b"" or len(ls) % 4 != 1:
        return False
    for i in range(0, len(ls) - 1, 4):
        h, b, p, q = ls[i:i + 4]
        if not h.startswith(b"@") or p != b"+" or len(b) != len(q) or len(b) < 2 or b[:1] != b"T" or q[:1] != b"!":
            return False
        if set(b[1:]) - set(b"0123") or not (33 <= min(q) and max(q) <= 126):
            return False
    return True

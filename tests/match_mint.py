"""Texts that take the match model's walk (gm.hip gm_predict / gm_update; the rule: sfq_oracle.c gm_walk) through every transition AT CHOSEN
PLACES: built, not drawn.  A text is gen 0 = `br` source reads, gen 1 = the same reads again (so that the verdict says "on"), and from block 2
on records made of pieces of the sources: a copy that starts where a k-mer of the sampled quarter ends is FOUND behind its sixteenth base and
predicts from its eighteenth on, so a substitution at a chosen base of the copy is a miss at a chosen m and a chosen offset of the pointer's window,
and a source that ends a chosen number of bases behind the k-mer is a sentinel at a chosen distance.  What a text claims (CLAIMS: class -> texts) is
counted from the oracle's own trace of the walk (O.gm_trace) by classes(); test_match_inputs.py holds every text to its claims on the CPU,
test_match_walk.py runs them on the GPU.

The classes, in the trace's terms (base i of a line or segment of n bases; a pointer found at p predicts from p + GM_D on, dist = pointer - p):
  run:L            a pointer's first L bases hit, then a substitution or the earlier line's end (L = 1 .. 33: across the window's shift at dist 16,
                   the prefetch at dist 8, GM_MCAP, and -- behind a kept miss -- the level borders 4 / 8 / 16)
  drop:m=K keep:m=K  a miss at m = K drops the pointer (K < 8) / keeps it, m back to 0 (K >= 8).  m < 16 means a miss K + 1 bases before: drop:m=3 is
                   two misses four bases apart, drop:m=7 eight apart, keep:m=8 nine apart
  reacquire        a pointer that had asked for its second window (dist >= 8) is dropped by a miss, and a later pointer of the same line walks into
                   ITS second window (dist >= 17)
  drop-at-prefetch a miss drops the pointer at dist = 8, on the base whose step asks for the second window (end-run:7 is the sentinel there)
  refused          the earlier line's sentinel at p + 1: the pending pointer is refused.  (A sentinel AT p does not occur: the index takes no k-mer
                   behind the line's last base, gm_insert's i + 1 < len.)
  end-run:L        the pointer runs into the earlier line's sentinel after L bases (end-run:1: the sentinel at p + 2)
  held-to-last-base  a duplicate of an earlier read: the pointer predicts the line's last base, the earlier line's sentinel behind it
  len:L            base lines of L bases (1, 15 .. 20; the block format refuses a record with an empty base line)
  lookup-last-eligible / none-one-later   an entry is read behind base n - 3 (i + 1 + GM_D == n - 1); behind base n - 2 none is, though the k-mer
                   is of the sampled quarter and no pointer stands or is pending
  insert:lane-per-record / insert:stretch-first / insert:stretch-last   a pointer found through an entry that launch_gm_insert wrote a lane per record
                   (no base line of 64) / whose k-mer ends on the first / the last base of a stretch of 32 (lines of 64 .. 150)
  lim / next-gen-taken / check   the entry's position is not below the generation's first (the k-mer's earliest occurrence is in the chain's own
                   generation); the same k-mer taken from the next generation; the slot holds another k-mer (table of 2^16)
  last-record-pointer  the last generation is ONE record that copies the tail of the record before it (see stage_end)
  lane-alone:K     a wavefront of 64 chains of which chain K alone ever has a pointer
  all-lanes        a wavefront whose 64 chains all have pointers, their first bases at all sixteen offsets i mod 16
  unequal          a wavefront whose chains all have pointers and are of 32 or more different lengths
  N-source / N-target / lc-source / lc-target : hit / miss   an N-like or lower-case letter under the pointer or predicted by it
  found-near-segment-end / cold-start / own-record-refused   chains that are segments: found in a segment's last eight bases; a segment that starts
                   without the pointer the segment before it ended with; an entry that points into an earlier segment of the record itself (lim)
"""
import functools

import numpy as np

import util
from oracle import oracle as O
from clamp_mint import generation_bounds
from test_frozen_tables import gm_chain_reads, gm_table_bits

GM_K, GM_D, GM_DROP = 16, 1, 8
MIN = 16                                                    # times a text's class must occur
RUNS = (1, 6, 7, 8, 9, 14, 15, 16, 17, 31, 32, 33)
DROPS, KEEPS = (0, 3, 4, 7), (8, 15, 16, 31)
END_RUNS = tuple(range(1, 21))
LENS = (1, 15, 16, 17, 18, 19, 20)
STAGE_END = tuple(range(19, 41))
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_HASH = np.uint64(0x9E3779B97F4A7C15)


# ---- the index's sampling, restated ------------------------------------------------------------------------------------------------------------
def sampled(codes):
    """[e]: the k-mer of sixteen bases that ends at base e is of the quarter the index holds (top two bits of kmer * HASH are zero)"""
    c = np.asarray(codes, np.uint64) & np.uint64(3)
    k = np.zeros(len(c), np.uint64)
    for j in range(min(GM_K, len(c))):
        k[j:] |= c[:len(c) - j] << np.uint64(2 * j)
    with np.errstate(over="ignore"):
        h = k * _HASH
    s = (h >> np.uint64(62)) == 0
    s[:GM_K - 1] = False
    return s


def slots(codes, tb=16):
    """the index's entries that the line's sampled k-mers go to (a table of 2^tb)"""
    c = np.asarray(codes, np.uint64) & np.uint64(3)
    k = np.zeros(len(c), np.uint64)
    for j in range(min(GM_K, len(c))):
        k[j:] |= c[:len(c) - j] << np.uint64(2 * j)
    with np.errstate(over="ignore"):
        h = k * _HASH
    return ((h >> np.uint64(62 - tb)) & np.uint64((1 << tb) - 1))[sampled(codes)]


def fresh(rng, n):
    return rng.integers(0, 4, n, dtype=np.uint8)


def source(rng, n, ends=(), not_ends=()):
    """n random bases whose k-mers ending at `ends` are sampled and those ending at `not_ends` are not"""
    while True:
        c = fresh(rng, n)
        s = sampled(c)
        if all(s[e] for e in ends) and not any(s[e] for e in not_ends):
            return c


def first_sampled(src, amin):
    """the first a >= amin at which a copy of src[a:] is found behind its sixteenth base"""
    s = sampled(src)
    return int(np.flatnonzero(s[amin + GM_K - 1:])[0]) + amin


def copy_of(rng, src, a, k, f=0, subs=(), tail=0):
    """f fresh bases, src[a : a + k] with the copy's bases `subs` replaced by other ones, `tail` fresh bases -- that do not go on as src does --:
    base j of the copy (j >= 17) is base f + j of the line and the pointer's base number j - 16"""
    c = src[a:a + k].copy()
    assert len(c) == k and all(GM_K < s < k for s in subs)
    for s in subs:
        c[s] = (c[s] + rng.integers(1, 4)) & 3
    t = fresh(rng, tail)
    if tail and a + k < len(src):
        t[0] = (src[a + k] + rng.integers(1, 4)) & 3
    h = fresh(rng, f)
    if f and a:
        h[-1] = (src[a - 1] + rng.integers(1, 4)) & 3        # (nor come from it: the first k-mer the copy shares with src ends at its sixteenth base)
    return np.concatenate([h, c, t]).astype(np.uint8)


# ---- a text ------------------------------------------------------------------------------------------------------------------------------------
def assemble(name, lines, br, cr, seed, seg=0, solid=False):
    """lines: the base lines' letters (bytes), gen 0 and gen 1 included -> dict(fq, br, cr, seg, solid, name)"""
    rng = np.random.default_rng(seed)
    q = np.frombuffer(b"5:?I", np.uint8)
    recs = []
    for i, ln in enumerate(lines):
        ql = q[rng.integers(0, 4, len(ln))].tobytes()
        if solid:
            ln, ql = b"T" + ln, b"!" + ql
        recs.append(b"@%s.%d\n%s\n+\n%s\n" % (name.encode(), i, ln, ql))
    nblocks = -(-len(lines) // br)
    assert 3 <= nblocks <= 64 and len(lines) <= 20000 and (seg or max(len(ln) for ln in lines) <= 150 + solid)
    return dict(name=name, fq=b"".join(recs), br=br, cr=cr, seg=seg, solid=solid)


def letters(lines):
    return [_ACGT[c].tobytes() for c in lines]


def two_generations(rng, br, n, special=()):
    """gen 0: the special sources, then random ones of n bases, br in all"""
    src = list(special) + [fresh(rng, n) for _ in range(br - len(special))]
    assert len(src) == br
    return src


def _runs_lines(rng, br=64):
    src = two_generations(rng, br, 150)
    later = []
    for L in RUNS:                                           # L hits, a substitution (a kept miss: m >= 16), twelve more hits, fresh bases
        for k in range(20):
            s = src[(k * 7 + L) % br]
            a = first_sampled(s, k % 11)
            later.append(copy_of(rng, s, a, 17 + L + 1 + 12, f=(5 * k + L) % 16, subs=(17 + L,), tail=3 + k % 4))
    return src + src + later


def _drops_lines(rng, br=64):
    src = two_generations(rng, br, 150)
    later = []
    for K in DROPS + KEEPS[:2]:                              # ten hits, a miss (kept), K hits, a miss at m = K, fifty bases of the copy
        for k in range(20):
            s = src[(k * 5 + K) % br]
            a = first_sampled(s, k % 13)
            later.append(copy_of(rng, s, a, 17 + 10 + 1 + K + 1 + 50, f=(3 * k + K) % 16, subs=(27, 28 + K), tail=2 + k % 3))
    for h in (0, 20):                                        # the first miss itself: at m = 16 (the first predicted base), at m = 31
        for k in range(20):
            s = src[(k * 3 + h) % br]
            a = first_sampled(s, k % 13)
            later.append(copy_of(rng, s, a, 17 + h + 1 + 40, f=(7 * k) % 16, subs=(17 + h,), tail=2))
    for k in range(20):                                      # misses at the pointer's fourth and eighth base: dropped by the step that asks for the second window
        s = src[(k * 13 + 1) % br]
        a = first_sampled(s, k % 13)
        later.append(copy_of(rng, s, a, 17 + 8 + 40, f=(k * 9) % 16, subs=(20, 24), tail=2))
    for k in range(20):                                      # sixteen hits behind a kept miss: a miss at m = 16 that m has COUNTED up to
        s = src[(k * 11) % br]
        a = first_sampled(s, k % 13)
        later.append(copy_of(rng, s, a, 17 + 3 + 1 + 16 + 1 + 20, f=k % 16, subs=(20, 37), tail=2))
    return src + src + later


def _ends_lines(rng, br=64):
    n = 100
    special = [source(rng, n, ends=(n - 2 - L,)) for L in range(21)]          # the pointer found behind base n - 2 - L predicts L bases of it
    src = two_generations(rng, br, n, special)
    later = []
    for L in range(21):
        for k in range(18):
            later.append(copy_of(rng, src[L], n - 17 - L, 17 + L, f=(k + L) % 16, tail=4 + k % 3))
    return src + src + later


def _short_lines(rng, br=64):
    src = two_generations(rng, br, 63)
    smp = [sampled(s) for s in src]
    later = []
    for n in LENS:                                           # (no line of 0 bases: the oracle takes one, the block format refuses the record, SFQ_E_UNSUPPORTED)
        if n < 18:
            later += [fresh(rng, n) for _ in range(20)]
            continue
        # src[a : a + n]: no k-mer sampled before the one ending at base n - 3, that one and the next one sampled
        spots = [(j, a) for j in range(br) for a in range(63 - n + 1)
                 if not smp[j][a + 15:a + n - 3].any() and smp[j][a + n - 3] and smp[j][a + n - 2]]
        assert len(spots) >= 4, (n, len(spots))
        later += [src[j][a:a + n].copy() for j, a in (spots[k % len(spots)] for k in range(20))]
    for k in range(24):                                      # new bases: an entry read behind base n - 3 and not taken, none read behind base n - 2
        later.append(source(rng, 18 + k % 3, ends=(15 + k % 3, 16 + k % 3)))
    for k in range(40):                                      # and ordinary copies, for the entries themselves
        s = src[k % br]
        a = first_sampled(s, k % 7)
        k_ = min(40, 63 - a)
        later.append(copy_of(rng, s, a, k_, subs=(25,) if k_ > 26 else (), tail=2))
    return src + src + later


def _long_lines(rng, br=64):
    borders = (31, 32, 63, 64, 95, 96, 127, 128)             # k-mers that end on a stretch's last base, and on the next one's first
    special = [source(rng, 150, ends=(e, e + 1) if e % 32 == 31 else (e - 1, e)) for e in borders for _ in range(2)]
    src = two_generations(rng, br, 150, special)
    later = []
    for j, e in enumerate(np.repeat(borders, 2)):
        for k in range(10):                                  # found through the entry of the k-mer that ends at base e of the source
            later.append(copy_of(rng, src[j], int(e) - 15, min(40, 150 - (int(e) - 15)), f=48 + (k + j) % 16, subs=(30,) if e < 120 else (), tail=5))
    pairs = [(j, a) for j in range(br) for a in np.flatnonzero(sampled(src[j])[15:-3] & sampled(src[j])[16:-2])]
    for k in range(24):                                      # a line of f + 18 bases: the lookup behind base n - 3, none behind base n - 2
        j, a = pairs[k % len(pairs)]
        later.append(copy_of(rng, src[j], int(a), 18, f=64 + 3 * k if k < 22 else 46 + k))
    for k in range(24):                                      # the same without a pointer: the entry behind base n - 3 is not taken
        later.append(source(rng, 64 + 3 * k, ends=(61 + 3 * k, 62 + 3 * k)))
    for k in range(30):                                      # lines of 64 .. 150 all through
        later.append(fresh(rng, 64 + (k * 43) % 87))
    return src + src + later


def _generations_lines(rng, br=64):
    src = two_generations(rng, br, 100)
    x = [fresh(rng, 100) for _ in range(br)]                 # block 2: new reads; block 3 (the same generation) and block 4 (the next) repeat them
    later = x + [c.copy() for c in x] + [copy_of(rng, c, 0, 100, subs=(60,)) for c in x]
    later += [fresh(rng, 100) for _ in range(3 * br)]        # blocks 5 .. 7: reads the index takes and nobody repeats: full slots
    for k in range(2 * br):                                  # the last generation: new reads that meet them, and copies
        later.append(fresh(rng, 100) if k % 2 else copy_of(rng, x[k % br], first_sampled(x[k % br], k % 9), 60, f=k % 16, subs=(40,), tail=3))
    return src + src + later


def stage_end_lines(rng, n, br=64):
    """Three blocks; the last generation is ONE record of n bases, the last n of the record before it: its pointer walks the stage's last full
    line, its windows lie as close to the stage's end as a walk's can.  (gm_ld16 holds an address at `cap` only from cap on, and no walk loads
    there: a pointer lies below its chain's generation, a window starts at most 24 bytes behind it, and a record that has a pointer is 18
    bases or more, so its generation alone is 19 bytes.  The hold is for k_gm_code's token window behind the last piece.)"""
    src = two_generations(rng, br, 100)
    taken = set(np.concatenate([slots(c) for c in src]).tolist())
    while True:                                              # (an entry of its own for every k-mer of the record before the last: the earliest stays)
        last = source(rng, 100, ends=(100 - n + 15,))
        if not taken & set(slots(last).tolist()):
            break
    return src + src[:br - 1] + [last, last[100 - n:].copy()]


def _lane_lines(rng, lane, nblocks=20, br=64):
    src = two_generations(rng, br, 120)
    later = []
    for b in range(2, nblocks):
        for j in range(br):
            if j != lane:
                later.append(fresh(rng, 100))
                continue
            s = src[(b * 5) % br]                            # nine hits, a miss (kept), three hits, a miss (dropped), found again
            later.append(copy_of(rng, s, first_sampled(s, b % 9), 17 + 9 + 1 + 3 + 1 + 50, f=b % 16, subs=(26, 30), tail=2))
    return src + src + later


def _all_lanes_lines(rng, nblocks=20, br=64):
    src = two_generations(rng, br, 120)
    later = []
    for b in range(2, nblocks):
        for j in range(br):
            s = src[(j + 3 * b) % br]
            subs = ((), (27,), (22, 30), (37,))[(j + b) % 4]
            later.append(copy_of(rng, s, first_sampled(s, (j * 7 + b) % 10), 17 + 60, f=(j + b) % 16, subs=subs, tail=1 + j % 5))
    return src + src + later


def _unequal_lines(rng, nblocks=20, br=64):
    src = two_generations(rng, br, 150, [source(rng, 150, ends=(15,)) for _ in range(br)])
    later = []
    for b in range(2, nblocks):
        for j in range(br):                                  # chain j: 20 + 2 j bases; the short chains' lanes have ended while the long ones walk
            n = 20 + 2 * j
            later.append(copy_of(rng, src[(j + b) % br], 0, n, subs=tuple(s for s in (19 + (b % 3), 40 + b, 90 + b) if s < n)))
    return src + src + later


def _decorate(rng, lines, solid):
    """The lines' letters: a third of the A's written N ('.'), and -- base space -- a fifth of the letters in lower case.  The staged codes stay."""
    out = []
    for c in lines:
        ln = (np.frombuffer(b"0123", np.uint8) if solid else _ACGT)[c].copy()
        ln[(c == 0) & (rng.random(len(c)) < 1 / 3)] = ord(".") if solid else ord("N")
        if not solid:
            lc = rng.random(len(c)) < 0.2
            ln[lc] |= 0x20
        out.append(ln.tobytes())
    return out


def _segments_lines(rng, br=4, nblocks=12, n=3000, L=600):
    src = [fresh(rng, n) for _ in range(br)]
    later = []
    for r in range((nblocks - 2) * br):
        c = fresh(rng, n)
        s = src[r % br]
        for sg in range(4):                                  # found seven bases before the segment's end; the copy goes on into the next one
            x = first_sampled(s, 200 * sg + r % 50)
            at = L * (sg + 1) - 22
            c[at:at + 22 + 60] = s[x:x + 22 + 60]
        c[4 * L + 100:4 * L + 160] = c[L + 200:L + 260]        # the last segment repeats bases of the record's second one
        later.append(c)
    return src + src + later


def _build(name):
    rng = np.random.default_rng(sum(name.encode()) * 1009 + len(name))
    if name == "runs":
        return assemble(name, letters(_runs_lines(rng)), 64, 4, 1)
    if name == "drops":
        return assemble(name, letters(_drops_lines(rng)), 64, 4, 2)
    if name == "ends":
        return assemble(name, letters(_ends_lines(rng)), 64, 4, 3)
    if name == "short":
        return assemble(name, letters(_short_lines(rng)), 64, 8, 4)
    if name == "long":
        return assemble(name, letters(_long_lines(rng)), 64, 4, 5)
    if name == "generations":
        return assemble(name, letters(_generations_lines(rng)), 64, 4, 6)
    if name.startswith("stage-end-"):
        return assemble(name, letters(stage_end_lines(rng, int(name[10:]))), 64, 4, 7)
    if name.startswith("lane"):
        return assemble(name, letters(_lane_lines(rng, int(name[4:]))), 64, 1, 8)
    if name == "all-lanes":
        return assemble(name, letters(_all_lanes_lines(rng)), 64, 1, 9)
    if name == "unequal":
        return assemble(name, letters(_unequal_lines(rng)), 64, 1, 10)
    if name == "alphabet":
        return assemble(name, _decorate(rng, _drops_lines(rng), False), 64, 4, 11)
    if name == "colour":
        return assemble(name, _decorate(rng, _drops_lines(rng), True), 64, 4, 12, solid=True)
    if name == "segments":
        return assemble(name, letters(_segments_lines(rng)), 4, 1, 13, seg=700)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def text(name):
    return _build(name)


# ---- what a text claims --------------------------------------------------------------------------------------------------------------------------
_HM = ("hit", "miss")
CLAIMS = {
    "runs": ["run:%d" % L for L in RUNS],
    "drops": ["drop:m=%d" % K for K in DROPS] + ["keep:m=%d" % K for K in KEEPS] + ["reacquire", "drop-at-prefetch"],
    "ends": ["refused", "held-to-last-base"] + ["end-run:%d" % L for L in END_RUNS],
    "short": ["len:%d" % L for L in LENS] + ["lookup-last-eligible", "none-one-later", "insert:lane-per-record"],
    "long": ["lookup-last-eligible", "none-one-later", "insert:stretch-first", "insert:stretch-last"],
    "generations": ["lim", "next-gen-taken", "check"],
    "lane0": ["lane-alone:0"], "lane31": ["lane-alone:31"], "lane63": ["lane-alone:63"],
    "all-lanes": ["all-lanes"],
    "unequal": ["unequal"],
    "alphabet": ["%s-%s:%s" % (a, w, h) for a in ("N", "lc") for w in ("source", "target") for h in _HM],
    "colour": ["N-%s:%s" % (w, h) for w in ("source", "target") for h in _HM],
    "segments": ["found-near-segment-end", "cold-start", "own-record-refused"],
}
# one record is the whole last generation: the class occurs once a text, in each of the 22
CLAIMS.update({"stage-end-%d" % n: ["last-record-pointer"] for n in STAGE_END})
TEXTS = sorted(CLAIMS)
PLACED = [n for n in TEXTS if n.startswith(("stage-end-", "lane")) or n in ("all-lanes", "unequal")]     # also through the device entries
MIN_OF = {"last-record-pointer": 1}


def geometry(t):
    """(goff, glen, other, nrec, tb, gcr): the base lines, and the index's bits and the base chains' records as api.cpp chooses them"""
    fq = t["fq"]
    starts, lens = util.line_table(fq)
    s = int(t["solid"])
    goff, glen, other = starts[1::4] + s, lens[1::4] - s, lens[3::4]
    nrec = len(goff)
    return goff, glen, other, nrec, gm_table_bits(len(fq)), (1 if t["seg"] else gm_chain_reads(len(fq), nrec, t["br"], t["cr"]))


@functools.lru_cache(maxsize=None)
def walk(name):
    """The oracle's trace of the text's walk and what classes() needs beside it, over the stage's positions"""
    t = text(name)
    fq, br, seg = t["fq"], t["br"], t["seg"]
    goff, glen, other, nrec, tb, gcr = geometry(t)
    tr = O.gm_trace(fq, goff, glen, tb, br, gcr, seg, other)
    soff = tr["soff"]
    npos = int(soff[-1])
    a = np.frombuffer(fq, np.uint8)
    rec = np.repeat(np.arange(nrec), glen.astype(np.int64) + 1)
    i = np.arange(npos) - soff[rec]
    n = glen.astype(np.int64)[rec]
    sent = i == n
    letter = np.full(npos, 10, np.uint8)
    letter[~sent] = a[(goff.astype(np.int64)[rec] + i)[~sent]]
    code = np.zeros(256, np.uint8)
    for chars, v in (("0Aa", 0), ("1Cc", 1), ("2Gg", 2), ("3Tt", 3)):
        for ch in chars:
            code[ord(ch)] = v
    b = code[letter]; b[sent] = 255
    if seg:                                                  # a walk's line is the segment (oracle seg_geometry)
        m = np.maximum(glen, other).astype(np.int64)
        k = np.maximum(1, -(-m // seg)); L = np.maximum(1, -(-m // k))
        si, sn = i % L[rec], np.minimum(L[rec], n - (i // L[rec]) * L[rec])
        si[sent], sn[sent] = 0, 0
    else:
        si, sn = i, n
    w = dict(tr, name=name, tb=tb, gcr=gcr, br=br, seg=seg, nrec=nrec, glen=glen, rec=rec, i=i, n=n, si=si, sn=sn, sent=sent, letter=letter, b=b,
             bound=generation_bounds(-(-nrec // br)))
    w["have"] = tr["tok"] != 0
    w["hit"] = w["have"] & ((tr["tok"] & 3) == b)
    w["miss"] = w["have"] & ~w["hit"]
    w["start"] = w["have"] & (tr["dist"] == GM_D)
    return w


def _runs(w):
    """(length, cause) of every pointer's first run of hits: cause 1 a substitution, 2 the earlier line's sentinel, 0 its own line's end"""
    s = np.flatnonzero(w["start"])
    stop = np.flatnonzero(~w["hit"])
    t = stop[np.searchsorted(stop, s)]
    cause = np.where(w["miss"][t], 1, np.where(w["ev"][t] & O.GMT_DROP_END, 2, 0))
    return t - s, cause


def classes(name):
    """class -> the times it occurs in the text, by the oracle's trace"""
    w = walk(name)
    ev, m, dist, ptr, have, hit, miss, si, sn, rec, soff, b = (w[k] for k in ("ev", "m", "dist", "ptr", "have", "hit", "miss", "si", "sn", "rec", "soff", "b"))
    br, nrec, glen = w["br"], w["nrec"], w["glen"]
    c = {}
    run, cause = _runs(w)
    for L in RUNS:
        c["run:%d" % L] = int(((run == L) & (cause != 0)).sum())
    for L in END_RUNS:
        c["end-run:%d" % L] = int(((run == L) & (cause == 2)).sum())
    dropped = (ev & O.GMT_DROP_MISS) != 0
    assert not (dropped & ~miss).any()
    for K in DROPS + KEEPS:
        c["drop:m=%d" % K] = int((dropped & (m == K)).sum())
        c["keep:m=%d" % K] = int((miss & ~dropped & (m == K)).sum())
    again = 0
    for d in np.flatnonzero(dropped & (dist >= 8)):
        again += bool((dist[d + 1:d + 1 + int(sn[d] - si[d] - 1)] >= 17).any())
    c["reacquire"] = again
    c["drop-at-prefetch"] = int((dropped & (dist == 8)).sum())
    c["refused"] = int(((ev & O.GMT_REFUSED) != 0).sum())
    last = have & (si == sn - 1) & (w["seg"] == 0)
    c["held-to-last-base"] = int((b[ptr[last].astype(np.int64) + 1] == 255).sum())
    for L in LENS:
        c["len:%d" % L] = int((glen[br:] == L).sum())
    lookup, found = (ev & O.GMT_LOOKUP) != 0, (ev & O.GMT_FOUND) != 0
    c["lookup-last-eligible"] = int((lookup & (si == sn - 3)).sum())
    q = np.flatnonzero((si == sn - 2) & (sn >= GM_K + 2) & (rec >= br))
    smp = sampled(np.where(w["sent"], 0, b))
    c["none-one-later"] = int((smp[q] & ~lookup[q] & ~have[q + 1] & ((ev[q + 1] & (O.GMT_REFUSED | O.GMT_DROP_END)) == 0) & ~found[q - 1]).sum())
    p = ptr[found].astype(np.int64)
    prec = np.searchsorted(soff, p, side="right") - 1
    kend = p - 1 - soff[prec]                                # the base of its line that the k-mer ends at
    longest = int(glen.max())
    c["insert:lane-per-record"] = int(found.sum()) if longest < 64 else 0
    c["insert:stretch-first"] = int((kend % 32 == 0).sum()) if 64 <= longest and int(glen.min()) >= 64 else 0
    c["insert:stretch-last"] = int((kend % 32 == 31).sum()) if 64 <= longest and int(glen.min()) >= 64 else 0
    c["lim"] = int(((ev & O.GMT_LIM) != 0).sum())
    c["check"] = int(((ev & O.GMT_CHECK) != 0).sum()) if w["tb"] == 16 else 0
    c["next-gen-taken"] = int((p >= soff[min(nrec, w["bound"][2] * br)]).sum())
    c["last-record-pointer"] = int(have[soff[nrec - 1]:].any()) if nrec == 2 * br + 1 else 0
    # wavefronts of the later generations: block = 64 records = 64 chains = the lanes of one wavefront of k_gm_plan, k_gm_code and k_gm_decode_c
    if br == 64 and w["gcr"] == 1 and not w["seg"]:
        any_have = np.bincount(rec[have], minlength=nrec) > 0
        first_i = np.full(nrec, -1); first_i[rec[w["start"]][::-1]] = si[w["start"]][::-1]
        for k in (0, 31, 63):
            c["lane-alone:%d" % k] = 0
        c["all-lanes"] = c["unequal"] = 0
        for blk in range(2, nrec // br):
            lanes = any_have[blk * br:(blk + 1) * br]
            if lanes.sum() == 1 and int(np.flatnonzero(lanes)[0]) in (0, 31, 63):
                c["lane-alone:%d" % int(np.flatnonzero(lanes)[0])] += 1
            if lanes.all():
                c["all-lanes"] += len(set(first_i[blk * br:(blk + 1) * br] % 16)) == 16
                c["unequal"] += len(set(glen[blk * br:(blk + 1) * br].tolist())) >= 32
    # letters
    nlike, lower = np.zeros(256, bool), np.zeros(256, bool)
    nlike[list(b"Nn.")] = True; lower[list(b"acgtn")] = True
    at = np.flatnonzero(have)
    src, tgt = w["letter"][ptr[at].astype(np.int64)], w["letter"][at]
    for tag, tab in (("N", nlike), ("lc", lower)):
        for where, l in (("source", src), ("target", tgt)):
            c["%s-%s:hit" % (tag, where)] = int((tab[l] & hit[at]).sum())
            c["%s-%s:miss" % (tag, where)] = int((tab[l] & miss[at]).sum())
    # segments
    if w["seg"]:
        c["found-near-segment-end"] = int((found & (si >= sn - 8)).sum())
        first = np.flatnonzero((si == 0) & (w["i"] > 0) & ~w["sent"])
        c["cold-start"] = int((have[first - 1] & ~have[first]).sum())
        lim = np.flatnonzero((ev & O.GMT_LIM) != 0)
        pl = ptr[lim].astype(np.int64)
        c["own-record-refused"] = int(((pl >= soff[rec[lim]]) & (pl < lim - si[lim])).sum())      # in an EARLIER segment of the record
    return c


def coverage(name):
    """What the text adds to the sum over all texts: event bits, (hit, level), (miss, level), pointer offsets"""
    w = walk(name)
    have, lv = w["have"], (w["tok"] >> 2) & 3
    out = {"ev:%d" % k for k in range(8) if ((w["ev"] >> k) & 1).any()}
    out |= {"hit:%d" % l for l in np.unique(lv[w["hit"]])} | {"miss:%d" % l for l in np.unique(lv[w["miss"]])}
    out |= {"offset:%d" % o for o in np.unique(w["dist"][have] % 16)}
    return out


COVERAGE = {"ev:%d" % k for k in range(8)} | {"%s:%d" % (h, l) for h in _HM for l in range(4)} | {"offset:%d" % o for o in range(16)}

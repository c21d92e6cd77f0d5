"""Small texts built for the GEOMETRY of chains that are segments of one record (dev_walk.h seg_count_of / seg_range /
LineWalk::bounds and their restatements in gm.hip and chains.hip): a record of M = max(bases, qualities) symbols is n = ceil(M / seg_len)
chains of L = ceil(M / n) symbols, chain s covers symbols [s L, s L + L) of the base line in one stream and of the quality line in the
other -- as far as each line goes, so the shorter line's late chains are EMPTY.  The rule is stated once more here, in plain Python (cut,
piece), and every class a text claims is counted by classes() from (glen, qlen, seg) and the text's letters alone: no oracle call.
test_segment_inputs.py holds every text to its claims on the CPU, test_segment_edges.py runs them on the GPU.

Texts (TEXTS): a variant and a segment length.  A segment under the match model finds its first pointer behind sixteen bases, so that variant
takes segments of 64 and 75 only; flat bases take 16, 17, 64 and 75; colour space 17 (flat) and 64 (match model).
  match-S      base lines are pieces of one small pool, repeated: the match model's verdict is "on"
  flat-S       iid bases: verdict "off", the bases two bits each (chn.idx flag bit 7)
  colour-S     digits behind a primer base, '!' in front of the qualities: M counts the lines without that character
  capacity     near-capacity qualities: see capacity_text()

Line-length classes, s = seg_len; ":g" the longer line is the bases, ":q" the qualities (lines of equal length count for both):
  M=1 M=s-1 M=s M=s+1 M=2s-1 M=2s M=2s+1 M=ks (k >= 5)      nL=M (n >= 2)      last-seg-1 (the last segment holds one symbol)
  equal differ-1      short=jL short=jL-1 short=jL+1 (0 < j < n)      short<L      short=1 (n >= 2)
  empty>=70 empty>=260 (the shorter line leaves that many chains in a row empty)      segs>=300
  aligned-256-empty (chains 256 j .. 256 j + 255 of the call all empty in the shorter line's stream: records of two symbols in front of a
  record of 300 segments put its second chain on a multiple of 256; the texts of 16 and 17 have records of 600 segments)
and without a direction: straddle-256 (ONE record can lie across chain 256 of a call: asked for once), straddle-64j.
Record and block classes, "@b" for block_reads = b in BRS where a block's size matters:
  one-seg-between      one-seg-first@b one-seg-last@b      all-one-seg-block@b      short-last-block@b (once)      last:long / last:short (once)
Exception classes, kind@place:  kinds N (quality not '!'), bang ('!' over a real base), Nbang, lc, lcrun (a lower-case run across a segment
border; place "border"); places first / last (a segment's first symbol, segment 1 or later; a whole segment's last symbol), tail (in the record's
last, short segment), only-tail (the same, the record's ONLY exception); and bang-behind-bases, N-behind-qualities, N-alone-by-300 (a record of
one base, an N, next to one of 300 bases).  Colour space has no lower case.
"""
import functools

import numpy as np

import util
from oracle import oracle as O
from test_frozen_tables import gm_table_bits

SEGS = (16, 17, 64, 75)
BRS = (4, 7, 64)
LEVELS = (1, 3)
MIN = 2                                                      # times a text's class must occur
PRIOR_SYMBOLS = 4096
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_QS = np.frombuffer(b"+5:?DIN", np.uint8)


# ---- the rule, restated ------------------------------------------------------------------------------------------------------------------------
def cut(glen, qlen, seg):
    """(M, n, L) of a record"""
    M = max(glen, qlen)
    n = max(1, -(-M // seg))
    return M, n, max(1, -(-M // n))


def piece(length, s, L):
    """the symbols [lo, hi) of a line of `length` that segment s holds"""
    lo = min(s * L, length)
    return lo, min(lo + L, length)


# ---- the records' shapes -----------------------------------------------------------------------------------------------------------------------
def _shapes(s):
    """(long, short) line lengths: every line-length class but the big ones"""
    out = []
    for M in (1, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1, 5 * s, 3 * s - 3):
        out.append((M, M))
        if M > 1:
            out.append((M, M - 1))
    for M in (5 * s, 3 * s - 3):
        _, n, L = cut(M, M, s)
        for j in (1, n - 1):
            out += [(M, j * L), (M, j * L - 1), (M, j * L + 1)]
        out += [(M, L // 2), (M, 1)]
    out.append((s * (s - 1) + 1, s - 2))                     # n = s, L = s: the last segment holds one symbol
    return out


def _exc_len(s):
    """M of the records that carry the placed exceptions: four segments or more, the last one short but of three symbols or more"""
    M = 3 * s + 5
    while True:
        _, n, L = cut(M, M, s)
        if 3 <= M - (n - 1) * L < L - 1:
            return M
        M += 1


KINDS = ("N", "bang", "Nbang", "lc")
PLACES = ("first", "last", "tail", "only-tail")


def _plan(s, variant, big):
    """The records of a text, as dicts(g, q, exc): line lengths and the exceptions to place"""
    solid = variant == "colour"
    both = lambda a, b: [dict(g=a, q=b)] + ([dict(g=b, q=a)] if a != b else [])
    body = []
    E = _exc_len(s)
    kinds = [k for k in KINDS if not (solid and k == "lc")]
    for rep in range(MIN):
        shapes = _shapes(s)
        if rep:
            shapes = shapes[::-1]
        for i, (a, b) in enumerate(shapes):
            body += both(a, b)
            if i % 3 == rep:
                body.append(dict(g=1 + (i * 5) % s, q=1 + (i * 7) % s))          # a one-segment record between many-segment ones
        for k in kinds:
            for p in PLACES:
                body.append(dict(g=E, q=E, exc=(k, p)))
        if not solid:
            body.append(dict(g=E, q=E, exc=("lcrun", "border")))
        body += [dict(g=E - s - 2, q=E, exc=("bang-behind-bases", "")), dict(g=E, q=E - s - 2, exc=("N-behind-qualities", ""))]
        # (colour space: a block is taken for colour space by its FIRST record's line, usrs.cpp:239-257 -- "T." alone does not say so)
        while solid and any((16 + len(body) + (128 if len(body) >= 112 else 0)) % b == 0 for b in BRS):
            body.append(dict(g=s + 2, q=s + 2))
        body += [dict(g=1, q=1, exc=("N-alone", "")), dict(g=300, q=300)]
    cover = [dict(g=5 * s + 3, q=5 * s + 3, cover=True) for _ in range(16)]
    a, b = body[:112], body[112:]
    while len(a) < 112:
        a.append(dict(g=2 * s + 3 + len(a) % 5, q=2 * s + 3))
    ones = [dict(g=1 + (i * 11) % s, q=1 + (i * 5) % s) for i in range(128)]       # records 128 .. 255: blocks of one-segment records only
    for i in (3, 40, 77, 120):
        ones[i] = dict(g=s, q=s - 1 - i % 3)
    plan = cover + a + ones + b
    for k in range(MIN):
        M = big * s if k == 0 else (big - 1) * s + 1                              # 300 segments: of s symbols, the last one full / of one symbol
        for d in (dict(g=M, q=1 + k), dict(g=2 * s + 1, q=s), dict(g=1 + k, q=M), dict(g=3, q=3)):
            if max(d["g"], d["q"]) == M:                                          # its empty chains start a workgroup of 256 chains of the call
                while (sum(cut(x["g"], x["q"], s)[1] for x in plan) + 1) % 256:
                    plan.append(dict(g=2, q=2))
            plan.append(d)
    return plan


def _finish(plan, last_long, s):
    """the text ends in a long record or in a short one, and no block size of BRS divides its record count"""
    plan = list(plan)
    while any(len(plan) % b in (0, b - 1) for b in BRS):
        plan.append(dict(g=s + 1 + len(plan) % 7, q=s + 2))
    plan.append(dict(g=6 * s + 1, q=6 * s - 2) if last_long else dict(g=2, q=3))
    return plan


def _letters(rng, plan, s, variant, pool):
    """-> the text"""
    solid = variant == "colour"
    recs = []
    for r, d in enumerate(plan):
        g, q = d["g"], d["q"]
        _, n, L = cut(g, q, s)
        if pool is None:
            codes = rng.integers(0, 4, g, dtype=np.uint8)
        elif g <= len(pool):
            a = 0 if d.get("cover") else (r * 13) % (len(pool) - g + 1)
            codes = pool[a:a + g].copy()
        else:
            codes = np.tile(pool, -(-g // len(pool)))[:g].copy()
        base = (np.frombuffer(b"0123", np.uint8) if solid else _ACGT)[codes].copy()
        qual = _QS[rng.integers(0, len(_QS), q)].copy()
        kind, place = d.get("exc", ("", ""))
        enn = ord(".") if solid else ord("N")

        def put(k, p):
            if k in ("N", "Nbang"):
                base[p] = enn
            if k in ("bang", "Nbang"):
                qual[p] = ord("!")
            if k == "lc":
                base[p] |= 0x20
        if place in PLACES:
            gn = (g - 1) // L                                 # the base line's last segment
            p = {"first": L * (1 + r % (gn - 1)), "last": L * (r % gn) + L - 1, "tail": gn * L + 1, "only-tail": gn * L + r % (g - gn * L)}[place]
            put(kind, p)
            if place == "tail":
                put(kind, 3)
        elif kind == "lcrun":
            base[2 * L - 3:2 * L + 4] |= 0x20
        elif kind == "bang-behind-bases":
            qual[g + 1 + r % (q - g - 1)] = ord("!")
        elif kind == "N-behind-qualities":
            base[q + 1 + r % (g - q - 1)] = enn
        elif kind == "N-alone":
            base[0] = enn
        bl, ql = base.tobytes(), qual.tobytes()
        if solid:
            bl, ql = b"T" + bl, b"!" + ql
        recs.append(b"@%d\n%s\n+\n%s\n" % (r, bl, ql))
    return b"".join(recs)


def _build(name):
    if name == "capacity":
        return capacity_text()
    variant, s = name.split("-")
    s = int(s)
    rng = np.random.default_rng(sum(name.encode()) * 1009 + s)
    match = variant == "match" or name == "colour-64"
    pool = rng.integers(0, 4, 5 * s + 3, dtype=np.uint8) if match else None
    plan = _finish(_plan(s, variant, 600 if s < 20 else 300), last_long=(s in (16, 64)), s=s)
    fq = _letters(rng, plan, s, variant, pool)
    return dict(name=name, fq=fq, seg=s, solid=variant == "colour", match=match, brs=BRS)


@functools.lru_cache(maxsize=None)
def text(name):
    return _build(name)


# ---- near-capacity qualities ---------------------------------------------------------------------------------------------------------------------
# A chain's output region is a share of its record's TEXT (dev_walk.h chain_region, restated in regions()): twice the share for qualities, three
# quarters of it for bases.  A record of one base whose quality line is many times as long and made of escapes (symbols of 63 and above) fills its
# quality chains' regions as far as legal text does.  Searched on the oracle, levels 1 and 3, the blocks of BRS, segments of 64 and 75, the fullest
# chain's bytes / region:
#   one such record in 100 / 400 / 800, 1 or 3 bases, 100 / 200 / 400 escapes, a header of 1 / 6 / 20 bytes      0.65 .. 0.76 (1 in 400, 1 base, 200, 1 byte)
#   the escapes BEHIND the record's first 4096 qualities, which is as far as the prior's sample looks (PRIOR_SYMBOLS): no row has seen them
#     all escapes 0.927 (segments of 64; 0.917 at 75)    every second one 0.68    two of three 0.77    symbol 62 or 40 .. 62 instead 0.39 .. 0.41
# (Records of the first kind beside one of the second put the escape into the rows the sample builds, and the second kind comes down to 0.83.)
# CAPACITY is the second kind: two records of 1 base, 4096 ordinary qualities and 600 escapes among 420 ordinary ones.
# CAPACITY_RATIO is what that text reaches (test_segment_inputs.py asserts it, and that no chain reaches 1).
CAPACITY = dict(seg=64, at=(150, 301), behind=600, nrec=420)
CAPACITY_RATIO = 0.9274                                      # 115 of 124 bytes, level 1 (level 3: 0.9194)


def capacity_text():
    c = CAPACITY
    rng = np.random.default_rng(c["behind"] * 31 + c["seg"])
    esc = lambda k: (33 + 63 + rng.integers(0, 31, k)).astype(np.uint8).tobytes()
    recs = []
    for r in range(c["nrec"]):
        g = q = 40 + (r * 7) % 100
        qual = _QS[rng.integers(0, len(_QS), q)].tobytes()
        head = b"@%d" % r
        if r in c["at"]:
            g, qual, head = 1, _QS[rng.integers(0, len(_QS), PRIOR_SYMBOLS)].tobytes() + esc(c["behind"]), b"@"
        recs.append(b"%s\n%s\n+\n%s\n" % (head, _ACGT[rng.integers(0, 4, g)].tobytes(), qual))
    return dict(name="capacity", fq=b"".join(recs), seg=c["seg"], solid=False, match=False, brs=BRS)


def capacity_ratio(level, br):
    t = text("capacity")
    return fill_ratio(quality_oracle("capacity", level)[1], regions(t, br, 2, 1))


# ---- what a text is -------------------------------------------------------------------------------------------------------------------------------
def lines(t):
    """(starts, goff, glen, qoff, qlen): the records' first bytes and their base and quality lines as the walkers see them (without a colour-space
    prefix character)"""
    starts, lens = util.line_table(t["fq"])
    s = int(t["solid"])
    return starts[0::4], starts[1::4] + s, lens[1::4] - s, starts[3::4] + s, lens[3::4] - s


def seg_table(t):
    """per record: n, L and the call's first chain of the record -- by cut(), record by record"""
    _, _, glen, _, qlen = lines(t)
    n, L = [], []
    for g, q in zip(glen.tolist(), qlen.tolist()):
        _, k, l = cut(g, q, t["seg"])
        n.append(k); L.append(l)
    off = [0]
    for k in n:
        off.append(off[-1] + k)
    return n, L, off


def regions(t, br, num, den):
    """Every chain's output region in bytes (dev_walk.h chain_region: the record's text in n equal parts, scaled by num / den, between dword
    borders counted from the block's first byte)"""
    rec0 = lines(t)[0].tolist() + [len(t["fq"])]
    n, _, _ = seg_table(t)
    caps = []
    for r, k in enumerate(n):
        t0, tc, ln = rec0[(r // br) * br], rec0[r], rec0[r + 1] - rec0[r]
        for s in range(k):
            a, b = tc + ln * s // k, tc + ln * (s + 1) // k
            lo, hi = ((a - t0) * num // den + 3) & ~3, ((b - t0) * num // den) & ~3
            caps.append(max(0, hi - lo))
    return caps


def fill_ratio(sizes, caps):
    """the fullest chain's bytes / region (an empty chain in an empty region is 0)"""
    top = 0.0
    for sz, cap in zip(sizes, caps):
        if sz:
            top = max(top, float("inf") if not cap else sz / cap)
    return top


@functools.lru_cache(maxsize=None)
def quality_oracle(name, level):
    """(streams, sizes, escapes): the quality chains as the oracle writes them under the prior a prior_step = 1 call counts"""
    t = text(name)
    _, _, glen, qoff, qlen = lines(t)
    rows66 = O.qlt_prior_rows(O.qlt_histogram(t["fq"], qoff, np.minimum(qlen, PRIOR_SYMBOLS), level, 0, 1))
    return O.qlt_encode_segs(t["fq"], qoff, qlen, glen, level, t["seg"], O.qlt_frozen_rows(rows66)) + (O.qlt_frozen_rows(rows66),)


@functools.lru_cache(maxsize=None)
def base_oracle(name, br):
    """(streams, sizes, verdict): the base chains as the oracle writes them (the match model, or two bits a base where its verdict is "off")"""
    t = text(name)
    _, goff, glen, _, qlen = lines(t)
    return O.gm_encode_segs(t["fq"], goff, glen, qlen, gm_table_bits(len(t["fq"])), br, t["seg"])


# ---- what a text claims ---------------------------------------------------------------------------------------------------------------------------
def _events(base, qual, L):
    """the exceptions of one record: [(kind, position)], a lower-case run one event at its first letter -> and the runs [(a, b)]"""
    ev, runs = [], []
    g, q = len(base), len(qual)
    p = 0
    while p < g:
        c = base[p]
        bang = p < q and qual[p] == 0x21
        isn = c in b"Nn."
        if isn:
            ev.append(("Nbang" if bang else "N", p))
        elif bang:
            ev.append(("bang", p))
        if 0x61 <= c <= 0x7a and not isn:
            a = p
            while p + 1 < g and 0x61 <= base[p + 1] <= 0x7a:
                p += 1
            runs.append((a, p + 1))
            ev.append(("lc", a))
        p += 1
    for p in range(g, q):
        if qual[p] == 0x21:
            ev.append(("bang-behind-bases", p))
    return ev, runs


def classes(name):
    """class -> the times it occurs in the text"""
    t = text(name)
    s = t["seg"]
    fq = t["fq"]
    _, goff, glen, qoff, qlen = lines(t)
    goff, glen, qoff, qlen = goff.tolist(), glen.tolist(), qoff.tolist(), qlen.tolist()
    n, Ls, off = seg_table(t)
    nrec = len(n)
    c = {}

    def add(k, by=1):
        c[k] = c.get(k, 0) + by
    empty = {"g": [], "q": []}                               # per stream: is chain i of the call empty
    for r in range(nrec):
        g, q, k, L = glen[r], qlen[r], n[r], Ls[r]
        M, lo = max(g, q), min(g, q)
        dirs = [d for d, yes in (("g", g >= q), ("q", q >= g)) if yes]
        for i in range(k):
            empty["g"].append(piece(g, i, L)[0] == piece(g, i, L)[1])
            empty["q"].append(piece(q, i, L)[0] == piece(q, i, L)[1])
        tags = []
        for tag, v in (("M=1", 1), ("M=s-1", s - 1), ("M=s", s), ("M=s+1", s + 1), ("M=2s-1", 2 * s - 1), ("M=2s", 2 * s), ("M=2s+1", 2 * s + 1)):
            if M == v:
                tags.append(tag)
        if M % s == 0 and M // s >= 5:
            tags.append("M=ks")
        if k >= 2 and k * L == M:
            tags.append("nL=M")
        if k >= 2 and M - (k - 1) * L == 1:
            tags.append("last-seg-1")
        if g == q:
            tags.append("equal")
        if M - lo == 1:
            tags.append("differ-1")
        if k >= 2 and lo < M:
            for j in range(1, k):
                for d, tag in ((0, "short=jL"), (-1, "short=jL-1"), (1, "short=jL+1")):
                    if lo == j * L + d:
                        tags.append(tag)
            if lo < L:
                tags.append("short<L")
            if lo == 1:
                tags.append("short=1")
            gone = k - -(-lo // L)
            if gone >= 70:
                tags.append("empty>=70")
            if gone >= 260:
                tags.append("empty>=260")
        if k >= 300:
            tags.append("segs>=300")
        for tag in tags:
            for d in dirs:
                add(tag + ":" + d)
        if k >= 2 and off[r] < 256 < off[r] + k:
            add("straddle-256")
        if k >= 2 and any(off[r] < 64 * j < off[r] + k for j in range(off[r] // 64, (off[r] + k) // 64 + 1)):
            add("straddle-64j")
        if k == 1 and 0 < r < nrec - 1 and n[r - 1] > 1 and n[r + 1] > 1:
            add("one-seg-between")
        for b in t["brs"]:
            if k == 1 and r % b == 0:
                add("one-seg-first@%d" % b)
            if k == 1 and (r % b == b - 1 or r == nrec - 1):
                add("one-seg-last@%d" % b)
        # exceptions
        base, qual = fq[goff[r]:goff[r] + g], fq[qoff[r]:qoff[r] + q]
        ev, runs = _events(base, qual, L)
        gn = (g - 1) // L
        short_tail = gn >= 1 and g - gn * L < L
        for kind, p in ev:
            if kind == "bang-behind-bases":
                add(kind)
                continue
            if p >= q and kind == "N":
                add("N-behind-qualities")
            if p % L == 0 and p >= L:
                add(kind + "@first")
            if p % L == L - 1 and p + 1 < g:
                add(kind + "@last")
            if short_tail and p // L == gn:
                add(kind + "@tail")
                if len(ev) == 1:
                    add(kind + "@only-tail")
        for a, b in runs:
            if a // L != (b - 1) // L:
                add("lcrun@border")
        if g == 1 and ev and ev[0][0] == "N" and ((r and glen[r - 1] == 300) or (r + 1 < nrec and glen[r + 1] == 300)):
            add("N-alone-by-300")
    for d in "gq":                                            # a whole workgroup of the call's chains empty in one stream
        e = empty[d]
        for j in range(0, len(e) - 255, 256):
            if all(e[j:j + 256]):
                add("aligned-256-empty:" + ("q" if d == "g" else "g"))          # (the bases' chains are empty where the qualities are the longer line)
    for b in t["brs"]:
        for r0 in range(0, nrec, b):
            if all(k == 1 for k in n[r0:r0 + b]) and r0 + b <= nrec:
                add("all-one-seg-block@%d" % b)
        if nrec % b:
            add("short-last-block@%d" % b)
    add("last:long" if n[-1] > 1 else "last:short")
    return c


_DIR = ("M=1", "M=s-1", "M=s", "M=s+1", "M=2s-1", "M=2s", "M=2s+1", "M=ks", "nL=M", "last-seg-1", "equal", "differ-1", "short=jL", "short=jL-1",
        "short=jL+1", "short<L", "short=1", "empty>=70", "empty>=260", "segs>=300")
LENGTH_CLASSES = [k + ":" + d for k in _DIR for d in "gq"]
BLOCK_CLASSES = ["straddle-256", "straddle-64j", "one-seg-between"] + ["%s@%d" % (k, b) for k in ("one-seg-first", "one-seg-last", "all-one-seg-block",
                                                                                                  "short-last-block") for b in BRS]
EXC_CLASSES = ["%s@%s" % (k, p) for k in KINDS for p in PLACES] + ["lcrun@border", "bang-behind-bases", "N-behind-qualities", "N-alone-by-300"]
MIN_OF = {"straddle-256": 1, "last:long": 1, "last:short": 1}
MIN_OF.update({"short-last-block@%d" % b: 1 for b in BRS})
TEXTS = ["match-64", "match-75", "flat-16", "flat-17", "flat-64", "flat-75", "colour-17", "colour-64"]


def claims(name):
    t = text(name)
    out = LENGTH_CLASSES + BLOCK_CLASSES + [k for k in EXC_CLASSES if not (t["solid"] and k.startswith("lc"))]
    out.append("last:long" if t["seg"] in (16, 64) else "last:short")
    return out + ["aligned-256-empty:g", "aligned-256-empty:q"]

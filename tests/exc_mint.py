"""The base-exception lists of the frozen-table mode (exc.hip, dev_rice.h, models_w.hip k_gen_exc_q), stated once more in plain
Python, and texts minted for the edges of that code.  No GPU and no oracle call in here: test_exception_inputs.py holds the rule against the
oracle's C and every text to its claims on the CPU, test_exception_lists.py runs the texts on the GPU.

The rule
  positions(chunk, solid)   gens.cpp:91-114 in numpy: a block's "gen.Ns" (N-like bases whose quality is not '!'), "gen.Nn" (real bases under
                            '!'), "gen.lc" (lowercase bases) as positions counted from 1 over the block's base lines, and its N byte.  A base
                            behind the end of a shorter quality line has quality 40; a '!' behind the end of the bases counts for nothing; 'n'
                            is an 'N' that is lowercase too; in colour space (solid = 1) both lines lose their first character.
  rice_encode / rice_decode the ten lines of exc.hip's header in Python integers; rice_encode reports what a list exercised.
  marked(fq)                the records the framing hands to the pass (frame.hip k_frame<MARKS>, frame_masks.h): a byte of the WHOLE base line
                            with bit 3 set or bits 5 and 6 both set (odd_flags: N, '.', lowercase -- and no A C G T 0 1 2 3), or a byte b of the
                            WHOLE quality line with (b & 0x5e) == 0 (nbang_flags: in 0x21 .. 0x7e that is '!').  Whole line: in colour space the
                            quality line's leading '!' marks every record.
  queue_peaks(flags)        k_gen_exc_q's LDS queue, 64 records a step: the fullest it gets in a block of these marks.

The texts (text(name) -> dict(name, fq, solid, geos, claims); geos[0] is the geometry the claims are counted at).  Bases are iid unless stated.
  edges          blocks of 64 reads of 150 bases; EDGE_BLOCKS says which block's which list reaches what
  far-20         one block of 3.2 M bases: first gaps of 2^20 - 1, 2^20 and 2^21 + 3, one a list (the escape's upper field 0, 1 and 2)
  far-25         one block of 34.6 M bases: the first event 2^25 + 5 bases in, so the gap behind it is coded with k = 24, clamped
  queue          blocks of 192 records with 0, 1, 63, 64, 65, 127, 128, 129, 191 and 192 marked records, the last block of 65 all marked; the
                 record kinds of k_gen_exc_q's edges (QUEUE_KINDS) in the block where every record is marked
  queue-dot      the same plan with '.' as the N byte in base space
  queue-colour   the same plan in colour space: every record is marked, most without an event
                 (One N byte a block is the format's rule, gens.cpp:169, and a block is in colour space by its first record: the second geometry
                 moves the block borders, so '.' and colour space get texts of their own instead of one block each inside `queue`.)
  ragged-flat    blocks of 2001 records for k_gen_exc_decode_r's rec_of: a record of 50 000 bases, then 2000 of 1 to 5; the mirror image; the first again
  ragged-match   the same lengths, bases from a small pool: the match model switches on (its stage keeps a sentinel behind every line)
                 The giant stays below format 6's 65 534; chain_reads is given, so the call does NOT cut it into segments (api.cpp takes
                 segments by itself only where chain_reads is 0).
"""
import functools

import numpy as np

import util

RICE_A0, RICE_KMAX, RICE_ESC = 256, 24, 32
NAMES = ("gen.Ns", "gen.Nn", "gen.lc")
_ACGT = np.frombuffer(b"ACGT", np.uint8)
_DIGITS = np.frombuffer(b"0123", np.uint8)
Q_LO, Q_HI = 35, 33 + 62                                    # qualities: above '!' and '"', below '!' + 62


# ---- the code, restated ------------------------------------------------------------------------------------------------------------------------
class RiceError(ValueError):
    pass


def rice_k(A, N, kmax=RICE_KMAX):
    """the smallest k <= kmax with (N << k) >= A"""
    k = 0
    while k < kmax and (N << k) < A:
        k += 1
    return k


def rice_encode(gaps):
    """-> (bytes, report).  report: ks (every k a gap was coded with), escapes, upper (an escape's upper 20 bits were not 0), q31, bits (the
    list's length in bits before the end mark), steps [(gap, k, q)]."""
    rep = dict(ks=set(), escapes=0, upper=False, q31=False, bits=0, steps=[])
    gaps = [int(g) for g in gaps]
    if not gaps:
        return b"", rep
    acc = n = 0
    A, N = RICE_A0, 1
    for v in gaps + [0]:
        assert 0 <= v < 1 << 40 and (v or n)
        if not v:
            rep["bits"] = n
        k = rice_k(A, N)
        q = v >> k
        if q < RICE_ESC:
            acc |= ((1 << q) - 1) << n                       # q one bits, a zero bit
            n += q + 1
            acc |= (v & ((1 << k) - 1)) << n                 # the low k bits
            n += k
        else:
            acc |= 0xFFFFFFFF << n                           # 32 one bits
            n += 32
            acc |= v << n                                    # v in 40 bits: two fields of 20, the low one first
            n += 40
        if v:
            rep["ks"].add(k); rep["steps"].append((v, k, q))
            rep["escapes"] += q >= RICE_ESC
            rep["upper"] |= q >= RICE_ESC and (v >> 20) != 0
            rep["q31"] |= q == RICE_ESC - 1
        A += v; N += 1
        if N == 32:
            A >>= 1; N >>= 1
    return acc.to_bytes((n + 7) // 8, "little"), rep        # (zero bits up to a byte)


def rice_gaps(blob):
    """The gaps of a stream, one by one (a generator).  Behind the stream's end zeros are read; a list whose end mark does not lie inside the
    stream ends in a RiceError."""
    if not blob:
        return
    acc = int.from_bytes(blob, "little")
    total = 8 * len(blob)
    at = 0
    A, N = RICE_A0, 1
    while True:
        if at > total + 128:
            raise RiceError("end outside the stream")
        k = rice_k(A, N)
        q = 0
        while q < RICE_ESC and (acc >> at) & 1:
            q += 1; at += 1
        if q < RICE_ESC:
            at += 1
            v = (q << k) | ((acc >> at) & ((1 << k) - 1))
            at += k
        else:
            v = (acc >> at) & ((1 << 40) - 1)
            at += 40
        if not v:
            if at > total:
                raise RiceError("end outside the stream")
            return
        yield v
        A += v; N += 1
        if N == 32:
            A >>= 1; N >>= 1


def rice_decode(blob):
    return list(rice_gaps(blob))


def verdict(blob, nbases):
    """What exc.hip's walk says of a list in a block of nbases bases: "ok", "position beyond the block" (its `at > nb`), or "end outside the
    stream" (RiceR's checks) -- whichever comes first."""
    at = 0
    try:
        for g in rice_gaps(blob):
            at += g
            if at > nbases:
                return "position beyond the block"
    except RiceError as e:
        return str(e)
    return "ok"


def gaps_of(pos):
    pos = np.asarray(pos, np.int64)
    return np.diff(pos, prepend=0).tolist()


# ---- the lists, restated -----------------------------------------------------------------------------------------------------------------------
def _lines(chunk, solid):
    starts, lens = util.line_table(chunk)
    s = int(solid)
    f = lambda x: np.maximum(x.astype(np.int64) - s, 0)
    return starts[1::4].astype(np.int64) + s, f(lens[1::4]), starts[3::4].astype(np.int64) + s, f(lens[3::4])


def positions(chunk, solid=0):
    """-> {"gen.Ns", "gen.Nn", "gen.lc": positions from 1 (int64), "n_byte": the block's N character or 0, "nbases"}"""
    a = np.frombuffer(chunk, np.uint8)
    goff, glen, qoff, qlen = _lines(chunk, solid)
    n = len(goff)
    if n and (glen == glen[0]).all() and (qlen == glen[0]).all() and len(a) % n == 0 and (np.diff(goff) == len(a) // n).all():
        rows = a.reshape(n, len(a) // n)                     # records of one shape (the far texts: tens of millions of bases)
        base = rows[:, goff[0]:goff[0] + glen[0]].ravel()
        qual = rows[:, qoff[0]:qoff[0] + glen[0]].ravel()
    else:
        rec = np.repeat(np.arange(n), glen)
        idx = np.arange(int(glen.sum())) - (np.cumsum(glen) - glen)[rec]
        base = a[goff[rec] + idx]
        has = idx < qlen[rec]
        qual = np.where(has, a[np.where(has, qoff[rec] + idx, 0)], 40)       # gens.cpp:153
    lower = (base == ord("a")) | (base == ord("c")) | (base == ord("g")) | (base == ord("t")) | (base == ord("n"))
    is_n = (base == ord("N")) | (base == ord("n")) | (base == ord("."))
    bang = qual == ord("!")
    at = np.flatnonzero(is_n)
    n_byte = 0
    if len(at):
        n_byte = int(base[at[0]])
        n_byte = ord("N") if n_byte == ord("n") else n_byte
    one = lambda m: np.flatnonzero(m).astype(np.int64) + 1
    return {"gen.Ns": one(is_n & ~bang), "gen.Nn": one(~is_n & bang), "gen.lc": one(lower), "n_byte": n_byte, "nbases": len(base)}


def expected(chunk, solid=0):
    """-> ({name: (bytes, report)}, n_byte, nbases) of one block, by positions() and rice_encode() alone"""
    p = positions(chunk, solid)
    return {name: rice_encode(gaps_of(p[name])) for name in NAMES}, p["n_byte"], p["nbases"]


def marked(fq):
    """per record: does the framing mark it for the exception pass"""
    a = np.frombuffer(fq, np.uint8)
    starts, _ = util.line_table(fq)
    odd = ((a & 0x08) != 0) | ((a & 0x60) == 0x60)
    bang = (a & 0x5e) == 0
    nl = a == 10
    odd = np.add.reduceat((odd & ~nl).astype(np.int64), starts.astype(np.int64))
    bang = np.add.reduceat((bang & ~nl).astype(np.int64), starts.astype(np.int64))
    return (odd[1::4] > 0) | (bang[3::4] > 0)


def event_count(bases: bytes, quals: bytes):
    """the events k_gen_exc_q finds in one record (lines without a colour-space prefix): bases that are N-like or lowercase or lie under a '!'"""
    g = np.frombuffer(bases, np.uint8)
    q = np.full(len(g), 40, np.uint8)
    m = min(len(g), len(quals))
    q[:m] = np.frombuffer(quals, np.uint8)[:m]
    return int(np.count_nonzero((g == ord("N")) | (g == ord(".")) | (g >= 0x61) | (q == ord("!"))))


def queue_peaks(flags):
    """k_gen_exc_q over one block's marks: (the most records its queue holds, the takes' sizes in order)"""
    qn = peak = 0
    takes = []
    for k0 in range(0, len(flags), 64):
        qn += int(np.count_nonzero(flags[k0:k0 + 64]))
        peak = max(peak, qn)
        if qn >= 64:
            takes.append(64); qn -= 64
    if qn:
        takes.append(qn)
    return peak, takes


def block_chunks(t, br):
    fq = t["fq"]
    return [fq] if br >= t["nrec"] else util.split_records(fq, br)


# ---- assembling a text ---------------------------------------------------------------------------------------------------------------------------
def _join(heads, bases, quals, solid=False):
    pb, pq = (b"T", b"!") if solid else (b"", b"")
    return b"".join(b"%s\n%s%s\n+\n%s%s\n" % (h, pb, g, pq, q) for h, g, q in zip(heads, bases, quals))


def _cut(arr, lens):
    arr = arr.tobytes()
    out, at = [], 0
    for n in lens:
        out.append(arr[at:at + n]); at += n
    return out


# ---- edges -------------------------------------------------------------------------------------------------------------------------------------
EDGE_BR, EDGE_LEN = 64, 150
EDGE_B = EDGE_BR * EDGE_LEN                                  # bases a block
K0_RUN = 150                                                 # adjacent events in front of the k = 0 gaps (143 unit gaps bring k down to 0)


def _fit(residue, mod, first, step=2):
    """gaps [first, g, g, ...] (g a multiple of `step`: the positions keep first's parity) whose bit length before the end mark is residue mod `mod`"""
    for m in range(3, 40):
        for g in range(step, 400, step):
            gaps = [first] + [g] * m
            if sum(gaps) <= EDGE_B and rice_encode(gaps)[1]["bits"] % mod == residue:
                return np.cumsum(gaps)
    raise AssertionError("no list of that bit length")


def _edge_plan():
    """per block: {list name: positions}"""
    run = np.arange(1, K0_RUN + 1)
    rng = np.random.default_rng(410)
    same = np.cumsum(rng.choice([1, 2, 3, 40, 300], 60))    # one list, coded as each of the three kinds
    spread = lambda n, first: first + 74 * np.arange(n)
    plan = [
        {"gen.Ns": [8191], "gen.Nn": [8192], "gen.lc": [8192]},
        {"gen.Ns": np.append(run, K0_RUN + 31), "gen.Nn": [EDGE_B], "gen.lc": np.append(run, K0_RUN + 32)},
        {"gen.Ns": spread(31, 1000), "gen.Nn": np.append(run, K0_RUN + 32), "gen.lc": spread(32, 2)},
        {"gen.Ns": spread(33, 1000), "gen.Nn": [1], "gen.lc": _fit(0, 8, 3)},
        {"gen.Ns": _fit(0, 32, 2), "gen.Nn": _fit(31, 32, 1), "gen.lc": _fit(31, 32, 7)},
        {"gen.Ns": [], "gen.Nn": np.arange(1, EDGE_B + 1), "gen.lc": np.arange(1, EDGE_B + 1)},
        {"gen.Ns": same, "gen.Nn": [], "gen.lc": []},
        {"gen.Ns": [], "gen.Nn": same, "gen.lc": []},
        {"gen.Ns": [], "gen.Nn": [], "gen.lc": same},
        {"gen.Ns": [700, 900], "gen.Nn": [], "gen.lc": [700, 900, 1100], "Nbang": [300, 1100]},        # 'n' under a real quality; 'N' and 'n' under '!'
        {"gen.Ns": [], "gen.Nn": [], "gen.lc": []},
    ]
    return plan


# claim -> (block, list); test_exception_inputs.py asserts each from rice_encode's report
EDGE_BLOCKS = {
    "first gap 8191: q = 31 at k = 8, no escape": (0, "gen.Ns"), "first gap 8192: escape at k = 8": (0, "gen.Nn"),
    "gap 31 at k = 0: q = 31": (1, "gen.Ns"), "gap 32 at k = 0: escape": (2, "gen.Nn"),
    "1 entry": (3, "gen.Nn"), "31 entries": (2, "gen.Ns"), "32 entries": (2, "gen.lc"), "33 entries": (3, "gen.Ns"),
    "bits = 0 mod 8": (3, "gen.lc"), "bits = 0 mod 32": (4, "gen.Ns"), "bits = 31 mod 32": (4, "gen.Nn"),
    "dense Nn": (5, "gen.Nn"), "dense lc": (5, "gen.lc"),
    "same list as Ns": (6, "gen.Ns"), "same list as Nn": (7, "gen.Nn"), "same list as lc": (8, "gen.lc"),
    "n in two lists": (9, "gen.Ns"), "no event": (10, "gen.Ns"),
}


def _edges():
    plan = _edge_plan()
    rng = np.random.default_rng(41)
    nb = len(plan) * EDGE_B
    base = _ACGT[rng.integers(0, 4, nb)].copy()
    qual = rng.integers(Q_LO, Q_HI, nb).astype(np.uint8)
    for b, lists in enumerate(plan):
        o = b * EDGE_B - 1
        ns, nn, lc, nbang = (np.asarray(lists.get(k, []), np.int64) for k in NAMES + ("Nbang",))
        assert not set(ns.tolist()) & set(nn.tolist()) and all(len(x) == 0 or (x.min() >= 1 and x.max() <= EDGE_B) for x in (ns, nn, lc, nbang))
        base[o + ns] = ord("N"); base[o + nbang] = ord("N")
        qual[o + nn] = ord("!"); qual[o + nbang] = ord("!")
        base[o + lc] |= 0x20
    nrec = nb // EDGE_LEN
    fq = _join([b"@e%d" % r for r in range(nrec)], _cut(base, [EDGE_LEN] * nrec), _cut(qual, [EDGE_LEN] * nrec))
    return dict(fq=fq, solid=0, geos=((EDGE_BR, 16), (100, 7)), claims=EDGE_BLOCKS, plan=plan)


# ---- far ---------------------------------------------------------------------------------------------------------------------------------------
_M = 1 << 20
# per list: its gaps.  A list's FIRST gap is coded with k = 8, whatever its size; behind a gap of 2^20 the parameter is 19 or more and nothing escapes
FAR = {"far-20": dict(nrec=21100, lists={"gen.Ns": (_M - 1, 2 * _M + 3), "gen.Nn": (_M, 5), "gen.lc": (2 * _M + 3, _M - 1)}),
       "far-25": dict(nrec=230700, lists={"gen.Ns": (32 * _M + 5, 1000, _M // 2), "gen.Nn": (32 * _M + 6, 1000, _M // 2),
                                          "gen.lc": (32 * _M + 5, 1000, _M // 2)})}


def _far(name):
    """One block of reads of 150 bases, all of one shape (a header "@f"): a table of nrec rows, filled column-wise."""
    nrec, lists = FAR[name]["nrec"], FAR[name]["lists"]
    rng = np.random.default_rng(len(name) + nrec)
    L = EDGE_LEN
    rows = np.empty((nrec, 3 + L + 3 + L + 1), np.uint8)
    rows[:, 0:3] = np.frombuffer(b"@f\n", np.uint8)
    rows[:, 3:3 + L] = _ACGT[rng.integers(0, 4, (nrec, L), dtype=np.uint8)]
    rows[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rows[:, 6 + L:6 + 2 * L] = rng.integers(Q_LO, Q_HI, (1024, L), dtype=np.uint8)[np.arange(nrec) % 1024]
    rows[:, 6 + 2 * L] = 10
    claims = {ln: np.cumsum(np.asarray(g, np.int64)) for ln, g in lists.items()}
    assert max(int(p[-1]) for p in claims.values()) <= nrec * L and not set(claims["gen.Ns"].tolist()) & set(claims["gen.Nn"].tolist())
    for ln, col, put in (("gen.Ns", 3, lambda c: ord("N")), ("gen.Nn", 6 + L, lambda c: ord("!")), ("gen.lc", 3, lambda c: c | 0x20)):
        for p in claims[ln].tolist():
            r, c = (p - 1) // L, col + (p - 1) % L
            rows[r, c] = put(int(rows[r, c]))
    return dict(fq=rows.tobytes(), solid=0, geos=((nrec, 64),), claims=claims)


# ---- queue -------------------------------------------------------------------------------------------------------------------------------------
QUEUE_BR = 192
# per block: the marked records of its three 64-record steps (None: the last block, 65 records, all marked)
QUEUE_STEPS = [(0, 0, 0), (0, 0, 1), (63, 0, 0), (63, 1, 0), (63, 2, 0), (63, 64, 0), (63, 64, 1), (63, 64, 2), (63, 64, 64), (64, 64, 64), None]
QUEUE_MARKED = [0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 65]
QUEUE_PEAK = [0, 1, 63, 64, 65, 127, 127, 127, 127, 64, 64]
QUEUE_ALL = 9                                                # the block where every record is marked: the record kinds lie here
# record of QUEUE_ALL -> kind.  10 / 11: nine events next to 1025 bases, both in the block's first take of 64
QUEUE_KINDS = {3: "8 events", 5: "9 events", 7: "ninth event in the last sixteen-byte step", 10: "9 events", 11: "1025 bases", 20: "1024 bases",
               30: "no event: '!' behind the bases", 31: "no event: '!' behind the bases", 40: "short quality line", 41: "header of '!'",
               70: "1025 bases", 71: "8 events", 100: "90 events", 130: "short quality line", 131: "header of '!'"}


def _queue(variant):
    colour = variant == "colour"
    letters = _DIGITS if colour else _ACGT
    enn = ord("N") if variant == "N" else ord(".")
    rng = np.random.default_rng(77 + len(variant))
    heads, bases, quals, kinds = [], [], [], {}
    want = []                                                # per record: marked by construction
    for b, steps in enumerate(QUEUE_STEPS):
        n = 65 if steps is None else QUEUE_BR
        for i in range(n):
            r = len(heads)
            m = True if steps is None else i % 64 < steps[i // 64]
            kind = QUEUE_KINDS.get(i, "") if b == QUEUE_ALL else ""
            ln = {"1024 bases": 1024, "1025 bases": 1025, "90 events": 300}.get(kind, 100 + (r * 7) % 97)
            g = letters[rng.integers(0, 4, ln)].copy()
            ql = ln
            if kind.startswith("no event"):
                ql = ln + 9
            if kind == "short quality line":
                ql = ln - 12
            q = rng.integers(Q_LO, Q_HI, ql).astype(np.uint8)
            head = b"@q%d" % r
            if kind == "header of '!'":
                head = b"@!!!!!!!!!!!!!!!!!!!!q%d" % r           # what a walk past the quality line before it would read as qualities

            def event(p, w):
                """w: 0 N, 1 N under '!', 2 '!' over a base, 3 lowercase, 4 lowercase under '!', 5 'n'"""
                if colour:
                    w = w % 3
                if w == 5 and variant != "N":
                    w = 3
                if w in (0, 1):
                    g[p] = enn
                if w in (1, 2, 4) and p < ql:
                    q[p] = ord("!")
                if w in (3, 4):
                    g[p] |= 0x20
                if w == 5:
                    g[p] = ord("n")
            if kind in ("8 events", "9 events", "90 events"):
                for j, p in enumerate(rng.choice(ln, int(kind.split()[0]), replace=False).tolist()):
                    event(p, (r + j) % 6)
            elif kind.startswith("ninth"):
                last = 16 * ((ln - 1) // 16)
                for j, p in enumerate(rng.choice(last, 8, replace=False).tolist() + [last + (ln - 1 - last) // 2]):
                    event(p, (r + j) % 6)
            elif kind in ("1024 bases", "1025 bases"):
                for j, p in enumerate((0, 511, ln - 1)):
                    event(p, (r + j) % 6)
            elif kind.startswith("no event"):
                q[ln + 2] = q[ql - 1] = ord("!")
            elif kind == "short quality line":
                event(ql + 1, 0); event(ql + 5, 3); event(3, 2)       # an N and a lowercase base behind the quality line's end: quality 40
            elif m:
                event(int(rng.integers(0, ln)), r % 6)
                if r % 5 == 0:
                    event(int(rng.integers(0, ln)), (r // 5) % 6)
            heads.append(head); bases.append(g.tobytes()); quals.append(q.tobytes()); want.append(m)
            if kind:
                kinds[r] = kind
    fq = _join(heads, bases, quals, colour)
    return dict(fq=fq, solid=int(colour), geos=((QUEUE_BR, 64), (191, 7)), claims=dict(marked=np.array(want), kinds=kinds, variant=variant))


# ---- ragged ------------------------------------------------------------------------------------------------------------------------------------
RAGGED_GIANT, RAGGED_SMALL = 50000, 2000
RAGGED_ONES = (600, 900)                                     # the small records [600, 900) of a block hold one base each


def _ragged(match):
    rng = np.random.default_rng(50 + match)
    pool = rng.integers(0, 4, 400)
    small = [1 if RAGGED_ONES[0] <= i < RAGGED_ONES[1] else 1 + (i * 7) % 5 for i in range(RAGGED_SMALL)]
    lens = [RAGGED_GIANT] + small + small + [RAGGED_GIANT] + [RAGGED_GIANT] + small     # (a third block, without events: the match model asks for
    nrec = len(lens)                                                                     #  three generations before it gives a verdict, gm.hip)
    br = nrec // 3
    bases, quals, where = [], [], {}
    first = np.cumsum([0] + lens)
    for r, ln in enumerate(lens):
        if match:
            a = (r * 13) % 300
            code = np.tile(pool, -(-(a + ln) // len(pool)))[a:a + ln]
        else:
            code = rng.integers(0, 4, ln)
        bases.append(_ACGT[code].copy()); quals.append(rng.integers(Q_LO, Q_HI, ln).astype(np.uint8))
    # events: (record, base of the record); every one lowercase, every second an 'n' (gen.Ns), the others under '!' (gen.Nn)
    g0, g1 = 0, 2 * br - 1
    ev = {"block's first base": [(0, 0), (br, 0)], "block's last base": [(br - 1, lens[br - 1] - 1), (g1, RAGGED_GIANT - 1)],
          "giant's first base": [(g0, 0), (g1, 0)], "giant's last base": [(g0, RAGGED_GIANT - 1), (g1, RAGGED_GIANT - 1)],
          "neighbour's first base": [(g0 + 1, 0), (g1 - 1, 0)], "neighbour's last base": [(g0 + 1, lens[g0 + 1] - 1), (g1 - 1, lens[g1 - 1] - 1)],
          "inside the giant": [(g0, 100), (g0, 12345), (g0, 12346), (g0, 25000), (g0, 25001), (g0, 49000), (g1, 1), (g1, 2), (g1, 30000), (g1, 30001), (g1, 40000)],
          "inside a run of one-base records": [(1 + i, 0) for i in (600, 650, 651, 652, 700, 701, 898, 899)] + [(br + i, 0) for i in (600, 601, 750, 751, 752, 753, 898, 899)]}
    done = set()
    for j, (r, p) in enumerate(x for v in ev.values() for x in v):
        if (r, p) in done:
            continue
        done.add((r, p))
        if j % 2:
            quals[r][p] = ord("!"); bases[r][p] |= 0x20
        else:
            bases[r][p] = ord("n")
    for k, v in ev.items():
        where[k] = [(r // br, int(first[r] - first[(r // br) * br]) + p + 1) for r, p in v]       # (block, position in the block)
    fq = _join([b"@r%d" % r for r in range(nrec)], [x.tobytes() for x in bases], [x.tobytes() for x in quals])
    return dict(fq=fq, solid=0, geos=((br, 64),), claims=dict(where=where, match=bool(match)))


_BUILD = {"edges": _edges, "far-20": lambda: _far("far-20"), "far-25": lambda: _far("far-25"), "queue": lambda: _queue("N"),
          "queue-dot": lambda: _queue("dot"), "queue-colour": lambda: _queue("colour"), "ragged-flat": lambda: _ragged(0),
          "ragged-match": lambda: _ragged(1)}
TEXTS = tuple(_BUILD)
SMALL = ("edges", "queue", "queue-dot", "queue-colour", "ragged-flat", "ragged-match")
QUEUES = ("queue", "queue-dot", "queue-colour")


@functools.lru_cache(maxsize=None)
def text(name):
    t = _BUILD[name]()
    t["name"] = name
    t["nrec"] = t["fq"].count(b"\n") // 4
    return t


@functools.lru_cache(maxsize=None)
def lists(name, br):
    """per block of `br` records: ({list: (bytes, report)}, n_byte, nbases) -- computed once, shared by the tests"""
    t = text(name)
    return [expected(c, t["solid"]) for c in block_chunks(t, br)]

"""Texts of more than 4 GiB for the device entries (test_large_texts.py; test_large_text_inputs.py holds all of this to its word on
the CPU).  No tests in here.

A text is head + tile * k + tail: three host pieces of whole records (whole pairs where the text is paired), the tile of ODD length, so
that its copies fall on every phase of the kernels' 16-byte units, 1 KiB rows and 16 KiB spans.  Only the pieces exist on the host; the
text is laid out on the device (Tiled.device).  The head is one record (one pair) whose first header is padded until byte 2^32 of the
text -- MARK -- is the byte the caller asks for: inside a base line, inside a quality line, a record's first byte or a '\\n'.

A pass f that treats every record (pair) by itself gives f(head) + f(tile) * k + f(tail): equal_tiled compares a result with that, chunk
by chunk, without either side ever being whole on the host; the same code runs on numpy arrays (the host twin the CPU tests plant
differences in) and on torch tensors.  crc32_tiled is zlib.crc32 fed piece by piece."""
import bisect
import zlib

import numpy as np

from test_overlap import bases, mates
from test_pairs import record, records
from test_trim import ADAPTER

MARK = 1 << 32
PLACES = ("base", "qual", "first", "newline")
CHUNK = 64 << 20


# ---- the pieces ------------------------------------------------------------------------------------------------------------------

def rec(hdr, b, q):
    assert len(b) == len(q)
    return hdr + b"\n" + b + b"\n+\n" + q + b"\n"


def _spoil(rng, b, q):
    """N, n, lower case and '!' into a read; a run of low qualities at either end now and then"""
    b, q = bytearray(b), bytearray(q)
    L = len(b)
    for p in rng.integers(0, L, int(rng.integers(0, 4))):
        w = int(rng.integers(0, 5))
        if w == 0: b[p] = ord("N")
        elif w == 1: b[p] = ord("n")
        elif w == 2: b[p] |= 0x20
        elif w == 3: q[p] = ord("!")
        else: b[p] = ord("N"); q[p] = ord("!")
    if rng.integers(0, 3) == 0:
        n = int(rng.integers(1, 12))
        q[-n:] = b"#" * min(n, L)
    if rng.integers(0, 4) == 0:
        n = int(rng.integers(1, 6))
        q[:n] = b"%" * min(n, L)
    return bytes(b), bytes(q)


def pair_tile(npairs, seed, tag=b"t"):
    """npairs pairs named tag<i>/1 and tag<i>/2, of 1 .. 160 bases: inserts shorter than the reads (read-through, an adapter behind some),
    inserts the mates overlap in, mates that lie apart, and ragged pairs of random reads; N, n, lower case and '!' among them."""
    rng = np.random.default_rng(seed)
    genome = bases(rng, 3000)
    out = []
    for i in range(npairs):
        kind = i % 4
        if kind == 3:
            a, b = bases(rng, int(rng.integers(1, 161))), bases(rng, int(rng.integers(1, 161)))
        else:
            La, Lb = int(rng.integers(40, 161)), int(rng.integers(40, 161))
            ins = int(rng.integers(20, min(La, Lb))) if kind == 0 else \
                int(rng.integers(max(La, Lb), La + Lb - 30)) if kind == 1 else int(rng.integers(La + Lb + 1, La + Lb + 200))
            at = int(rng.integers(0, len(genome) - ins))
            frag = genome[at:at + ins]
            a, b = mates(rng, frag, La, Lb)
            if kind == 0 and i % 8 == 0:
                a = (frag + ADAPTER * 6)[:La]                                 # the read-through is the adapter
        for x, t in ((a, b"/1"), (b, b"/2")):
            q = rng.integers(ord("!") + 28, ord("J") + 1, len(x), dtype=np.uint8).tobytes()
            x, q = _spoil(rng, x, q)
            out.append(rec(b"@" + tag + b"%d" % i + t + (b" x:%d" % (i % 7) if i % 5 == 0 else b""), x, q))
    return odd(b"".join(out))


def odd(fq):
    """the text with a byte more behind its first name where its length is even: the name itself stays"""
    if len(fq) % 2:
        return fq
    e = fq.index(b"\n")
    return fq[:e] + (b"o" if b" " in fq[:e] else b" ") + fq[e:]


def read_tile(n, lo, hi, seed, tag=b"a", mate=b"/1"):
    """n single reads of lo .. hi bases named tag<i><mate> (test_pairs.record)"""
    rng = np.random.default_rng(seed)
    return odd(b"".join(record(rng, int(rng.integers(lo, hi + 1)), b"@" + tag + b"%d" % i + mate) for i in range(n)))


def tiny_tile(n, tag=b"a", mate=b"/2"):
    """n reads of one base: the second input of the interleave"""
    return b"".join(rec(b"@" + tag + b"%d" % i + mate, b"ACGT"[i % 4:i % 4 + 1], b"I") for i in range(n))


def genome_tile(n, length, seed, qlen=3):
    """n genome-like records for the match model (the style of test_frozen_tables._folded_genome_reads: rotated reads of a few sources):
    base lines of `length` bases, quality lines of qlen bytes -- the block format takes unequal lines"""
    rng = np.random.default_rng(seed)
    src = [bases(rng, length) for _ in range(8)]
    out = []
    for i in range(n):
        s, r = src[int(rng.integers(len(src)))], int(rng.integers(0, 40))
        out.append(b"@g%d\n" % i + s[r:] + s[:r] + b"\n+\n" + b"I5?!"[:qlen] + b"\n")
    return odd(b"".join(out))


# ---- the text --------------------------------------------------------------------------------------------------------------------

class Tiled:
    """head + tile * k + tail.  off[i], first[i]: the byte offset and the record number at which piece i begins, the pieces being the
    head, copy 0 .. copy k - 1 of the tile and the tail (copy_off / copy_first give them by arithmetic; nobody lists 40 000 copies)."""

    def __init__(self, head, tile, k, tail):
        self.head, self.tile, self.k, self.tail = head, tile, k, tail
        self.rh, self.rt, self.rl = records(head) if head else [], records(tile), records(tail) if tail else []
        assert (b"".join(self.rh), b"".join(self.rt), b"".join(self.rl)) == (head, tile, tail)
        self.H, self.T, self.L = len(head), len(tile), len(tail)
        self.nbytes = self.H + k * self.T + self.L
        self.nrec = len(self.rh) + k * len(self.rt) + len(self.rl)
        self._starts = np.cumsum([0] + [len(r) for r in self.rt]).tolist()

    @property
    def pieces(self):
        return self.head, self.tile, self.tail

    def copy_off(self, c):
        """where copy c of the tile begins (c == k: the tail)"""
        assert 0 <= c <= self.k
        return self.H + c * self.T

    def copy_first(self, c):
        assert 0 <= c <= self.k
        return len(self.rh) + c * len(self.rt)

    def tables(self):
        """(offsets, first records) of every piece, the text's end behind them: for a small k"""
        off = [0] + [self.copy_off(c) for c in range(self.k + 1)] + [self.nbytes]
        first = [0] + [self.copy_first(c) for c in range(self.k + 1)] + [self.nrec]
        return off, first

    def record(self, r):
        assert 0 <= r < self.nrec
        if r < len(self.rh):
            return self.rh[r]
        r -= len(self.rh)
        if r < self.k * len(self.rt):
            return self.rt[r % len(self.rt)]
        return self.rl[r - self.k * len(self.rt)]

    def records(self, first, n):
        """the bytes of records [first, first + n)"""
        return b"".join(self.record(r) for r in range(first, first + n))

    def record_off(self, r):
        """the byte offset of record r"""
        assert 0 <= r <= self.nrec
        if r <= len(self.rh):
            return sum(len(x) for x in self.rh[:r])
        q = r - len(self.rh)
        if q <= self.k * len(self.rt):
            c, j = divmod(q, len(self.rt))
            return self.H + c * self.T + self._starts[j]
        return self.H + self.k * self.T + sum(len(x) for x in self.rl[:q - self.k * len(self.rt)])

    def locate(self, at):
        """(record, line 1 .. 4, offset inside the line, the line's length with its '\\n') of byte `at`, by arithmetic"""
        assert self.H <= at < self.H + self.k * self.T, "the byte lies in the head or the tail"
        c, o = divmod(at - self.H, self.T)
        j = bisect.bisect_right(self._starts, o) - 1
        o -= self._starts[j]
        for line, l in enumerate(self.rt[j].split(b"\n")[:4]):
            if o <= len(l):
                return self.copy_first(c) + j, line + 1, o, len(l) + 1
            o -= len(l) + 1
        raise AssertionError

    def mark(self):
        return self.locate(MARK)

    def text(self):
        """the whole text on the host: for a small k alone"""
        assert self.nbytes < 1 << 28
        return self.head + self.tile * self.k + self.tail

    def device(self):
        """the text as a torch uint8 tensor on the device: the pieces uploaded, the tile copied k times there"""
        import torch
        t = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        for off, piece in ((0, self.head), (self.H + self.k * self.T, self.tail)):
            if piece:
                t[off:off + len(piece)] = to_device(piece)
        t[self.H:self.H + self.k * self.T].view(self.k, self.T)[:] = to_device(self.tile)
        return t


def to_device(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def placed(tile, tail, place, head_pair=True, mark=MARK, spare=2, min_line=8):
    """The Tiled whose byte `mark` is, as `place` says, inside a base line, inside a quality line, a record's first byte or a '\\n', and
    that is `mark` + `spare` tiles long or longer.  The head's first header is padded; of the tile's records the one that needs the
    shortest pad is taken."""
    T = len(tile)
    assert T % 2 == 1 and place in PLACES
    h0 = [rec(b"@head/1", b"ACGTNacgtn" * 3, b"IIIII5555!" * 3)] + ([rec(b"@head/2", b"TTGCA", b"I5I5!")] if head_pair else [])
    H0 = sum(len(x) for x in h0)
    best = None
    s = 0
    for r in records(tile):
        l = r.split(b"\n")
        if place == "first":
            t = s
        elif place == "newline":
            t = s + len(l[0]) + 1 + len(l[1])                                 # the '\n' behind the base line
        elif len(l[1]) >= min_line and len(l[3]) >= 3:
            t = s + len(l[0]) + 1 + len(l[1]) // 2 if place == "base" else s + len(l[0]) + len(l[1]) + 4 + len(l[3]) // 2
        else:
            t = None
        if t is not None:
            pad = (mark - H0 - t) % T
            if best is None or pad < best:
                best = pad
        s += len(r)
    head = h0[0][:5] + b"h" * best + h0[0][5:] + b"".join(h0[1:])
    k = -(-(mark + spare * T - len(head) - len(tail)) // T)
    return Tiled(head, tile, k, tail)


# ---- comparing a tiled result ----------------------------------------------------------------------------------------------------------

class NumpyOps:
    """the host twin: arrays are numpy's"""

    @staticmethod
    def put(b):
        return np.frombuffer(b, np.uint8)

    @staticmethod
    def repeat(a, n):
        return np.tile(a, n)

    @staticmethod
    def first_diff(a, b):
        d = np.flatnonzero(a != b)
        return int(d[0]) if len(d) else None

    @staticmethod
    def take(a, lo, hi):
        return a[lo:hi].tobytes()


class TorchOps:
    """arrays are torch tensors on the device; 32 bytes come back on a mismatch, a flag otherwise"""

    @staticmethod
    def put(b):
        return to_device(b)

    @staticmethod
    def repeat(a, n):
        return a.repeat(n)

    @staticmethod
    def first_diff(a, b):
        import torch
        if torch.equal(a, b):
            return None
        return int((a != b).nonzero()[0].item())

    @staticmethod
    def take(a, lo, hi):
        return a[lo:hi].cpu().numpy().tobytes()


def chunk_plan(lens, k, chunk):
    """[(offset in the result, piece 0 / 1 / 2, first copy, copies)]: the head, the tile's copies `chunk` bytes or one copy at a
    time, the tail; pieces of no bytes are left out"""
    lh, lt, ll = lens
    plan = [(0, 0, 0, 1)] if lh else []
    per = max(1, chunk // lt) if lt else 0
    c = 0
    while lt and c < k:
        n = min(per, k - c)
        plan.append((lh + c * lt, 1, c, n))
        c += n
    return plan + ([(lh + k * lt, 2, 0, 1)] if ll else [])


def expected_bytes(pieces, k, lo, hi):
    """bytes [lo, hi) of head' + tile' * k + tail', from the pieces (a few bytes: the excerpt of a mismatch)"""
    lh, lt = len(pieces[0]), len(pieces[1])
    out, at = [], lo
    while at < hi:
        if at < lh:
            piece, o = pieces[0], at
        elif at < lh + k * lt:
            piece, o = pieces[1], (at - lh) % lt
        else:
            piece, o = pieces[2], at - lh - k * lt
        out.append(piece[o:o + hi - at])
        assert out[-1]
        at += len(out[-1])
    return b"".join(out)


def equal_tiled(got, pieces, k, what, ops, chunk=CHUNK):
    """got[0 : len(head') + k * len(tile') + len(tail')] against head' + tile' * k + tail' (pieces: the three as host bytes), a chunk
    at a time.  AssertionError at the first byte that differs: its offset as a 64-bit number, the copy and the offset inside the
    copy, 32 bytes of either side from there."""
    lens = [len(p) for p in pieces]
    total = lens[0] + k * lens[1] + lens[2]
    assert len(got) >= total, "%s: the result holds %d bytes, %d are expected" % (what, len(got), total)
    dev = [ops.put(p) if p else None for p in pieces]
    many = None
    for off, piece, c0, n in chunk_plan(lens, k, chunk):
        if piece != 1 or n == 1:
            want = dev[piece]
        else:
            if many is None:
                many = ops.repeat(dev[1], n)                                  # the first chunk is the longest
            want = many[:n * lens[1]]
        d = ops.first_diff(got[off:off + len(want)], want)
        if d is not None:
            at = off + d
            c, o = (c0 + d // lens[1], d % lens[1]) if piece == 1 else (None, d)
            where = "copy %d of the tile, offset %d inside it" % (c, o) if piece == 1 else "offset %d inside the %s" % (o, ("head", "", "tail")[piece])
            raise AssertionError("%s: the first byte that differs is at %d (0x%x) of %d: %s; got %r, want %r" % (
                what, at, at, total, where, ops.take(got, at, min(at + 32, total)), expected_bytes(pieces, k, at, min(at + 32, total))))
    return total


def device_equal_tiled(got, pieces, k, what, chunk=CHUNK):
    return equal_tiled(got, pieces, k, what, TorchOps, chunk)


def equal_bytes(got, off, want, what, ops):
    """got[off : off + len(want)] against the host bytes `want` (a small result)"""
    assert len(got) >= off + len(want), "%s: the result holds %d bytes, %d are expected" % (what, len(got), off + len(want))
    if not want:
        return
    d = ops.first_diff(got[off:off + len(want)], ops.put(want))
    if d is not None:
        raise AssertionError("%s: the first byte that differs is at %d (0x%x), %d of %d of the window; got %r, want %r" % (
            what, off + d, off + d, d, len(want), ops.take(got, off + d, min(off + d + 32, off + len(want))), want[d:d + 32]))


def device_equal_bytes(got, off, want, what):
    equal_bytes(got, off, want, what, TorchOps)


def device_all(t, value):
    """every byte of the device tensor is `value` (the guards behind a result; an output that a refused call must leave alone)"""
    return bool((t == value).all().item())


def summed(h, t, k, l):
    """report(head) + k * report(tile) + report(tail), field by field (fields are numbers or lists of them)"""
    if isinstance(t, (list, tuple)):
        return type(t)(summed(a, b, k, c) for a, b, c in zip(h, t, l))
    return h + k * t + l


# ---- CRC ---------------------------------------------------------------------------------------------------------------------------

def crc32_tiled(pieces, k, stops=()):
    """(zlib.crc32 of head + tile * k + tail, [zlib.crc32 of its first s bytes for s in stops]): zlib fed piece by piece, in one pass"""
    head, tile, tail = pieces
    stops = list(stops)
    assert stops == sorted(stops)
    out, c, at = [], 0, 0
    for piece in [head] + [tile] * k + [tail]:
        while stops and len(out) < len(stops) and stops[len(out)] <= at + len(piece):
            out.append(zlib.crc32(piece[:stops[len(out)] - at], c))
        c = zlib.crc32(piece, c)
        at += len(piece)
    assert len(out) == len(stops)
    return c, out


# ---- the texts and the rules of the cases ------------------------------------------------------------------------------------------------

def _rules():
    from slimfastq_amd.capi import Overlap, Select, Trim, SELECT_BOTH
    from test_trim_decode import RULE
    return (Trim(**RULE), Select(min_len=30, max_n=1, min_mean_q_x100=3350, motif=b"GGAC", motif_rc=True, pairs=SELECT_BOTH),
            Overlap(cut=1), Overlap(cut=0))


TRIM, SELECT, OVERLAP, OVERLAP_COUNT = _rules()
U_BLOCK_READS, U_CHAIN_READS = 128, 32
L_BLOCK_READS, L_CHAIN_READS = 64, 8


def _s(place):
    return placed(pair_tile(300, seed=46), pair_tile(3, seed=47, tag=b"z"), place)


def _a():
    tile = read_tile(2000, 100, 160, seed=48)
    return Tiled(b"", tile, -(-(MARK + 2 * len(tile)) // len(tile)), b"")


def _b():
    a = text("A")
    return Tiled(b"", odd(tiny_tile(len(a.rt))), a.k, b"")


def _u():
    from test_frozen_tables import _exception_heavy_fastq
    return placed(odd(_exception_heavy_fastq(4 * U_BLOCK_READS, 49)), _exception_heavy_fastq(70, 50), "base", head_pair=False)


def _l():
    head, tile, tail = genome_tile(1, 5000, 51), genome_tile(150, 5000, 52), genome_tile(3, 5000, 53)
    stage = lambda fq: sum(len(r.split(b"\n")[1]) + 1 for r in records(fq))
    return Tiled(head, tile, -(-(MARK - stage(head) - stage(tail)) // stage(tile)) + 2, tail)


# name -> (builder, paired, where the mark lies; None: nowhere in particular)
TEXTS = {"S:base": (lambda: _s("base"), True, "base"), "S:qual": (lambda: _s("qual"), True, "qual"), "S:first": (lambda: _s("first"), True, "first"),
         "S:newline": (lambda: _s("newline"), True, "newline"), "A": (_a, False, None), "B": (_b, False, None), "U": (_u, False, "base"),
         "L": (_l, False, None)}
_built = {}


def text(name):
    """the Tiled of a name, built once (host pieces alone)"""
    if name not in _built:
        _built[name] = TEXTS[name][0]()
    return _built[name]

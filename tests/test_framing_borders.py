"""GPU: the framing kernel (frame.hip k_frame) at the smallest shapes where its mask assembly and its handovers can go wrong.

k_frame reads the text 16 bytes a lane, tests every dword for line ends, '@', '+', '!' candidates and odd-base candidates, gathers
the flags into 16-bit masks per 16-byte piece and 64-bit masks per 64-byte window, and hands line numbers and "a line starts
here" from window to window, wave to wave, 16 KiB sub-tile to sub-tile and 64 KiB tile to tile.  Every text here is at most
256 KiB (three tiles and a partial one); a CPU assertion proves that it has the property its test is named for before the GPU
sees it.  A text is checked against the input (round trip) and against the oracle's streams of each block (util.block_reference,
util.exc_rice_reference) -- never against another run of the library: a missed or invented mark shows in the exception
streams, a wrong line offset everywhere.

Bytes that test the exactness of the per-dword tests (SWAR_BYTES), placed next to line ends in headers, are the ones the
commit before this file accepted there: 0x00 0x09 0x0b 0x2a 0x2c 0x3f 0x41 0x80 0x8a 0xab 0xc0 0xff."""
import numpy as np
import pytest

import util
from slimfastq_amd import capi

pytestmark = pytest.mark.gpu
SUB, TILE = 16384, 65536
SIZE = 3 * TILE + 2 * SUB + 5000                          # three tiles and a partial one, under 256 KiB
BORDERS = [b for b in range(SUB, SIZE, SUB)]
SWAR_BYTES = (0x00, 0x09, 0x0b, 0x2a, 0x2c, 0x3f, 0x41, 0x80, 0x8a, 0xab, 0xc0, 0xff)
SIDE_FROZEN = ("gen.Ns", "gen.Nn", "gen.lc", "usr.x", "usr.x.q")


# ---- texts -----------------------------------------------------------------------------------------------------------------
def _hdr(i, n, fill=b"x"):
    """n header bytes behind the '@'"""
    return (b"r%d." % i + fill * n)[:n]


class Builder:
    """Records one after another; place(T, line) puts the start of line `line` (1 bases, 2 '+', 3 qualities, 4 the NEXT
    record's header) of a record exactly at offset T by the length of that record's header."""

    def __init__(self, seed, blen=(1, 60), hlen=(1, 30), bases=None, quals=None, hdr_of=None):
        self.rng = np.random.default_rng(seed)
        self.blen, self.hlen = blen, hlen
        self.bases = bases or (lambda rng, n: bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8)))
        self.quals = quals or (lambda rng, n: bytes(rng.integers(35, 74, n).astype(np.uint8)))
        self.hdr_of = hdr_of or _hdr                       # (record number, length) -> the header behind its '@'
        self.out, self.p, self.i = [], 0, 0

    def rec(self, hl, b, hdr=None):
        h = hdr if hdr is not None else self.hdr_of(self.i, hl)
        r = b"@" + h + b"\n" + self.bases(self.rng, b) + b"\n+\n" + self.quals(self.rng, b) + b"\n"
        self.out.append(r); self.p += len(r); self.i += 1
        return r

    def any(self):
        return self.rec(int(self.rng.integers(self.hlen[0], self.hlen[1] + 1)), int(self.rng.integers(self.blen[0], self.blen[1] + 1)))

    def place(self, T, line, b=10):
        while T - self.p > 400:
            self.any()
        gap = T - self.p
        hl = {1: gap - 2, 2: gap - 3 - b, 3: gap - 5 - b, 4: gap - 6 - 2 * b}[line]
        assert 1 <= hl <= 400, (T, line, gap)
        self.rec(hl, b)

    def fill(self, size):
        while self.p < size:
            self.any()
        return b"".join(self.out)


def _lines(fq):
    """(starts, ends) of every line; a line's type is its index mod 4"""
    starts, lens = util.line_table(fq)
    return starts.astype(np.int64), starts.astype(np.int64) + lens


def _border_targets(lines=(1, 2, 3, 4)):
    """a line start on every sub-tile / tile border, on the byte before and the byte after, the line types in turn"""
    t = []
    for k, B in enumerate(BORDERS):
        t.append((B + (k % 3) - 1, lines[(k // 3) % len(lines)]))
    return t


def _code_and_check(ctx, fq, what, br=300):
    """the text through both table modes: the round trip, and every block's streams against the oracle's"""
    chunks = util.split_records(fq, br)
    enc = ctx.encode_host(fq, level=3, block_reads=br)                                        # adaptive tables, cold blocks
    assert enc.res.n_blocks == len(chunks), what
    for b, chunk in enumerate(chunks):
        want = util.block_reference(chunk, 3, gen_bits=enc.blocks[b].gen_bits).streams
        for name in capi.STREAM_NAMES:
            util.first_difference(enc.stream(name, b), want.get(name, b""), "%s: adaptive, block %d, %s" % (what, b, name))
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq, what
    enc = ctx.encode_host(fq, level=3, block_reads=br, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN, chain_reads=40)
    for b, chunk in enumerate(chunks):
        want = dict(util.block_reference(chunk, 3, gen_bits=enc.blocks[b].gen_bits).streams)
        want.update(util.exc_rice_reference(chunk))
        for name in SIDE_FROZEN:
            util.first_difference(enc.stream(name, b), want.get(name, b""), "%s: frozen, block %d, %s" % (what, b, name))
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq, what


def _refused(ctx, bad, what, both=True):
    for kw in (dict(block_reads=300, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN), dict(block_reads=300))[:2 if both else 1]:
        with pytest.raises(capi.SfqError) as e:
            ctx.encode_host(bytes(bad), level=3, **kw)
        assert e.value.code == -4, (what, e.value)


# ---- line ends -------------------------------------------------------------------------------------------------------------
def test_line_ends_on_every_residue_and_line_starts_on_every_border(ctx):
    bld = Builder(1)
    targets = _border_targets()
    for T, line in targets:
        bld.place(T, line)
    fq = bld.fill(SIZE)
    assert len(fq) <= 256 * 1024
    starts, ends = _lines(fq)
    assert set(ends % 64) == set(range(64))
    sset = set(starts.tolist())
    for T, line in targets:
        assert T in sset and int(np.searchsorted(starts, T)) % 4 == line % 4
    for B in (TILE, 2 * TILE, 3 * TILE):
        assert {B - 1, B, B + 1} & sset
    assert {d for B in BORDERS for d in (-1, 0, 1) if B + d in sset} == {-1, 0, 1}
    _code_and_check(ctx, fq, "line ends everywhere")


def test_several_line_ends_in_one_piece(ctx):
    """headers of 2 bytes, base and quality lines of 1..20, a bare '+': up to five line ends in a 16-byte piece; the '\\n+\\n'
    group at every byte of a dword and of a window, and across a piece, a window and a sub-tile border"""
    bld = Builder(2, blen=(1, 20), hlen=(1, 1))

    def steer(T):                                          # the '+' of a record at T: line 2 starts 4 + b behind the record's start
        while True:
            gap = T - bld.p
            if 5 <= gap <= 24:
                bld.rec(1, gap - 4, hdr=b"a")
                return
            if gap > 71:
                bld.rec(1, int(bld.rng.integers(1, 21)), hdr=b"a")
                continue
            L = next(L for L in range(9, 48, 2) if 5 <= gap - L <= 24)      # a record of 7 + 2 b bytes that leaves a gap in reach
            bld.rec(1, (L - 7) // 2, hdr=b"a")
    plus_at = [B + d for k, B in enumerate(BORDERS) for d in ((k % 3) - 1,)]
    for T in plus_at:
        steer(T)
    while bld.p < SIZE:
        bld.rec(1, int(bld.rng.integers(1, 21)), hdr=b"a")
    fq = b"".join(bld.out)
    assert len(fq) <= 256 * 1024
    a = np.frombuffer(fq, np.uint8)
    starts, ends = _lines(fq)
    plus = starts[2::4]
    assert all(fq[p - 1:p + 2] == b"\n+\n" for p in plus.tolist())
    assert set(plus % 64) == set(range(64))                # the group at every byte of a dword, a piece, a window
    assert set(plus_at) <= set(plus.tolist())              # ... and across the sub-tile and tile borders: '\n' | '+', '+' | '\n', '\n+\n' |
    per_piece = np.bincount(np.flatnonzero(a == 10) // 16)
    assert per_piece.max() >= 4 and (per_piece >= 2).sum() > 1000
    _code_and_check(ctx, fq, "several line ends in a piece", br=1500)


# ---- prefixes --------------------------------------------------------------------------------------------------------------
def _prefix_text():
    bld = Builder(3, blen=(5, 60))
    targets = _border_targets(lines=(4, 2))                # headers and '+' lines on the borders, the byte before, the byte after
    for T, line in targets:
        bld.place(T, line)
    return bld.fill(SIZE), targets


WRONG = {0: (b"+", b"X", b"\xc0", b"\xab", b"\x0b"), 2: (b"@", b"X", b"\xab", b"\xc0", b"\x0b")}


def test_wrong_prefixes_are_refused_wherever_a_line_starts(ctx):
    """a wrong byte -- the other prefix, 'X', either prefix with bit 7 set, 0x0b -- in place of a header's '@' and of a '+' line's
    '+': on every residue mod 16, on the first, second and last byte of a window, of a sub-tile and of a tile; an empty header
    or '+' line followed by a line that starts with the other prefix.  Every one is refused with SFQ_E_FORMAT (-4)"""
    fq, targets = _prefix_text()
    starts, _ = _lines(fq)
    _code_and_check(ctx, fq, "the untouched text")
    places = []                                            # (offset, line type)
    for t in (0, 2):
        s = starts[t::4]
        for r in range(16):                                # every residue mod 16 ...
            hit = s[s % 16 == r]
            assert len(hit), (t, r)
            places.append((int(hit[len(hit) // 2]), t))
        for r in (0, 1, 63):                               # ... the first, second and last byte of a window ...
            hit = s[(s % 64 == r) & (s % SUB > 64) & (s % SUB < SUB - 64)]
            assert len(hit), (t, r)
            places.append((int(hit[0]), t))
    for T, line in targets:                                # ... of a sub-tile and of a tile
        places.append((T, line % 4))
    on = {(T % SUB if T % SUB < 2 else T % SUB - SUB, t, T % TILE in (0, 1, TILE - 1)) for T, t in places[-len(targets):]}
    assert {(d, t) for d, t, _ in on} == {(d, t) for d in (-1, 0, 1) for t in (0, 2)}
    assert {d for d, _, tile in on if tile} == {-1, 0, 1}
    border = {(T, line % 4) for T, line in targets}
    for off, t in places:
        assert fq[off:off + 1] == (b"@" if t == 0 else b"+") and fq[off - 1:off] in (b"", b"\n")
        for w in WRONG[t]:
            bad = bytearray(fq); bad[off:off + 1] = w
            _refused(ctx, bad, (off, t, w), both=(off, t) in border and w == b"X")
    # an empty header line followed by a line that starts with the other prefix
    recs = util.split_records(fq, 1)
    j = len(recs) // 2
    bad = b"".join(recs[:j]) + b"\n+ACGT\n+\nIIIII\n" + b"".join(recs[j + 1:])
    _refused(ctx, bad, "empty header, then '+'")
    bad = b"".join(recs[:j]) + b"@h\nACGT\n\n@III\n" + b"".join(recs[j + 1:])
    _refused(ctx, bad, "empty '+' line, then '@'")


def test_prefix_bytes_where_no_prefix_is_due_change_nothing(ctx):
    """'@' and '+' as the first and last byte of quality lines -- right behind the line end of a '+' line, right before a
    header's '@' -- and as the second byte of headers.  (A base line that starts with '@' or '+' is not among the cases: what
    the base coders make of such a base is not the framing's business.)"""
    def quals(rng, n):
        q = bytearray(rng.integers(35, 74, n).astype(np.uint8))
        q[0] = b"@+"[int(rng.integers(2))]; q[-1] = b"+@"[int(rng.integers(2))]
        return bytes(q)
    bld = Builder(4, blen=(2, 60), quals=quals, hdr_of=lambda i, n: ((b"@", b"+", b"r")[i % 3] + _hdr(i, n))[:n])
    for T, line in _border_targets(lines=(3, 4, 1)):       # quality lines start, end (the next header starts) and bases start at the borders
        bld.place(T, line)
    fq = bld.fill(SIZE)
    starts, ends = _lines(fq)
    q0, q1, h1 = starts[3::4], ends[3::4] - 1, starts[0::4] + 1
    for pos in (q0, q1):
        assert all(fq[p] in b"@+" for p in pos.tolist())
        assert {(int(p) % 64, fq[p]) for p in pos.tolist()} == {(r, c) for r in range(64) for c in b"@+"}
    assert {(int(p) % 16, fq[p]) for p in h1.tolist() if fq[p] in b"@+"} == {(r, c) for r in range(16) for c in b"@+"}
    _code_and_check(ctx, fq, "prefix bytes where none is due")


# ---- marks -----------------------------------------------------------------------------------------------------------------
def test_marks_on_every_residue(ctx):
    """N . lowercase bases and '!' qualities at every residue mod 64, as the first and last byte of their line, of a window, of
    a sub-tile and of a tile; the same bytes in headers and in quality lines ('N', '.', 'a' are qualities 45, 13, 64), and
    '!' in headers, where they are no exception"""
    br = 300                                               # (a block holds 'N' and 'n' or '.', never both: the reference has one N byte a file)
    sets = (b"Nacgtn", b".acgt")

    def bases(rng, n):
        odd = sets[(bld.i // br) % 2]
        b = rng.choice(list(b"ACGT"), n).astype(np.uint8)
        m = (rng.random(n) < 0.08) | (n == 10)             # (the placed records, 10 bases long: marks alone)
        b[m] = rng.choice(list(odd), int(m.sum()))
        if rng.random() < 0.5: b[0] = odd[int(rng.integers(len(odd)))]
        if rng.random() < 0.5: b[-1] = odd[int(rng.integers(len(odd)))]
        return bytes(b)

    def quals(rng, n):
        q = rng.integers(35, 74, n).astype(np.uint8)
        q[(rng.random(n) < 0.08) | (n == 10)] = ord("!")
        m = (rng.random(n) < 0.08) & (n != 10)
        q[m] = rng.choice(list(b"N.a"), int(m.sum()))
        if rng.random() < 0.5: q[0] = ord("!")
        if rng.random() < 0.5: q[-1] = ord("!")
        return bytes(q)
    def hdr_of(i, n):                                      # (at most 64 bytes of a header may be neither letters nor digits)
        h = bytearray(_hdr(i, n, fill=b"Nagt"[i % 4:i % 4 + 1]))
        for k in range(3, min(n, 60), 3):
            h[k] = b".!"[(i + k) % 2]
        return bytes(h)
    bld = Builder(5, blen=(1, 40), bases=bases, quals=quals, hdr_of=hdr_of)
    # lines of marks alone across and on the borders: marks on the last byte before and the first byte behind them
    for T, line in ((SUB - 5, 1), (2 * SUB - 5, 3), (3 * SUB, 1), (TILE - 5, 1), (5 * SUB, 3), (6 * SUB + 1, 2), (7 * SUB + 1, 4), (2 * TILE - 5, 3),
                    (9 * SUB - 1, 1), (10 * SUB - 1, 3), (3 * TILE - 5, 1), (13 * SUB - 5, 3)):
        bld.place(T, line)
    fq = bld.fill(SIZE)
    assert len(fq) <= 256 * 1024
    a = np.frombuffer(fq, np.uint8)
    starts, ends = _lines(fq)
    typ = np.zeros(len(fq), np.int8)                       # the line type of every byte
    for t in range(4):
        for s, e in zip(starts[t::4].tolist(), ends[t::4].tolist()):
            typ[s:e + 1] = t
    is_odd = np.isin(a, list(b"N.acgtn")) & (typ == 1)
    for cls in (b"N", b".", b"acgtn"):
        assert set(np.flatnonzero(np.isin(a, list(cls)) & (typ == 1)) % 64) == set(range(64)), cls
    is_bang = (a == ord("!")) & (typ == 3)
    first, last = np.zeros(len(fq), bool), np.zeros(len(fq), bool)
    first[starts] = True; last[ends - 1] = True
    for m, t in ((is_odd, 1), (is_bang, 3)):
        pos = np.flatnonzero(m)
        assert set(pos % 64) == set(range(64))
        assert set(np.flatnonzero(m & first) % 64) == set(range(64)) and set(np.flatnonzero(m & last) % 64) == set(range(64))
        assert {0, SUB - 1} <= set((pos % SUB).tolist()) and {0, TILE - 1} <= set((pos % TILE).tolist())
    for t in (0, 3):                                       # the same bytes where they are no exception
        assert np.isin(a[typ == t], list(b"N.a")).sum() > 500
    assert (a[typ == 0] == ord("!")).sum() > 500
    _code_and_check(ctx, fq, "marks everywhere")


# ---- exactness of the per-dword tests --------------------------------------------------------------------------------------
def test_bytes_next_to_line_ends_that_test_the_dword_tests(ctx):
    """bytes one bit from a line end, from '@', from '+', and bytes of 0x80 and more -- as a header's first and last byte, so
    that they lie right behind the '@' and right before a line end, at every place of a dword"""
    bld = Builder(6, blen=(1, 40))
    while bld.p < 40000:
        hl = int(bld.rng.integers(2, 12))
        c = bytes([SWAR_BYTES[bld.i % len(SWAR_BYTES)]]); d = bytes([SWAR_BYTES[(bld.i // 3) % len(SWAR_BYTES)]])
        bld.rec(hl, int(bld.rng.integers(1, 41)), hdr=c + _hdr(bld.i, hl - 2) + d)
    fq = b"".join(bld.out)
    starts, ends = _lines(fq)
    assert {(fq[e - 1], int(e) % 4) for e in ends[0::4].tolist()} == {(c, r) for c in SWAR_BYTES for r in range(4)}
    assert {(fq[s + 1], int(s + 1) % 4) for s in starts[0::4].tolist()} == {(c, r) for c in SWAR_BYTES for r in range(4)}
    _code_and_check(ctx, fq, "bytes that test the dword tests")


# ---- the text's end --------------------------------------------------------------------------------------------------------
def test_the_texts_end_at_every_length_of_the_last_piece(ctx):
    """the last piece of the text 1 .. 16 bytes long, in a tile's second sub-tile; without its final line end the text is
    refused (no final newline: the reference's 'record seems truncated')"""
    bld = Builder(7, blen=(1, 40))
    body = bld.fill(TILE + SUB + 3000)
    seen = set()
    for r in range(16):
        b = 12
        hl = (r - (len(body) + 6 + 2 * b)) % 16 + 16
        fq = body + b"@" + _hdr(9, hl) + b"\n" + b"ACGTNACGTACG" + b"\n+\n" + b"IIII!IIIIII!" + b"\n"
        assert len(fq) % 16 == r
        seen.add(len(fq) % 16)
        _code_and_check(ctx, fq, "text of %d bytes" % len(fq), br=2000)
        with pytest.raises(capi.SfqError) as e:
            ctx.encode_host(fq[:-1], level=3, block_reads=300, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN)
        assert e.value.code == -4, r
    assert seen == set(range(16))

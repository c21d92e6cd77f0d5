"""CPU: what test_large_texts.py relies on (large_text.py), at k = 3 on whole host texts and by arithmetic at the k of the 4 GiB texts:
the pieces hold whole records and whole pairs; the builder's offsets, record numbers and the record, line and byte at the mark are
right in each of the four placements; odd tiles give every phase of a 16-byte unit within 16 copies; every Python rule the GPU cases
use gives f(head) + f(tile) * 2 + f(tail) on head + tile + tile + tail, its report the sum; the chunked comparison finds a planted
difference on either side of every chunk border and names it; crc32_tiled is zlib.crc32 of the text."""
import zlib

import numpy as np
import pytest

import large_text as LT
from large_text import MARK, NumpyOps, Tiled
from test_overlap import overlapped
from test_pairs import ILLUMINA8, interleaved, numpy_mapped, records, split
from test_pick import ALL, picked
from test_select import keep, selected
from test_text_stats import ref_stats
from test_trim import trimmed

LC = LT
TEXTS_PLACE = {n: v[2] for n, v in LT.TEXTS.items()}


def small(t, k=3):
    return Tiled(t.head, t.tile, k, t.tail)


# ---- the pieces ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LC.TEXTS))
def test_pieces_hold_whole_records_and_whole_pairs(name):
    t = LC.text(name)
    paired = LC.TEXTS[name][1]
    for piece in t.pieces:
        if not piece:
            continue
        rs = records(piece)                                             # (asserts a multiple of four lines)
        assert piece.endswith(b"\n") and b"".join(rs) == piece and len(piece) <= (1 << 20) + 4096
        for r in rs:
            l = r.split(b"\n")
            assert len(l) == 5 and l[0][:1] == b"@" and l[2] == b"+" and l[4] == b"" and b"\r" not in r
        if paired:
            assert len(rs) % 2 == 0
    assert t.T % 2 == 1 and len(t.rh) == (2 if paired else 1 if t.head else 0)
    if name == "B":
        assert t.nbytes < 1 << 29 and t.k == LC.text("A").k
    else:                                                               # the text reaches over the mark, two tiles or more behind it
        assert MARK + 2 * t.T <= t.nbytes
        assert TEXTS_PLACE[name] is None or t.nbytes < MARK + 3 * t.T + t.L + 1    # ... and not a tile more than that
    assert t.nbytes == t.H + t.k * t.T + t.L and t.nrec == len(t.rh) + t.k * len(t.rt) + len(t.rl)


def test_the_tile_of_pairs_gives_every_pass_something_to_do():
    tile = LC.text("S:base").tile
    lens = [len(r.split(b"\n")[1]) for r in records(tile)]
    assert min(lens) == 1 and max(lens) >= 155 and len(set(lens)) > 80
    b = b"".join(r.split(b"\n")[1] for r in records(tile))
    q = b"".join(r.split(b"\n")[3] for r in records(tile))
    assert b.count(b"N") and b.count(b"n") and sum(b.count(c) for c in (b"a", b"c", b"g", b"t")) and q.count(b"!")
    heads = [r.split(b"\n")[0] for r in records(tile)]
    assert all(x.split()[0][-2:] == b"/1" and y.split()[0][-2:] == b"/2" and x.split()[0][:-2] == y.split()[0][:-2] for x, y in zip(heads[0::2], heads[1::2]))
    _, rep = trimmed(tile, LC.TRIM)
    assert 0 < rep[2] < rep[0] // 4 and rep[6] > rep[5] // 2 and all(x > 10 for x in rep[7]), rep       # emptied, bases kept, every one of the four cuts
    _, rep, wins = overlapped(tile, LC.OVERLAP)
    assert rep[2] > 20 and rep[3] > 10 and wins.count(None) > 20 and rep[8] > 0    # overlaps, cuts, pairs apart, mismatches
    kept, nfail, n = selected(tile, LC.SELECT)
    assert 0 < len(kept) < n and all(nfail), (len(kept), nfail)
    assert numpy_mapped(tile, ILLUMINA8) != tile


# ---- the builder's tables ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("place", LT.PLACES)
def test_offsets_records_and_the_mark_at_k_3(place):
    """a small mark instead of 2^32: the whole text exists, and every table is compared with a walk over it"""
    big = LC.text("S:base")
    mark = 5 * big.T + 12345
    t = LT.placed(big.tile, big.tail, place, mark=mark, spare=2)
    fq = t.text()
    assert len(fq) == t.nbytes and mark + 2 * t.T <= t.nbytes
    rs = records(fq)
    starts = np.cumsum([0] + [len(r) for r in rs])
    assert len(rs) == t.nrec
    off, first = t.tables()
    assert off[0] == 0 and off[1] == t.H and off[-2] == t.nbytes - t.L and off[-1] == len(fq)
    for o, f in zip(off, first):
        assert starts[f] == o                                           # piece i begins at record first[i], at byte off[i]
    for r in (0, 1, 2, 3, len(t.rh) + len(t.rt) - 1, len(t.rh) + len(t.rt), t.nrec - len(t.rl) - 1, t.nrec - len(t.rl), t.nrec - 1, t.nrec):
        assert t.record_off(r) == starts[r]
        if r < t.nrec:
            assert t.record(r) == rs[r]
    assert t.records(len(t.rh) + len(t.rt) - 3, 7) == b"".join(rs[len(t.rh) + len(t.rt) - 3:][:7])
    assert t.records(t.nrec - 5, 5) == b"".join(rs[-5:])
    # the mark: found by a walk over the text
    r = int(np.searchsorted(starts, mark, side="right")) - 1
    o = mark - int(starts[r])
    lines = rs[r].split(b"\n")
    line = 0
    while o > len(lines[line]):
        o -= len(lines[line]) + 1
        line += 1
    assert t.locate(mark) == (r, line + 1, o, len(lines[line]) + 1)
    check_place(place, fq[mark:mark + 1], t.locate(mark))


def check_place(place, byte, where):
    r, line, o, n = where
    if place == "base":
        assert line == 2 and 0 < o < n - 2 and byte.upper() in (b"A", b"C", b"G", b"T", b"N")
    elif place == "qual":
        assert line == 4 and 0 < o < n - 2
    elif place == "first":
        assert (line, o, byte) == (1, 0, b"@")
    else:
        assert line == 2 and o == n - 1 and byte == b"\n"


@pytest.mark.parametrize("name", sorted(LC.TEXTS))
def test_the_mark_of_the_large_texts_by_arithmetic(name):
    t = LC.text(name)
    place = LC.TEXTS[name][2]
    if place is None:
        return
    r, line, o, n = where = t.mark()
    # the same byte from the pieces: the record's offset, then the lines in front of it
    rec = t.record(r)
    at = t.record_off(r) + sum(len(l) + 1 for l in rec.split(b"\n")[:line - 1]) + o
    assert at == MARK and t.record_off(r) <= MARK < t.record_off(r + 1)
    check_place(place, rec[MARK - t.record_off(r):][:1], where)
    c = (MARK - t.H) // t.T
    assert t.copy_first(c) <= r < t.copy_first(c + 1) and 16 <= c <= t.k - 2
    assert len(t.head.split(b"\n")[0]) < 600                             # the pad is a header, not a text


@pytest.mark.parametrize("name", sorted(LC.TEXTS))
def test_copies_fall_on_every_phase(name):
    t = LC.text(name)
    assert {t.copy_off(c) % 16 for c in range(16)} == set(range(16))
    assert len({t.copy_off(c) % 1024 for c in range(1024)}) == 1024
    c = (MARK - t.H) // t.T                                             # and behind the mark as in front of it
    assert name == "B" or (len({t.copy_off(x) % 16 for x in range(c - 13, c + 3)}) == 16 and c + 3 <= t.k)


# ---- the rules are record-local on these pieces --------------------------------------------------------------------------------------

def test_every_rule_is_local_to_the_pieces():
    t = small(LC.text("S:base"), 2)
    fq = t.text()
    h, m, l = t.pieces

    def tiled(f):
        return f(h) + f(m) * 2 + f(l)
    for f in (trimmed, overlapped):
        for rule in ((LC.TRIM,) if f is trimmed else (LC.OVERLAP, LC.OVERLAP_COUNT)):
            whole, parts = f(fq, rule), [f(p, rule) for p in (h, m, l)]
            assert whole[0] == parts[0][0] + parts[1][0] * 2 + parts[2][0]
            assert whole[1] == LT.summed(parts[0][1], parts[1][1], 2, parts[2][1])
    assert overlapped(fq, LC.OVERLAP_COUNT)[0] == fq
    for what in ALL:
        assert picked(fq, what) == tiled(lambda p: picked(p, what))
    assert keep(fq, LC.SELECT) == tiled(lambda p: keep(p, LC.SELECT))
    whole, parts = selected(fq, LC.SELECT), [selected(p, LC.SELECT) for p in (h, m, l)]
    assert whole[1] == LT.summed(parts[0][1], parts[1][1], 2, parts[2][1]) and whole[2] == parts[0][2] + 2 * parts[1][2] + parts[2][2]
    assert numpy_mapped(fq, ILLUMINA8) == tiled(lambda p: numpy_mapped(p, ILLUMINA8))
    # the split: the even records of every piece, then the odd ones
    ev, od = (lambda p: b"".join(records(p)[0::2])), (lambda p: b"".join(records(p)[1::2]))
    assert split(fq) == tiled(ev) + tiled(od)
    # the interleave of two texts that are tiles alone
    a, b = LC.text("A"), LC.text("B")
    assert (a.H, a.L, b.H, b.L) == (0, 0, 0, 0) and a.k == b.k and len(a.rt) == len(b.rt)
    assert interleaved(a.tile * 2, b.tile * 2) == interleaved(a.tile, b.tile) * 2
    assert a.nbytes > MARK and b.nbytes < 1 << 29
    # statistics: sums add up, the range is the pieces'
    st = [ref_stats(p) for p in (h, m, l)]
    whole = ref_stats(fq)
    assert whole.n_records == st[0].n_records + 2 * st[1].n_records + st[2].n_records
    assert whole.seq_len_min == min(s.seq_len_min for s in st) and whole.seq_len_max == max(s.seq_len_max for s in st)
    assert list(whole.qlt_hist) == [x + 2 * y + z for x, y, z in zip(st[0].qlt_hist, st[1].qlt_hist, st[2].qlt_hist)]


# ---- the comparison's host twin ------------------------------------------------------------------------------------------------------

def test_chunk_plan_covers_the_result_once():
    for lens, k, chunk in (((5, 7, 3), 10, 21), ((0, 7, 0), 10, 7), ((5, 7, 3), 1, 100), ((5, 0, 3), 4, 8), ((1, 1, 1), 9, 4), ((9, 11, 0), 13, 1)):
        plan = LT.chunk_plan(lens, k, chunk)
        at, copies = 0, 0
        for off, piece, c0, n in plan:
            assert off == at and (piece != 1 or c0 == copies)
            assert piece == 1 or n == 1
            at += lens[piece] * n
            copies += n if piece == 1 else 0
            assert piece != 1 or n * lens[1] <= max(chunk, lens[1])
        assert at == lens[0] + k * lens[1] + lens[2] and copies == (k if lens[1] else 0)


def test_the_comparison_finds_a_planted_difference_on_either_side_of_a_chunk_border():
    rng = np.random.default_rng(1)
    pieces = tuple(rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (37, 101, 23))
    k, chunk = 11, 303                                                  # three copies a chunk: chunks of 3, 3, 3 and 2 copies
    good = np.frombuffer(pieces[0] + pieces[1] * k + pieces[2], np.uint8)
    slack = np.concatenate([good, np.full(9, 73, np.uint8)])
    assert LT.equal_tiled(slack, pieces, k, "good", NumpyOps, chunk) == len(good)
    borders = [off for off, _, _, _ in LT.chunk_plan([len(p) for p in pieces], k, chunk)] + [len(good)]
    assert borders == [0, 37, 37 + 303, 37 + 606, 37 + 909, 37 + 11 * 101, len(good)]
    for b in borders:
        for at in (b - 1, b):
            if not 0 <= at < len(good):
                continue
            bad = slack.copy()
            bad[at] ^= 0x10
            if at + 40 < len(good):
                bad[at + 40] ^= 1                                           # a later difference is not the one reported
            with pytest.raises(AssertionError) as e:
                LT.equal_tiled(bad, pieces, k, "planted", NumpyOps, chunk)
            msg = str(e.value)
            assert "is at %d (0x%x) of %d" % (at, at, len(good)) in msg, msg
            if 37 <= at < 37 + k * 101:
                assert "copy %d of the tile, offset %d inside it" % ((at - 37) // 101, (at - 37) % 101) in msg, msg
            else:
                assert "inside the %s" % ("head" if at < 37 else "tail") in msg, msg
            assert "got %r, want %r" % (bad[at:at + 32].tobytes()[:len(good) - at], good[at:at + 32].tobytes()) in msg, msg
    with pytest.raises(AssertionError):
        LT.equal_tiled(good[:-1], pieces, k, "short", NumpyOps, chunk)
    # the variant for host bytes
    LT.equal_bytes(good, 40, good[40:90].tobytes(), "window", NumpyOps)
    bad = good.copy(); bad[77] ^= 4
    with pytest.raises(AssertionError) as e:
        LT.equal_bytes(bad, 40, good[40:90].tobytes(), "window", NumpyOps)
    assert "is at 77 (0x4d), 37 of 50" in str(e.value)


def test_expected_bytes_is_a_slice_of_the_text():
    p = (b"abc", b"defgh", b"ij")
    fq = p[0] + p[1] * 3 + p[2]
    assert all(LT.expected_bytes(p, 3, a, b) == fq[a:b] for a in range(len(fq)) for b in range(a, len(fq) + 1))
    assert LT.expected_bytes((b"", b"xyz", b""), 1 << 40, (1 << 41) + 1, (1 << 41) + 6) == b"xyzxy"


def test_offsets_are_named_as_64_bit_numbers():
    """the arithmetic of the message at the real sizes: python's integers, no array index of 32 bits in between"""
    t = LC.text("S:base")
    plan = LT.chunk_plan((t.H, t.T, t.L), t.k, LT.CHUNK)
    assert plan[-1][0] == t.H + t.k * t.T > MARK and plan[-1][0] + t.L == t.nbytes
    assert sum(n for _, p, _, n in plan if p == 1) == t.k and len(plan) < 100


# ---- CRC -------------------------------------------------------------------------------------------------------------------------------

def test_crc32_tiled_is_zlibs_of_the_text():
    t = small(LC.text("S:base"), 3)
    fq = t.text()
    stops = [0, 1, t.H, t.H + 5, t.H + t.T, t.H + 2 * t.T + 77, len(fq) - 1, len(fq)]
    whole, parts = LT.crc32_tiled(t.pieces, 3, stops)
    assert whole == zlib.crc32(fq) and parts == [zlib.crc32(fq[:s]) for s in stops]


# ---- the texts of the coding cases -------------------------------------------------------------------------------------------------------

def test_the_unpaired_text_repeats_its_blocks():
    t = LC.text("U")
    br = LC.U_BLOCK_READS
    assert len(t.rt) % br == 0 and len(t.rh) == 1 and len(t.rl) > 0
    # a block of the copies behind the first begins one record into a tile's block: blocks are not the tile's, records repeat all the same
    per = len(t.rt) // br
    first = [b * br for b in range(3 * per)]
    assert t.records(first[1], br) == t.records(first[1 + per], br) != t.records(first[2], br)


def test_the_genome_like_text_stages_4_gib_of_bases():
    t = LC.text("L")
    stage = sum(len(r.split(b"\n")[1]) + 1 for r in t.rh) + t.k * sum(len(r.split(b"\n")[1]) + 1 for r in t.rt) + \
        sum(len(r.split(b"\n")[1]) + 1 for r in t.rl)
    assert stage >= MARK and t.nbytes < int(4.45 * (1 << 30))
    assert all(len(r.split(b"\n")[3]) <= 4 for r in t.rt)
    # the oracle's verdict on three copies: the match model pays on records like these (at 4 GiB the oracle would take minutes)
    import util
    from oracle import oracle as O
    from test_frozen_tables import gm_chain_reads, gm_table_bits
    fq = small(t).text()
    starts, lens = util.line_table(fq)
    gcr = gm_chain_reads(len(fq), len(starts) // 4, LC.L_BLOCK_READS, LC.L_CHAIN_READS)
    coded, _, on = O.gm_encode_chains(fq, starts[1::4], lens[1::4], gm_table_bits(len(fq)), LC.L_BLOCK_READS, gcr)
    assert on == 1 and len(coded) * 8 < int(lens[1::4].sum())            # under a bit a base

"""GPU: every device entry on texts that cross the 4 GiB offset (large_text.py builds them; test_large_text_inputs.py holds the builder,
the rules' locality and the comparison to their word on the CPU).  Every byte the suite handed a kernel before lay below offset 2^32;
here the text is 2^32 bytes and two tiles or more, byte 2^32 -- the mark -- inside a base line (S:base) or a quality line (S:qual).
Every comparison is exact byte equality against the Python rules of test_trim / test_pick / test_select / test_overlap / test_pairs and
zlib; whole-text results against f(head) + f(tile) * k + f(tail) on the device, windows against the rule on just those records.  Only the
pieces, the windows' results and the 32-byte excerpts of a mismatch are on the host.

The texts (large_text.TEXTS): S -- interleaved pairs of 1 .. 160 bases, 4 295 255 416 bytes, 20.4 M records, a tile of 126 279 bytes 34 014
times; A and B -- the interleave's inputs, 4.3 GB of reads and as many reads of one base (228 MB); U -- exception-heavy single reads for
the coding entries, blocks of 128 records, the tile four blocks; L -- genome-like records of 5000 bases and three quality bytes, 4.31 GB,
whose staged bases reach 2^32.  torch's stream is not the context's: every text and every guarded output is synchronised before a call.

Still not reached: a reference for the match model at this size.  The oracle would take minutes on 4 GiB, so case (b) is a round trip alone
(encode, decode_device, a window of the last blocks): an error that the walk's u64 instantiation makes the same way in both directions
passes it.  Nothing was dropped for memory.  sfq_get_pick's mark_off belongs to the host decoders; sfq_pick_lines reports none.  No entry
showed a size limit that the header does not state.

Measured on one MI355X, this module alone, 28 cases in 25.9 s (--durations=0; the rest of the 25.9 s is the process's first use of torch,
the context and building the texts).  Wall time of a case; the peak of torch's allocations; the drop of free device memory over the case
(torch.cuda.mem_get_info: what the context and torch's cache took anew, negative where torch gave memory back):
    trim_records S:base / S:qual             0.39 / 0.97 s    6.7 GiB    16.8 / 0 GiB   (the context's first working buffers)
    pick_lines whole, each of four           0.01 s           4.3 - 6.2 GiB    0
    overlap_pairs cut S:base / S:qual        0.06 / 0.45 s    7.8 GiB    3.6 / -2.1 GiB
    overlap_pairs counted only               0.05 s           4.0 GiB    -3.8 GiB
    select_records whole                     0.02 s           4.3 GiB    0.3 GiB
    map_qualities, each of two               0.01 s           4.1 GiB    0
    split_pairs whole                        0.53 s           8.1 GiB    4.0 GiB
    pick_lines windows, each of six          0.01 s (one 0.70) 4.0 GiB   0
    split_pairs_range, select window         0.01 - 0.02 s    4.0 GiB    0
    overlap_pairs range                      0.02 s           8.1 GiB    4.1 GiB
    refusals                                 0.02 s           12.0 GiB   6.1 GiB
    crc32 around the mark / to the mark and whole   0.02 / 2.18 s (zlib over 4.3 GB on the host)   8.0 GiB   0
    interleave and check_mates               0.04 s           16.6 GiB   2.4 GiB
    (a) coding with a given prior            5.19 s           14.1 GiB   64.5 GiB  (sfq_encode_bound's output is torch's; some 50 GiB are the context's)
    (b) match model, a stage of 4 GiB        2.81 s           14.2 GiB   2.1 GiB
The whole GPU suite, same machine and run: 493.8 s with this module (1067 tests), 468 s without it (by subtraction).

Checked once on scratch copies of the kernels, one offset narrowed at a time so that it addresses a LOWER byte of the same buffer (no bound
touched); with each, the cases named fail and the modules named still pass:
    pick.hip piece():  *src = J.src + (u32)J.from[k]            all four pick_lines whole, all six windows (first at copy 34 011, the first
                                                                 copy behind the mark); test_pick, test_pick_cli, test_pairs pass
    dev_pieces.h as trim.hip includes it:  from[1] = (u64)(u32)a1 + s   (the base line's start)   trim_records S:base and S:qual (copy 34 011);
                                                                 test_trim, test_trim_decode, test_trim_cli, test_overlap pass
    crc.hip k_crc_ranges:  a = d + (u32)S                       both crc32 cases; test_checksums passes
  not run, from reading crc.hip: it changes no byte or it is a bound
    launch_crc32's own `lo` narrowed where the tiles' origin `o` is laid: the origin moves down by 2^32, a multiple of the 4 KiB tile, so
    k_crc_ranges finds no whole tile of the moved grid inside its range (ta > tb) and takes the range piece by piece: the same CRC, slower.
    Narrowed in crc_scratch_words as well, the tiles outgrow the scratch that sfq_crc32 sized from the true `lo`: that is a bound, not an offset.
    The range start is therefore narrowed where k_crc_ranges reads it.
"""
import time
import zlib

import pytest

import large_text as LT
from large_text import MARK, device_all, device_equal_bytes, device_equal_tiled
from slimfastq_amd import capi
from slimfastq_amd.capi import Overlap, Select
from test_overlap import fields as overlap_fields, overlapped
from test_pairs import ILLUMINA8, interleaved, numpy_mapped, records
from test_pick import ALL, NAME, picked
from test_select import keep, selected
from test_trim import fields as trim_fields, trimmed

pytestmark = pytest.mark.gpu
E_ARG, E_OVERFLOW = -1, -5
GUARD, SLACK = ord("I"), 64
BOTH = ("S:base", "S:qual")


# ---- the context, the text on the device, the measurements ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def big():
    """A context of this module's own: the session's stays as small as it is"""
    c = capi.Context(0)
    yield c
    held.clear()
    c.close()


held = {}                                                        # name -> the one text that is on the device


def device_text(name):
    """the text `name` on the device; a text that was there before is released first"""
    import torch
    if name not in held:
        held.clear()
        torch.cuda.empty_cache()
        held[name] = LT.text(name).device()
        torch.cuda.synchronize()                                 # torch's stream is not the context's: the text is whole before a call reads it
    return LT.text(name), held[name]


def guarded(n):
    """n bytes and SLACK more, every one the guard's, written before anything else runs"""
    import torch
    t = torch.full((n + SLACK,), GUARD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


@pytest.fixture(autouse=True)
def measured(request, big):
    """prints the case's time, the peak of torch's allocations and the drop in free device memory over the case (what the context took)"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    free0, t0 = torch.cuda.mem_get_info()[0], time.time()
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                    # a fault on the device: nothing more is started on it
        pytest.exit("the device failed in %s: %s" % (request.node.name, e), returncode=3)
    free1 = torch.cuda.mem_get_info()[0]
    print("\nMEASURED %s: %.2f s, torch peak %.2f GiB, free memory fell by %.2f GiB" % (
        request.node.name, time.time() - t0, torch.cuda.max_memory_allocated() / 2 ** 30, (free0 - free1) / 2 ** 30))


def tiled_result(out, n, parts, k, what):
    """the n bytes of a result are parts[0] + parts[1] * k + parts[2]; the bytes behind them are the guard's"""
    want = len(parts[0]) + k * len(parts[1]) + len(parts[2])
    assert n == want, "%s: %d bytes, %d are expected" % (what, n, want)
    device_equal_tiled(out, parts, k, what)
    assert device_all(out[n:], GUARD), what + ": bytes behind the result were written"


def text_untouched(name, what):
    t, d = device_text(name)
    device_equal_tiled(d, t.pieces, t.k, what + ": the text")


# ---- record-local passes over the whole text -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BOTH)
def test_trim_records(big, name):
    t, d = device_text(name)
    f = [trimmed(p, LT.TRIM) for p in t.pieces]
    out = guarded(f[0][1][4] + t.k * f[1][1][4] + f[2][1][4])
    n, rep = big.trim_records(d.data_ptr(), t.nbytes, LT.TRIM, out.data_ptr(), out.numel() - SLACK)
    assert trim_fields(rep) == LT.summed(f[0][1], f[1][1], t.k, f[2][1])
    tiled_result(out, n, [x[0] for x in f], t.k, "trim_records of " + name)
    del out
    text_untouched(name, "trim_records")


@pytest.mark.parametrize("what", ALL, ids=NAME.get)
def test_pick_lines_of_the_whole_text(big, what):
    t, d = device_text("S:base")
    f = [picked(p, what) for p in t.pieces]
    out = guarded(len(f[0]) + t.k * len(f[1]) + len(f[2]))
    n, recs = big.pick_lines(d.data_ptr(), t.nbytes, what, out.data_ptr(), out.numel() - SLACK)
    assert recs == t.nrec
    tiled_result(out, n, f, t.k, "pick_lines %s" % NAME[what])


@pytest.mark.parametrize("name", BOTH)
def test_overlap_pairs_cut(big, name):
    t, d = device_text(name)
    f = [overlapped(p, LT.OVERLAP) for p in t.pieces]
    out = guarded(sum(len(x[0]) * (t.k if i == 1 else 1) for i, x in enumerate(f)))
    n, rep = big.overlap_pairs(d.data_ptr(), t.nbytes, LT.OVERLAP, out.data_ptr(), out.numel() - SLACK)
    got, want = overlap_fields(rep), LT.summed(f[0][1], f[1][1], t.k, f[2][1])
    assert got[:9] == want[:9]
    assert got[9] == want[9], [(i, x, y) for i, (x, y) in enumerate(zip(got[9], want[9])) if x != y]
    tiled_result(out, n, [x[0] for x in f], t.k, "overlap_pairs of " + name)


def test_overlap_pairs_counted_only(big):
    """cut = 0: the counts and the histogram; the output is left alone"""
    t, d = device_text("S:base")
    f = [overlapped(p, LT.OVERLAP_COUNT) for p in t.pieces]
    out = guarded(4096)
    n, rep = big.overlap_pairs(d.data_ptr(), t.nbytes, LT.OVERLAP_COUNT, out.data_ptr(), 4096)
    assert n == t.nbytes
    assert overlap_fields(rep) == LT.summed(f[0][1], f[1][1], t.k, f[2][1])
    assert device_all(out, GUARD), "a call that does not cut wrote to its output"


def test_select_records_of_the_whole_text(big):
    t, d = device_text("S:base")
    f = [keep(p, LT.SELECT) for p in t.pieces]
    s = [selected(p, LT.SELECT) for p in t.pieces]
    out = guarded(len(f[0]) + t.k * len(f[1]) + len(f[2]))
    n, rep = big.select_records(d.data_ptr(), t.nbytes, LT.SELECT, out.data_ptr(), out.numel() - SLACK)
    assert (rep.n_in_range, rep.text_bytes, rep.kept_bytes) == (t.nrec, t.nbytes, n)
    assert rep.n_kept == len(s[0][0]) + t.k * len(s[1][0]) + len(s[2][0])
    assert list(rep.n_fail) == LT.summed(s[0][1], s[1][1], t.k, s[2][1])
    tiled_result(out, n, f, t.k, "select_records")


@pytest.mark.parametrize("name", BOTH)
def test_map_qualities_in_place(big, name):
    import numpy as np
    t, d = device_text(name)
    f = [numpy_mapped(p, ILLUMINA8) for p in t.pieces]
    diff = [int(np.count_nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))) for a, b in zip(f, t.pieces)]
    try:
        assert big.map_qualities(d.data_ptr(), t.nbytes, ILLUMINA8) == diff[0] + t.k * diff[1] + diff[2] > MARK // 8
        device_equal_tiled(d, f, t.k, "map_qualities of " + name)
    finally:
        held.clear()                                             # the text is no longer the text


def test_split_pairs_of_the_whole_text(big):
    t, d = device_text("S:base")
    ev = [b"".join(records(p)[0::2]) for p in t.pieces]
    od = [b"".join(records(p)[1::2]) for p in t.pieces]
    out = guarded(t.nbytes)
    at, pairs = big.split_pairs(d.data_ptr(), t.nbytes, out.data_ptr(), t.nbytes)
    assert (at, pairs) == (len(ev[0]) + t.k * len(ev[1]) + len(ev[2]), t.nrec // 2)
    device_equal_tiled(out[:at], ev, t.k, "split_pairs: the first mates")
    device_equal_tiled(out[at:t.nbytes], od, t.k, "split_pairs: the second mates, from byte %d on" % at)
    assert device_all(out[t.nbytes:], GUARD)


# ---- windows behind and across the mark ----------------------------------------------------------------------------------------------

def windows(t, m=50):
    """(first record, records): from the record that holds the mark, from the first record wholly behind it, the text's last m"""
    r = t.mark()[0]
    assert t.record_off(r) < MARK < t.record_off(r + 1) and t.record_off(r + 1) > MARK
    return (r, m), (r + 1, m), (t.nrec - m, m)


@pytest.mark.parametrize("name", BOTH)
@pytest.mark.parametrize("which", (0, 1, 2), ids=("straddling", "behind", "last"))
def test_pick_lines_of_a_window(big, name, which):
    """(sfq_get_pick's mark_off is the host decoders' own: the device entry reports bytes and records alone)"""
    t, d = device_text(name)
    first, m = windows(t)[which]
    fq = t.records(first, m)
    for what in ALL:
        want = picked(fq, what)
        out = guarded(len(want))
        n, recs = big.pick_lines(d.data_ptr(), t.nbytes, what, out.data_ptr(), len(want), first, m)
        assert (n, recs) == (len(want), m)
        device_equal_bytes(out, 0, want, "pick_lines %s of records %d..+%d" % (NAME[what], first, m))
        assert device_all(out[n:], GUARD)


def test_split_pairs_range_across_the_mark(big):
    t, d = device_text("S:base")
    for first in (t.mark()[0] - 21, t.mark()[0] - 20):            # a window that begins at a first mate, and at a second
        rs = records(t.records(first, 40))
        want = b"".join(rs[0::2]), b"".join(rs[1::2])
        out = guarded(len(want[0] + want[1]))
        at, n = big.split_pairs_range(d.data_ptr(), t.nbytes, first, 40, out.data_ptr(), out.numel() - SLACK)
        assert (at, n) == (len(want[0]), len(want[0] + want[1]))
        device_equal_bytes(out, 0, want[0] + want[1], "split_pairs_range of records %d..+40" % first)
        assert device_all(out[n:], GUARD)


def test_select_records_of_a_sampled_window_across_the_mark(big):
    """The sample hashes index_base + the record's number in the text: the case cannot be tiled"""
    t, d = device_text("S:base")
    first, m, base = t.mark()[0] - 151, 400, 7 * MARK + 12346
    for pairs in (0, capi.SELECT_BOTH):
        kw = dict(min_len=30, max_n=2, motif=b"GGAC", motif_rc=True, pairs=pairs, sample=3 << 30, sample_seed=99)
        first -= first % 2 if pairs else 0
        fq = t.records(first, m)
        s = Select(first_record=first, n_records=m, index_base=base, **kw)
        ref = Select(first_record=0, n_records=m, index_base=base + first, **kw)        # the rule on just those records
        kept, nfail, _ = selected(fq, ref)
        want = keep(fq, ref)
        assert 0 < len(kept) < m and any(nfail)
        out = guarded(len(want))
        n, rep = big.select_records(d.data_ptr(), t.nbytes, s, out.data_ptr(), len(want))
        assert (n, rep.n_in_range, rep.n_kept, rep.kept_bytes, list(rep.n_fail)) == (len(want), m, len(kept), len(want), nfail)
        device_equal_bytes(out, 0, want, "select_records of records %d..+%d, pairs %d" % (first, m, pairs))
        assert device_all(out[n:], GUARD)


def test_overlap_pairs_of_a_range_across_the_mark(big):
    """The result is the text with the range's pairs cut: the text in front of the range, the rule's result, the text behind it"""
    t, d = device_text("S:base")
    first, m = (t.mark()[0] - 60) & ~1, 120
    fq = t.records(first, m)
    want, rep_want, _ = overlapped(fq, Overlap(cut=1))
    lo, hi = t.record_off(first), t.record_off(first + m)
    assert lo < MARK < hi and len(want) < len(fq)
    total = t.nbytes - len(fq) + len(want)
    out = guarded(total)
    n, rep = big.overlap_pairs(d.data_ptr(), t.nbytes, Overlap(first_record=first, n_records=m, cut=1), out.data_ptr(), total)
    got = overlap_fields(rep)
    # (text_bytes and out_bytes are the whole text's; every other field is the range's)
    assert (n, got[4], got[5]) == (total, t.nbytes, total)
    assert got[:4] + got[6:] == rep_want[:4] + rep_want[6:]
    device_equal_bytes(out, lo, want, "overlap_pairs of records %d..+%d" % (first, m))
    c = (lo - t.H) // t.T                                         # in front of the range: the head, c whole copies, a part of one
    device_equal_tiled(out, (t.head, t.tile, t.tile[:lo - t.copy_off(c)]), c, "overlap_pairs: the text in front of the range")
    c2 = -(-(hi - t.H) // t.T)                                    # behind it: the rest of a copy as the head, the copies, the tail
    device_equal_tiled(out[lo + len(want):], (t.tile[hi - t.copy_off(c2 - 1):] if hi < t.copy_off(c2) else b"", t.tile, t.tail), t.k - c2,
                       "overlap_pairs: the text behind the range, from byte %d on" % (lo + len(want)))
    assert device_all(out[n:], GUARD)


def test_refusals_keep_their_64_bit_numbers(big):
    t, d = device_text("S:base")
    out = guarded(1 << 20)
    with pytest.raises(capi.SfqError) as e:
        big.pick_lines(d.data_ptr(), t.nbytes, capi.PICK_NAMES, out.data_ptr(), 1 << 20, t.nrec - 10, 11)
    assert e.value.code == E_ARG and "%d..+11" % (t.nrec - 10) in str(e.value) and "text's %d records" % t.nrec in str(e.value), str(e.value)
    assert device_all(out, GUARD)
    del out
    need = sum(len(picked(p, capi.PICK_FASTA)) * (t.k if i == 1 else 1) for i, p in enumerate(t.pieces))
    assert need > 1 << 31
    out = guarded(need)
    with pytest.raises(capi.SfqError) as e:
        big.pick_lines(d.data_ptr(), t.nbytes, capi.PICK_FASTA, out.data_ptr(), need - 1)
    assert (e.value.code, e.value.needed) == (E_OVERFLOW, need), str(e.value)
    assert device_all(out, GUARD), "a refused call wrote to its output"
    # the same for a result of more than 2^32 bytes: a trim that cuts nothing, into 2^32 bytes
    del out
    out = guarded(t.nbytes)
    with pytest.raises(capi.SfqError) as e:
        big.trim_records(d.data_ptr(), t.nbytes, capi.Trim(), out.data_ptr(), MARK)
    assert e.value.code == E_OVERFLOW and e.value.needed == t.nbytes > MARK, (str(e.value), e.value.needed)
    assert device_all(out, GUARD), "a refused call wrote to its output"


# ---- checksums ---------------------------------------------------------------------------------------------------------------------------

def test_crc32_of_ranges_around_the_mark(big):
    t, d = device_text("S:base")
    bounds = [MARK - 64, MARK - 17, MARK - 1, MARK, MARK + 1, MARK + 16, MARK + 63, MARK + 64]
    near = LT.expected_bytes(t.pieces, t.k, MARK - 64, MARK + 64)
    want = [zlib.crc32(near[a - MARK + 64:b - MARK + 64]) for a, b in zip(bounds, bounds[1:])]
    assert big.crc32(d.data_ptr(), bounds) == want
    for a, b in ((MARK - 64, MARK + 64), (MARK, MARK + 64), (MARK - 64, MARK), (MARK - 1, MARK + 1)):
        assert big.crc32(d.data_ptr(), [a, b]) == [zlib.crc32(near[a - MARK + 64:b - MARK + 64])], (a, b)


def test_crc32_of_the_text_up_to_the_mark_and_whole(big):
    t, d = device_text("S:base")
    whole, (part,) = LT.crc32_tiled(t.pieces, t.k, [MARK + 5])
    assert big.crc32(d.data_ptr(), [0, MARK + 5]) == [part]
    assert big.crc32(d.data_ptr(), [0, t.nbytes]) == [whole]
    tail = LT.expected_bytes(t.pieces, t.k, MARK + 5, MARK + 5 + 100)
    assert big.crc32(d.data_ptr(), [0, MARK + 5, MARK + 105]) == [part, zlib.crc32(tail)]
    # a long range that begins behind the mark: the rest of the text, from the host's pieces
    rest = LT.expected_bytes(t.pieces, t.k, MARK + 5, t.nbytes)
    assert len(rest) > 2 * t.T and big.crc32(d.data_ptr(), [MARK + 5, t.nbytes]) == [zlib.crc32(rest)]


# ---- two inputs ------------------------------------------------------------------------------------------------------------------------------

def test_interleave_and_check_mates(big):
    """A: 4 GiB of reads.  B: as many reads of one base, a few hundred MB: A's read offsets and the output's cross the mark, B's do not"""
    import torch
    held.clear()
    torch.cuda.empty_cache()
    a, b = LT.text("A"), LT.text("B")
    A, B = a.device(), b.device()
    torch.cuda.synchronize()
    both = interleaved(a.tile, b.tile)
    out = guarded(a.nbytes + b.nbytes)
    n, pairs = big.interleave(A.data_ptr(), a.nbytes, B.data_ptr(), b.nbytes, out.data_ptr(), a.nbytes + b.nbytes)
    assert pairs == a.nrec == b.nrec
    tiled_result(out, n, (b"", both, b""), a.k, "interleave")
    del out
    rep = big.check_mates(A.data_ptr(), a.nbytes, B.data_ptr(), b.nbytes)
    assert (rep.n_pairs, rep.n_mismatch) == (a.nrec, 0)
    # one name spoiled in a pair behind the mark
    p = a.copy_first((MARK - a.H) // a.T + 1) + 77
    off = a.record_off(p)
    assert off > MARK and a.record(p)[:2] == b"@a" and b.record(p)[:2] == b"@a"
    A[off + 1] = ord("b")
    torch.cuda.synchronize()
    rep = big.check_mates(A.data_ptr(), a.nbytes, B.data_ptr(), b.nbytes)
    assert (rep.n_pairs, rep.n_mismatch, rep.first_mismatch, rep.first_off_a, rep.first_off_b) == (a.nrec, 1, p, off, b.record_off(p))


# ---- the coding entries ------------------------------------------------------------------------------------------------------------------------

FROZEN = capi.TABLES_FROZEN
SIDE = ("qlt", "rec", "usr.x", "usr.x.q", "usr.pfg", "usr.pfq", "gen.Ns", "gen.Nn", "gen.lc")


class DeviceCall:
    """One sfq_encode_blocks call whose streams stay on the device: the result, the block index, the blobs, and where every block's share of
    every stream begins (the block index's sizes, summed up)"""

    def __init__(self, ctx, d, nbytes, **kw):
        import ctypes as C
        import numpy as np
        import torch
        cap = capi.lib().sfq_encode_bound(nbytes)
        self.out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.res = ctx.encode_device(d.data_ptr(), nbytes, self.out.data_ptr(), cap, **kw)
        self.blocks = ctx.index(self.res.n_blocks)
        self.first, self.prior, self.rec_prior, self.chains = ctx.first_headers(self.res.first_hdr_bytes), ctx.prior(), ctx.rec_prior(), ctx.chains()
        self.crcs, self.text_crc = ctx.checksums()
        self.stats = ctx.text_stats()
        dt = np.dtype([("first_record", "<u8"), ("n_records", "<u4"), ("llen", "<u4"), ("solid", "u1"), ("two_id", "u1"), ("n_byte", "u1"),
                       ("gen_bits", "u1"), ("extra_hi", "<u4"), ("first_hdr_len", "<u4"), ("first_hdr_off", "<u8"), ("size", "<u8", (capi.NSTREAMS,)),
                       ("status", "<u4"), ("hdr_bytes", "<u4")], align=True)
        assert dt.itemsize == C.sizeof(capi.BlockInfo)
        self.table = np.frombuffer(self.blocks, dt)
        size = self.table["size"].astype(np.uint64)
        self.at = np.cumsum(size, axis=0) - size + np.array(list(self.res.stream_offset), np.uint64)
        assert [int(x) for x in size.sum(axis=0)] == list(self.res.stream_bytes)

    def share(self, name, b):
        """block b's bytes of the stream, on the device"""
        s = capi.STREAM_NAMES.index(name)
        return self.out[int(self.at[b, s]):int(self.at[b, s]) + int(self.table["size"][b, s])]

    def decode_args(self):
        return self.blocks, self.first, self.out.data_ptr(), list(self.res.stream_offset)

    def decode_kw(self):
        return dict(prior=self.prior, level=3, chains=self.chains, rec_prior=self.rec_prior)


def first_vints(blob, n):
    """the first n numbers of a "chn.idx" (util._vints reads all of them: a million here)"""
    out, p = [], 0
    while len(out) < n:
        v = sh = 0
        while True:
            c = blob[p]; p += 1
            v |= (c & 0x7f) << sh; sh += 7
            if not c & 0x80:
                break
        out.append(v)
    return out


@pytest.fixture
def coding(big):
    try:
        yield big
    finally:
        big.set_checksums(False)
        big.set_stats(False)
        big.set_priors(b"", b"")


def test_coding_with_a_given_prior(coding):
    """(a) Priors of head + tile alone, installed: blocks that hold the same records hold the same bytes wherever they lie.  Blocks 1 .. 3 of
    head + tile pass the oracle at that size (check_against_oracle, as the suite does now); their twins in front of, across and behind the
    mark and at the text's end must equal them.  Then the whole call decodes to the text, windows of blocks to their records; the checksums
    and the statistics are the text's."""
    import numpy as np
    import torch
    from test_frozen_tables import check_against_oracle
    from test_text_stats import ref_stats
    ctx = coding
    t, d = device_text("U")
    br, cr = LT.U_BLOCK_READS, LT.U_CHAIN_READS
    per = len(t.rt) // br
    kw = dict(level=3, block_reads=br, tables=FROZEN, chain_reads=cr)
    first = t.head + t.tile
    small = check_against_oracle(ctx, first, 3, br, cr, 1, what="head + tile")
    ctx.set_priors(small.prior, small.rec_prior)
    ctx.set_checksums(True); ctx.set_stats(True)
    call = DeviceCall(ctx, d, t.nbytes, prior_step=capi.PRIOR_GIVEN, **kw)
    assert (call.res.n_records, call.res.n_blocks) == (t.nrec, -(-t.nrec // br))
    assert (call.prior, call.rec_prior) == (small.prior, small.rec_prior)
    assert [int(x) for x in call.table["first_record"][:3]] == [0, br, 2 * br] and int(call.table["n_records"][-2]) == br
    # twins: block b holds records b * br ..., record r >= 1 is the tile's (r - 1) % R: block b + per * j holds what block b holds
    at = t.mark()[0] // br
    last = (1 + t.k * len(t.rt)) // br - 1                          # the last block inside the copies
    assert call.at[at].max() < call.out.numel() and int(call.table["first_record"][at]) == at * br
    for b in (1, 2, 3, 4):
        twins = [x for x in list(range(at - per, at + per + 1)) + list(range(last - per + 1, last + 1)) if (x - b) % per == 0]
        assert len(twins) >= 3 and t.records(b * br, br) == t.records(twins[-1] * br, br)
        for name in SIDE:
            want = call.share(name, b)
            if b < 4:                                            # (block 4 of head + tile is its last record alone)
                device_equal_bytes(want, 0, small.stream(name, b), "block %d of the text against block %d of head + tile, %s" % (b, b, name))
                assert want.numel() == len(small.stream(name, b))
            for x in twins:
                got = call.share(name, x)
                assert got.numel() == want.numel() and torch.equal(got, want), "%s of block %d differs from its twin, block %d" % (name, x, b)
        assert len({call.crcs[x] for x in twins + [b]}) == 1 and call.crcs[b] == zlib.crc32(t.records(b * br, br))
    # checksums and statistics
    assert len(call.crcs) == call.res.n_blocks and call.crcs[at] == zlib.crc32(t.records(at * br, br))
    assert call.crcs[-1] == zlib.crc32(t.records((call.res.n_blocks - 1) * br, t.nrec - (call.res.n_blocks - 1) * br))
    assert call.text_crc == LT.crc32_tiled(t.pieces, t.k)[0]
    st = [ref_stats(p) for p in t.pieces]
    for name, ty in capi.TextStats._fields_:
        got, h, m, l = (getattr(x, name) for x in [call.stats] + st)
        if name in ("seq_len_min", "seq_len_max"):
            assert got == (min if name.endswith("min") else max)(h, m, l), name
        elif isinstance(got, int):
            assert got == h + t.k * m + l, name
        else:
            assert list(got) == [x + t.k * y + z for x, y, z in zip(h, m, l)], name
    # back: the whole call, a window across the mark, the last blocks
    ctx.set_checksums(False); ctx.set_stats(False)
    out = guarded(t.nbytes)
    n, _ = ctx.decode_device(*call.decode_args(), out.data_ptr(), t.nbytes, **call.decode_kw())
    assert n == t.nbytes
    device_equal_tiled(out, t.pieces, t.k, "decode_device")
    assert device_all(out[n:], GUARD)
    del out
    nb = call.res.n_blocks
    for b0, cnt in ((at - 1, 3), (nb - 2, 2)):
        want = t.records(b0 * br, min(cnt * br, t.nrec - b0 * br))
        out = guarded(len(want))
        n, res = ctx.decode_range_device(*call.decode_args(), b0, cnt, out.data_ptr(), len(want), crcs=call.crcs[b0:b0 + cnt], **call.decode_kw())
        assert (n, res.n_blocks) == (len(want), cnt)
        device_equal_bytes(out, 0, want, "decode_range_device of blocks %d..+%d" % (b0, cnt))
        assert device_all(out[n:], GUARD)
    text_untouched("U", "the coding entries")


def test_match_model_walk_of_a_4_gib_stage(coding):
    """(b) Genome-like records, long base lines and quality lines of three bytes: the staged bases and a '\\n' a record reach 2^32, which takes
    gm.hip's u64 instantiation of the walk (gm_plan_line<..., u64>, k_gm_decode_c<TH, u64>).  There is NO reference at this size: the oracle's
    match model would take minutes on 4 GiB.  The check is the exact round trip through decode_device, and a window of the last blocks, whose
    base chains lie behind the mark of the stage."""
    from test_frozen_tables import gm_table_bits
    ctx = coding
    held.clear()
    t, d = device_text("L")
    stage = sum((len(r.split(b"\n")[1]) + 1) * (t.k if i == 1 else 1) for i, p in enumerate(t.pieces) for r in records(p))
    assert stage >= MARK
    br, cr = LT.L_BLOCK_READS, LT.L_CHAIN_READS
    call = DeviceCall(ctx, d, t.nbytes, level=3, block_reads=br, prior_step=1, tables=FROZEN, chain_reads=cr)
    v = first_vints(call.chains, 3)
    assert v[1] & 1 and v[1] & 32, "the match model is off: flags %#x" % v[1]
    assert v[2] == gm_table_bits(t.nbytes)
    out = guarded(t.nbytes)
    n, _ = ctx.decode_device(*call.decode_args(), out.data_ptr(), t.nbytes, **call.decode_kw())
    assert n == t.nbytes
    device_equal_tiled(out, t.pieces, t.k, "decode_device")
    assert device_all(out[n:], GUARD)
    del out
    nb = call.res.n_blocks
    want = t.records((nb - 3) * br, t.nrec - (nb - 3) * br)
    out = guarded(len(want))
    n, res = ctx.decode_range_device(*call.decode_args(), nb - 3, 3, out.data_ptr(), len(want), **call.decode_kw())
    assert (n, res.n_blocks) == (len(want), 3)
    device_equal_bytes(out, 0, want, "decode_range_device of the last three blocks")
    text_untouched("L", "the coding entries")
    held.clear()

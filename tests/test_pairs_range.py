"""sfq_split_pairs_range (pair.hip): a window of records cut out of a text and split into its even and odd records in
one copy, against two slices of records(fq); windows whose ends fall on every border of the kernels, in buffers at every alignment
and between guard bytes; the refusals.  Every comparison is exact byte equality."""
import numpy as np
import pytest

from test_pairs import (Buf, E_ARG, E_FORMAT, E_OVERFLOW, ROW, SCAN_BLOCK, SPAN, UNIT, WG_TILE, WINDOW, first_difference,
                        longer_first_header, reads, record, records, split, starts_of)
from slimfastq_amd import capi

pytestmark = pytest.mark.gpu


def halves(r, lo, n):
    return b"".join(r[lo:lo + n:2]), b"".join(r[lo + 1:lo + n:2])


def check(ctx, fq, lo, n, offs=(0, 0), what="", r=None):
    """records [lo, lo + n) of fq; offs: the device offsets of the text and of the output"""
    r = records(fq) if r is None else r
    assert 0 <= lo and lo + n <= len(r) and n > 0 and n % 2 == 0
    first, second = halves(r, lo, n)
    want = first + second
    T, out = Buf(len(fq), offs[0], fq), Buf(len(want), offs[1])
    at, nbytes = ctx.split_pairs_range(T.ptr, len(fq), lo, n, out.ptr, out.n)
    got = out.back("the output of the window %d:%d %s" % (lo, n, what))
    assert T.back("the text") == fq
    assert (at, nbytes) == (len(first), len(want)), what
    first_difference(got, want, "%s: records %d..+%d, offsets %s" % (what, lo, n, offs))
    return want


def test_the_whole_text_is_split_pairs_byte_for_byte(ctx):
    fq = reads(2 * (SCAN_BLOCK + 3), 1, 120, seed=1)
    r = records(fq)
    want = check(ctx, fq, 0, len(r), (3, 5), "the whole text", r)
    assert want == split(fq)
    T, out = Buf(len(fq), 3, fq), Buf(len(fq), 5)
    at, pairs = ctx.split_pairs(T.ptr, len(fq), out.ptr, out.n)
    assert out.back("sfq_split_pairs") == want and (at, pairs) == (len(b"".join(r[0::2])), len(r) // 2)


def test_small_windows_at_both_ends_and_at_odd_and_even_records(ctx):
    fq = reads(41, 1, 90, seed=2)                                    # an odd record count: a window does not mind
    r = records(fq)
    for n in (2, 4):
        for lo in (0, 1, 2, 7, 8, len(r) - n - 1, len(r) - n):
            check(ctx, fq, lo, n, what="a small window", r=r)


@pytest.mark.parametrize("pairs", (1, WINDOW - 1, WINDOW, WINDOW + 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1))
def test_pair_counts(ctx, pairs):
    fq = reads(2 * (SCAN_BLOCK + 1) + 6, 1, 40, seed=3)
    r = records(fq)
    for lo in (3, 4):
        check(ctx, fq, lo, 2 * pairs, what="%d pairs" % pairs, r=r)


def test_alignment(ctx):
    fq = reads(40, 90, 110, seed=4)
    r = records(fq)
    assert len(b"".join(r[5:31])) > 4 * ROW
    for off in range(UNIT):
        check(ctx, fq, 5, 26, (off, 0), "the text's offset", r)     # the window's first source byte at every offset ...
        check(ctx, fq, 5, 26, (0, off), "the output's offset", r)   # ... and the output's first byte


@pytest.mark.parametrize("border", (SPAN, WG_TILE))
def test_a_window_that_begins_or_ends_at_a_record_on_and_around_a_border(ctx, border):
    base = reads(900, 80, 120, seed=border)
    assert len(base) > WG_TILE + 2 * SPAN
    for d in (-1, 0, 1):
        target = border + d
        s = starts_of(base)
        near = int(s[(s <= target) & (s > 0)].max())
        fq = longer_first_header(base, target - near)
        r = records(fq)
        s = starts_of(fq)
        k = int(np.flatnonzero(s == target)[0])
        assert k >= 21
        check(ctx, fq, k, 320, what="the first record starts at %d" % target, r=r)           # more than a tile of output
        check(ctx, fq, k - 19, 20, what="the last record starts at %d" % target, r=r)
        m = 301 if k >= 301 else k - 1 + k % 2                      # an odd number of records in front of it
        check(ctx, fq, k - m, m + 1, what="the last record starts at %d, a long window" % target, r=r)


@pytest.mark.parametrize("where", ("first", "last", "before", "after"))
def test_one_long_record_in_and_next_to_the_window(ctx, where):
    rng = np.random.default_rng(5)
    long = record(rng, 200000)
    recs = [record(rng, 100) for _ in range(60)]
    lo, n = 20, 20
    recs[{"first": lo, "last": lo + n - 1, "before": lo - 1, "after": lo + n}[where]] = long
    fq = b"".join(recs)
    check(ctx, fq, lo, n, (7, 9), "a long record: " + where, recs)
    check(ctx, fq, lo - 1, n + 2, (0, 0), "a long record inside, " + where, recs)


def test_a_text_without_the_final_line_end(ctx):
    fq = reads(30, 50, 150, seed=6)[:-1]
    r = records(fq)
    assert not r[-1].endswith(b"\n")
    want = check(ctx, fq, 20, 10, what="the last record inside the window", r=r)
    assert not want.endswith(b"\n")
    check(ctx, fq, 19, 10, what="the last record inside, an odd first record", r=r)
    check(ctx, fq, 18, 10, what="the last record outside the window", r=r)
    check(ctx, fq, 0, 30, what="the whole text", r=r)


def test_smallest_records_and_empty_lines(ctx):
    a, e = b"@\nA\n+\nI\n", b"@h\n\n+\n\n"
    assert len(a) < UNIT
    fq = a * 3 + e * 70 + a.replace(b"A", b"C") * 70 + e * 5
    r = records(fq)
    for lo, n in ((0, 2), (1, 2), (0, len(r)), (2, 100), (3, 130), (len(r) - 2, 2)):
        check(ctx, fq, lo, n, (1, 15), "eight-byte records", r)


def refused(ctx, code, fq, lo, n, cap=None, needs=None):
    """the call fails with `code` and leaves its output and the guards as they were"""
    T, out = Buf(len(fq), 0, fq), Buf(len(fq), 5)
    with pytest.raises(capi.SfqError) as e:
        ctx.split_pairs_range(T.ptr, len(fq), lo, n, out.ptr, out.n if cap is None else cap)
    assert e.value.code == code, str(e.value)
    assert out.back("the output of a refused call") == b"I" * out.n, "a refused call wrote to its output"
    assert T.back("the text") == fq
    if needs is not None:
        assert e.value.needed == needs


def test_refusals(ctx):
    fq = reads(20, 30, 60, seed=7)
    r = records(fq)
    refused(ctx, E_FORMAT, fq, 0, 3)                                 # an odd count
    refused(ctx, E_FORMAT, fq, 4, 0)                                 # none
    refused(ctx, E_ARG, fq, 0, 22)                                   # past the end
    refused(ctx, E_ARG, fq, 19, 2)
    refused(ctx, E_ARG, fq, 20, 2)
    refused(ctx, E_ARG, fq, 1 << 62, 2)
    refused(ctx, E_ARG, fq, 2, (1 << 64) - 2)
    refused(ctx, E_FORMAT, fq + b"extra\n", 0, 2)                    # the text's own rules: five lines at its end
    need = len(b"".join(r[3:9]))
    refused(ctx, E_OVERFLOW, fq, 3, 6, cap=need - 1, needs=need)     # one byte short
    refused(ctx, E_OVERFLOW, fq, 0, 20, cap=0, needs=len(fq))
    check(ctx, fq, 3, 6, what="after the refusals", r=r)

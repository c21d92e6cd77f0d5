"""BGZF members deflated on the GPU (bgz.hip): sfq_bgzf_deflate against zlib.  bgzf_check.py walks every result member
by member (header, BSIZE chain, a deflate stream that ends exactly at the trailer, CRC, ISIZE) and gzip.decompress must agree; the
members are also compared byte for byte with bgzf_model.cpp's, the same deflater run serially on the CPU -- the parse is a function of
the piece alone, so the two must not differ anywhere.  Sizes around the piece, texts that aim at one edge of RFC 1951 each, parts,
placement at every alignment between guard bytes, the refusals."""
import gzip
import os
import zlib

import numpy as np
import pytest

from slimfastq_amd import capi
import bgzf_check
from test_bgzf_host import fibonacci_text, limit_texts, model      # noqa: F401  (model: the fixture)
from test_pairs import Buf, E_ARG, E_OVERFLOW

pytestmark = pytest.mark.gpu
PIECE = 65280
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_gold = {}


def golden(name, n=1500000):
    if name not in _gold:
        _gold[name] = gzip.open(os.path.join(GOLDEN, name + ".fq.gz")).read()[:n]
    return _gold[name]


def deflate(ctx, text, bounds=None, offs=(0, 0), slack=41):
    """sfq_bgzf_deflate of text; returns (the result's bytes, part offsets, report).  The output holds `slack` bytes more than the
    bound: they and the guards of both buffers come back as they were."""
    bounds = [0, len(text)] if bounds is None else bounds
    T = Buf(len(text), offs[0], text)
    out = Buf(capi.bgzf_bound(bounds[-1] - bounds[0], len(bounds) - 1) + slack, offs[1])
    off, rep = ctx.bgzf_deflate(T.ptr, bounds, out.ptr, out.n)
    got = out.back("the BGZF output")
    assert T.back("the text") == text, "the text was written"
    n = rep.out_bytes
    assert off[-1] == n and off[0] == 0 and off == sorted(off)
    assert got[n:] == b"I" * (out.n - n), "bytes behind the result were written"
    assert rep.text_bytes == bounds[-1] - bounds[0]
    return got[:n], off, rep


def checked(ctx, text, model=None, **kw):
    got, off, rep = deflate(ctx, text, **kw)
    assert bgzf_check.check(got, off) == text
    ms = bgzf_check.members(got)
    assert rep.members == len(ms) == -(-len(text) // PIECE)
    assert rep.stored_members == sum(m[4] for m in ms)
    assert all(m[1] <= len(m[3]) + 31 for m in ms), "a member larger than stored"
    if model is not None:
        assert got == model(text), "the kernel's members differ from the CPU model's"
    return got, ms, rep


@pytest.mark.parametrize("n", [1, 3, 4, 65279, 65280, 65281, 2 * 65280, 2 * 65280 + 1])
def test_sizes(ctx, model, n):
    checked(ctx, golden("tst7")[:n], model)


def test_no_match_possible(ctx, model):
    checked(ctx, bytes(range(256)) * 4, model)


def test_one_byte_repeated(ctx, model):
    """distance 1, length 258: matches that run into themselves, one distance symbol (sent with one bit), three literal/length symbols"""
    got, ms, rep = checked(ctx, b"A" * PIECE, model)
    assert rep.stored_members == 0 and len(got) < 400


def test_repeated_record(ctx, model):
    rng = np.random.default_rng(5)
    rec = bytes(rng.integers(33, 90, 299, dtype=np.uint8)) + b"\n"
    text = (rec * 701)[:210000]
    got, _, _ = checked(ctx, text, model)
    assert len(got) <= 0.05 * len(text), len(got)


def test_random_bytes_are_stored(ctx, model):
    text = bytes(np.random.default_rng(6).integers(0, 256, 2 * PIECE, dtype=np.uint8))
    got, ms, rep = checked(ctx, text, model)
    assert rep.stored_members == rep.members == 2
    assert all(m[4] and m[1] == len(m[3]) + 31 for m in ms)


def test_fibonacci_counts(ctx, model):
    """24 values with Fibonacci counts (test_bgzf_host.fibonacci_text).  The parse turns so many of the frequent literals into matches
    that the tree over what is left is 14 levels deep here: the limit does not act on this text -- test_length_limits_act's do that."""
    text = fibonacci_text()
    lit = np.bincount(np.frombuffer(text, np.uint8))
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    assert sorted(int(c) for c in lit[lit > 0]) == sorted(fib + [1, PIECE - sum(fib) - 1])
    checked(ctx, text, model)


def test_length_limits_act(ctx, model):
    """Texts whose literals stay literals (no four bytes occur twice), so that the histogram is the text's own: one whose
    literal/length tree is 16 levels deep, one whose code-length tree is deeper than 7 -- the model says so (limit_texts asserts it).
    The kernel's clamp and its fold run on both; zlib refuses an over-subscribed or incomplete code, and the members are the model's
    byte for byte."""
    deep, cl = limit_texts(model)
    for text in (deep, cl):
        got, ms, rep = checked(ctx, text, model)
        assert rep.stored_members == 0


def test_forty_equal_symbols_and_one(ctx, model):
    rng = np.random.default_rng(7)
    checked(ctx, bytes(rng.permutation(np.repeat(np.arange(40, dtype=np.uint8) + 48, 500))), model)
    checked(ctx, b"x", model)


@pytest.mark.parametrize("name", ["tst7", "tst1", "small"])
def test_ratio_against_zlib_level_1(ctx, model, name):
    """deflate bytes (member sizes - 26 each) <= 1.05 x zlib level 1 over the same pieces"""
    text = golden(name)
    got, ms, _ = checked(ctx, text, model)
    ours = sum(m[2] for m in ms)
    theirs = 0
    for at in range(0, len(text), PIECE):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        theirs += len(c.compress(text[at:at + PIECE]) + c.flush())
    print("%s: %d bytes, deflate %d, zlib level 1 %d, ratio %.4f" % (name, len(text), ours, theirs, ours / theirs))
    assert ours <= 1.05 * theirs, (ours, theirs, ours / theirs)


# ---- parts ------------------------------------------------------------------------------------------------------------------------------

def test_parts_at_odd_bounds(ctx):
    text = golden("tst7")[:200003]
    for bounds in ([0, 0, 70001, 200003], [0, 70001, 70001, 200003], [0, 70001, 200003, 200003], [3, 65283, 65284, 199999]):
        got, off, rep = deflate(ctx, text, bounds)
        assert bgzf_check.check(got, off) == text[bounds[0]:bounds[-1]]
        for i in range(len(bounds) - 1):
            assert bgzf_check.check(got[off[i]:off[i + 1]]) == text[bounds[i]:bounds[i + 1]]
        assert rep.members == sum(-(-(b - a) // PIECE) for a, b in zip(bounds, bounds[1:]))


def test_a_part_alone_and_as_a_range(ctx):
    """the same piece gives the same member whatever else is in the call and wherever it lies in memory"""
    text = golden("tst7")[:200003]
    bounds = [0, 1001, 70001, 200003]
    got, off, _ = deflate(ctx, text, bounds)
    for i in range(3):
        part = text[bounds[i]:bounds[i + 1]]
        for o in (0, 5):
            alone, _, _ = deflate(ctx, part, offs=(o, 0))
            assert alone == got[off[i]:off[i + 1]], "part %d alone at offset %d" % (i, o)


def test_same_call_twice(ctx):
    text = golden("tst1")[:300000]
    a = deflate(ctx, text, [0, 100000, 300000])
    b = deflate(ctx, text, [0, 100000, 300000])
    assert a[0] == b[0] and a[1] == b[1]


def test_empty_text(ctx):
    T, out = Buf(16, 0, b"x" * 16), Buf(64, 0)
    off, rep = ctx.bgzf_deflate(T.ptr, [4, 4, 4], out.ptr, out.n)
    assert off == [0, 0, 0] and (rep.text_bytes, rep.out_bytes, rep.members, rep.stored_members) == (0, 0, 0, 0)
    assert out.back("the output") == b"I" * 64


# ---- placement --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offs", [(1, 15), (7, 1), (15, 7)])
def test_any_alignment(ctx, offs):
    text = golden("tst7")[:PIECE + 4097]
    want, _, _ = deflate(ctx, text)
    got, off, _ = deflate(ctx, text, offs=offs)
    assert got == want
    got, off, _ = deflate(ctx, text, [0, 33, len(text)], offs=offs)
    assert bgzf_check.check(got, off) == text


def test_overflow_and_arguments(ctx):
    text = golden("tst7")[:PIECE + 4097]
    want, _, rep = deflate(ctx, text)
    T = Buf(len(text), 3, text)
    out = Buf(len(want) - 1, 5)
    with pytest.raises(capi.SfqError) as e:
        ctx.bgzf_deflate(T.ptr, [0, len(text)], out.ptr, out.n)
    assert e.value.code == E_OVERFLOW and e.value.needed == len(want)
    assert out.back("the refused output") == b"I" * out.n
    out = Buf(len(want), 5)                                            # exactly enough
    off, rep = ctx.bgzf_deflate(T.ptr, [0, len(text)], out.ptr, out.n)
    assert out.back("the output") == want
    L, h = capi.lib(), ctx._h
    import ctypes as C
    b, o, r = (C.c_uint64 * 3)(0, 10, 20), (C.c_uint64 * 3)(), capi.BgzfReport()
    vp = C.c_void_p
    assert L.sfq_bgzf_deflate(h, None, b, 2, vp(out.ptr), out.n, o, C.byref(r)) == E_ARG
    assert L.sfq_bgzf_deflate(h, vp(T.ptr), None, 2, vp(out.ptr), out.n, o, C.byref(r)) == E_ARG
    assert L.sfq_bgzf_deflate(h, vp(T.ptr), b, 2, None, out.n, o, C.byref(r)) == E_ARG
    assert L.sfq_bgzf_deflate(h, vp(T.ptr), b, 2, vp(out.ptr), out.n, None, C.byref(r)) == E_ARG
    assert L.sfq_bgzf_deflate(h, vp(T.ptr), b, 0, vp(out.ptr), out.n, o, C.byref(r)) == E_ARG
    bad = (C.c_uint64 * 3)(0, 20, 10)
    assert L.sfq_bgzf_deflate(h, vp(T.ptr), bad, 2, vp(out.ptr), out.n, o, C.byref(r)) == E_ARG
    assert L.sfq_bgzf_deflate(h, vp(T.ptr), b, 2, vp(out.ptr), out.n, o, None) == 0      # the report may be NULL
    assert out.back("the output")[:o[2]] and bgzf_check.check(out.back("the output")[:o[2]], list(o)) == text[:20]

"""Mates by name (pair.hip k_pair_names, slimfastq_amd.h): sfq_check_mates on two texts and on one interleaved text against the rule
written out in Python, with names of every length around the kernel's 16-byte steps and header lines at every alignment; the
count, the first pair and its offsets are exact; the switch of sfq_encode_pairs_host."""
import ctypes as C

import numpy as np
import pytest

from test_pairs import Buf, E_FORMAT, UNIT, interleaved, mates, same_archive, starts_of
from slimfastq_amd import capi

pytestmark = pytest.mark.gpu


def name(header: bytes) -> bytes:
    """the rule: the first line behind its first byte, up to the first ' ' or '\\t', without a "/1" or "/2" at its end"""
    x = header[1:]
    for i, c in enumerate(x):
        if c in b" \t":
            x = x[:i]
            break
    return x[:-2] if len(x) >= 2 and x[-2:] in (b"/1", b"/2") else x


def text(headers, seed=0):
    """a record per header, of 1 .. 40 bases, so that the header lines start anywhere"""
    rng = np.random.default_rng(seed)
    out = []
    for h in headers:
        assert b"\n" not in h
        n = int(rng.integers(1, 41))
        out.append(h + b"\n" + b"ACGT" * (n // 4) + b"A" * (n % 4) + b"\n+\n" + b"I" * n + b"\n")
    return b"".join(out)


def check(ctx, ha, hb, offs=(0, 0), what=""):
    """both forms of sfq_check_mates on records with the headers ha[i] and hb[i]; returns the pairs that differ"""
    bad = [i for i, (x, y) in enumerate(zip(ha, hb)) if name(x) != name(y)]
    a, b = text(ha, 1), text(hb, 2)
    both = interleaved(a, b)
    sa, sb, s2 = starts_of(a), starts_of(b), starts_of(both)
    A, B, T = Buf(len(a), offs[0], a), Buf(len(b), offs[1], b), Buf(len(both), offs[0], both)
    two = ctx.check_mates(A.ptr, len(a), B.ptr, len(b))
    one = ctx.check_mates(T.ptr, len(both))
    assert (A.back("A"), B.back("B"), T.back("the interleaved text")) == (a, b, both)
    for r, oa, ob in ((two, sa, sb), (one, s2[0::2], s2[1::2])):
        assert (r.n_pairs, r.n_mismatch) == (len(ha), len(bad)), (what, r.n_pairs, r.n_mismatch, bad[:5])
        if bad:
            assert (r.first_mismatch, r.first_off_a, r.first_off_b) == (bad[0], oa[bad[0]], ob[bad[0]]), what
    return bad


def test_the_examples_of_the_rule(ctx):
    same = [(b"@r/1", b"@r/2"), (b"@r 1:N:0:ACGT", b"@r 2:N:0:ACGT"), (b"@r/1", b"@r"), (b"@", b"@"), (b"@/1", b"@"), (b"@ x", b"@\ty"),
            (b"@r\t1", b"@r 2"), (b"@r/2", b"@r/2"), (b"@r/1/1", b"@r/1/2"), (b"@/", b"@/"), (b"@1", b"@1")]
    differ = [(b"@r1", b"@r10"), (b"@ra", b"@rb"), (b"@r/1", b"@r/3"), (b"@r/1/1", b"@r"), (b"@r", b"@"), (b"@/1", b"@/"), (b"@a/1", b"@b/1"),
              (b"@r/", b"@r"), (b"@1", b"@2")]
    for x, y in same:
        assert name(x) == name(y)
        assert check(ctx, [x], [y], what="%r %r" % (x, y)) == []
        assert check(ctx, [y], [x]) == []
    for x, y in differ:
        assert name(x) != name(y)
        assert check(ctx, [x], [y], what="%r %r" % (x, y)) == [0]
        assert check(ctx, [y], [x]) == [0]
    ha, hb = [p[0] for p in same + differ], [p[1] for p in same + differ]
    assert check(ctx, ha, hb) == list(range(len(same), len(same) + len(differ)))


LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33)


def test_name_lengths_and_where_they_differ(ctx):
    rng = np.random.default_rng(3)
    ha, hb, want = [], [], []
    for n in LENGTHS:
        w = bytes(rng.integers(ord("a"), ord("z") + 1, n, dtype=np.uint8))
        tails = ((b"", b""), (b"/1", b"/2"), (b" 1:N:0:A", b" 2:N:0:CCCCCCCCCCCCCCCCCCCCCCCC"), (b"\tx", b" y"), (b"/1", b""))
        for ta, tb in tails:                                          # the same name, what follows differs
            ha.append(b"@" + w + ta); hb.append(b"@" + w + tb); want.append(False)
        if n:
            for at in {0, n - 1}:                                     # only the first byte differs, only the last
                v = bytearray(w); v[at] ^= 1
                for ta, tb in tails[:3]:
                    ha.append(b"@" + w + ta); hb.append(b"@" + bytes(v) + tb); want.append(True)
            ha.append(b"@" + w); hb.append(b"@" + w[:-1]); want.append(True)                 # a proper prefix
            ha.append(b"@" + w[:n // 2] + b" " + w); hb.append(b"@" + w + b" " + w); want.append(n // 2 != n)
            ha.append(b"@" + w + b"/1"); hb.append(b"@" + w + b"x/2"); want.append(True)    # differ in front of the slash
    assert [name(x) != name(y) for x, y in zip(ha, hb)] == want
    assert check(ctx, ha, hb) == [i for i, w in enumerate(want) if w]
    assert check(ctx, hb, ha) == [i for i, w in enumerate(want) if w]
    for x, y, w in zip(ha, hb, want):                                 # and each alone: the first pair, the text's first bytes
        assert check(ctx, [x], [y], what="%r %r" % (x, y)) == ([0] if w else [])


def test_header_lines_at_every_alignment(ctx):
    w = b"M7:42:000000000-A7XYZ:1:1101:15589:1332"
    assert len(w) > 2 * UNIT
    ha = [b"@" + w[:k] + b"/1" for k in range(0, len(w), 3)] + [b"@" + w + b" 1:N:0:1"]
    hb = [b"@" + w[:k] + b"/2" for k in range(0, len(w), 3)] + [b"@" + w[:-1] + b"3 2:N:0:1"]
    for off in range(UNIT):
        assert check(ctx, ha, hb, (off, 0), "A's offset") == [len(ha) - 1]
        assert check(ctx, ha, hb, (0, off), "B's offset") == [len(ha) - 1]
        assert check(ctx, ha[:-1], hb[:-1], (off, (off * 7) % UNIT)) == []


def test_a_long_name(ctx):
    rng = np.random.default_rng(4)
    w = bytes(rng.integers(ord("a"), ord("z") + 1, 9000, dtype=np.uint8))
    v = w[:-1] + bytes([w[-1] ^ 1])
    assert check(ctx, [b"@r", b"@" + w + b"/1", b"@s"], [b"@r", b"@" + w + b"/2 x", b"@s"], (5, 11)) == []
    assert check(ctx, [b"@r", b"@" + w + b"/1", b"@s"], [b"@r", b"@" + v + b"/2 x", b"@s"], (5, 11)) == [1]
    assert check(ctx, [b"@" + w], [b"@" + w + b"a"]) == [0]


N = 1500
_good = None


def good_headers():
    global _good
    if _good is None:
        rng = np.random.default_rng(5)
        _good = [b"@M7:42:%d:%d" % (i, int(rng.integers(0, 10 ** int(rng.integers(1, 9))))) for i in range(N)]
    return _good


@pytest.mark.parametrize("at", (0, 63, 64, 65, 255, 256, 257, N - 1))
def test_one_mismatch_is_found_where_it_is(ctx, at):
    h = good_headers()
    ha, hb = [x + b"/1" for x in h], [x + b"/2" for x in h]
    hb[at] = h[at] + b"x/2"
    assert check(ctx, ha, hb, (at % UNIT, 3)) == [at]


@pytest.mark.parametrize("count", (0, 1, 2, 700))
def test_the_count_is_exact(ctx, count):
    h = good_headers()
    ha, hb = [x + b" 1:N:0:1" for x in h], [x + b" 2:N:0:1" for x in h]
    where = sorted(np.random.default_rng(count).choice(N, count, replace=False).tolist())
    for i in where:
        hb[i] = h[i][:-1] + bytes([h[i][-1] ^ 1]) + b" 2:N:0:1"
    assert check(ctx, ha, hb) == where


def test_the_refusals_of_the_passes_it_shares(ctx):
    a, b = text([b"@r/1"] * 4), text([b"@r/2"] * 3)
    A, B = Buf(len(a), 0, a), Buf(len(b), 0, b)
    with pytest.raises(capi.SfqError) as e:
        ctx.check_mates(A.ptr, len(a), B.ptr, len(b))                # record counts
    assert e.value.code == E_FORMAT
    with pytest.raises(capi.SfqError) as e:
        ctx.check_mates(B.ptr, len(b))                               # an odd number of records
    assert e.value.code == E_FORMAT
    assert ctx.check_mates(A.ptr, len(a)).n_mismatch == 0


# ---- the switch of sfq_encode_pairs_host -------------------------------------------------------------------------------------------

@pytest.fixture
def mctx(ctx):
    try:
        yield ctx
    finally:
        ctx.set_mate_check(False)


def test_encode_pairs_host_refuses_files_out_of_step(mctx):
    ctx = mctx
    a, b = mates(400, 60, seed=6)
    ra = b.split(b"\n")
    bad = b"\n".join(ra[:4 * 123] + ra[4 * 124:4 * 125] + ra[4 * 123:])        # record 124 once more in front of record 123
    assert len(bad.split(b"\n")) == len(ra) + 4
    a2 = a + b"".join(l + b"\n" for l in a.split(b"\n")[-5:-1])                 # and A one record longer: the counts agree
    ha, hb = a2.split(b"\n")[0::4][:-1], bad.split(b"\n")[0::4][:-1]
    wrong = [i for i, (x, y) in enumerate(zip(ha, hb)) if name(x) != name(y)]
    assert wrong[0] == 123 and len(wrong) > 1
    L = capi.lib()
    p = capi.Params(3, 256, 0, 0, 0, 0, capi.PRIOR_AUTO, 0, 0, 0)
    res = capi.Result()
    cap = L.sfq_encode_bound(len(a2) + len(bad))
    out = np.full(cap, 0xA5, np.uint8)
    xa, xb = np.frombuffer(a2, np.uint8), np.frombuffer(bad, np.uint8)
    args = (ctx._h, xa.ctypes.data_as(C.c_void_p), len(a2), xb.ctypes.data_as(C.c_void_p), len(bad), C.byref(p), out.ctypes.data_as(C.c_void_p), cap, C.byref(res))
    assert L.sfq_encode_pairs_host(*args) == 0 and ctx.mate_report() is None
    out[:] = 0xA5
    ctx.set_mate_check(True)
    assert L.sfq_encode_pairs_host(*args) == E_FORMAT
    msg = L.sfq_last_error(ctx._h).decode()
    assert " 123" in msg and name(ha[123]).decode() in msg and name(hb[123]).decode() in msg and str(len(wrong)) in msg, msg
    assert bool((out == 0xA5).all()), "a refused call wrote to its output"
    r = ctx.mate_report()
    assert (r.n_pairs, r.n_mismatch, r.first_mismatch) == (len(ha), len(wrong), 123)
    assert (r.first_off_a, r.first_off_b) == (starts_of(a2)[123], starts_of(bad)[123])
    ctx.set_mate_check(False)
    assert L.sfq_encode_pairs_host(*args) == 0 and ctx.mate_report() is None


def test_encode_pairs_host_on_good_files_codes_what_it_codes_without_the_check(mctx):
    ctx = mctx
    a, b = mates(2000, 100, seed=7)
    kw = dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO)
    off = ctx.encode_pairs_host(a, b, **kw)
    assert ctx.mate_report() is None
    ctx.set_mate_check(True)
    on = ctx.encode_pairs_host(a, b, **kw)
    r = ctx.mate_report()
    assert (r.n_pairs, r.n_mismatch) == (2000, 0)
    assert same_archive(on, off)
    ctx.set_mate_check(False)
    assert same_archive(ctx.encode_pairs_host(a, b, **kw), off) and ctx.mate_report() is None

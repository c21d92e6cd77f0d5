"""BGZF, the host side (no GPU): sfq_bgzf_bound, the end-of-file block, capi.py's argument checks, the report's size -- and the
deflater's serial half on the CPU: bgzf_model.cpp runs the code construction, its length limit, the code-length header and the bit
placement of bgz.hip (the very functions, slimfastq_amd/csrc/bgz_code.h) behind a serial restatement of the parse, and zlib inflates
what it writes."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from slimfastq_amd import capi
import bgzf_check

HERE = os.path.dirname(os.path.abspath(__file__))
PIECE = 65280


def test_bound():
    assert capi.BGZF_PIECE == PIECE == bgzf_check.PIECE
    assert capi.bgzf_bound(0, 1) == 31
    assert capi.bgzf_bound(1, 1) == 1 + 31
    assert capi.bgzf_bound(65280, 1) == 65280 + 62
    assert capi.bgzf_bound(65281, 1) == 65281 + 62
    assert capi.bgzf_bound(2 ** 32 + 1, 1) == 2 ** 32 + 1 + 31 * ((2 ** 32 + 1) // 65280 + 1)
    assert capi.bgzf_bound(65280, 3) == 65280 + 31 * 4
    # a part of n bytes in members of 26 bytes around at most piece + 5: never above the bound
    for n in (1, 65279, 65280, 65281, 3 * 65280):
        assert -(-n // PIECE) * 31 + n <= capi.bgzf_bound(n, 1)


def test_eof_block():
    eof = capi.bgzf_eof()
    assert eof == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000") == bgzf_check.EOF
    assert len(eof) == 28 and gzip.decompress(eof) == b""
    assert bgzf_check.check(eof) == b""
    assert capi.lib().sfq_bgzf_eof(None) == -1


def test_report_size():
    assert C.sizeof(capi.BgzfReport) == 32
    assert [f[0] for f in capi.BgzfReport._fields_] == ["text_bytes", "out_bytes", "members", "stored_members"]


def test_capi_argument_checks():
    class NoCtx(capi.Context):
        def __init__(self):
            self._h = None
    c = NoCtx()
    for bad in ([], [0], [5, 3], [0, 4, 2], [-1, 2]):
        with pytest.raises(ValueError):
            c.bgzf_deflate(0, bad, 0, 0)
    L = capi.lib()
    assert L.sfq_ctx_set_bgzf(None, 1) == -1
    assert L.sfq_get_bgzf(None, None, None, None, 0) == -1
    assert L.sfq_bgzf_deflate(None, None, None, 0, None, 0, None, None) == -1


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bgzf_model") / "bgzf_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(HERE, "bgzf_model.cpp")])

    def run(text, maxbits=15):
        d = os.path.dirname(exe)
        with open(os.path.join(d, "in"), "wb") as f:
            f.write(text)
        said = subprocess.check_output([exe, os.path.join(d, "in"), os.path.join(d, "out"), str(maxbits)]).decode().splitlines()
        # per member: the depths of Huffman's own trees before the limits (literal/length, distance, code lengths), the tokens
        run.members = [tuple(int(v) for v in line.split()) for line in said]
        with open(os.path.join(d, "out"), "rb") as f:
            return f.read()
    return run


def _pairs_once(k):
    """a sequence over 0 .. k - 1 of length k * k in which no pair of neighbours occurs twice (de Bruijn, order 2)"""
    a, seq = [0] * (2 * k), []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return np.array(seq, np.uint8)


def woven(xs, k):
    """xs (byte values below 256 - k) at the even positions, at the odd ones a sequence over the k highest byte values in which no
    pair of neighbours repeats: every four bytes of the text hold such a pair, so no four bytes occur twice, the parse finds no match
    and the literal histogram is the text's own"""
    c = _pairs_once(k)
    assert len(xs) <= len(c) and int(xs.max()) < 256 - k
    out = np.empty(2 * len(xs), np.uint8)
    out[0::2] = xs
    out[1::2] = c[:len(xs)] + (256 - k)
    return out.tobytes()


def deep_literal_text():
    """65280 bytes, all literals: 16 values with counts 1, 1, 2, 4, ... 8192 and the rest, woven with 192 values of 170 each.
    Huffman's tree over them (with the end-of-block symbol) is 16 levels deep: the 15-bit limit has to act."""
    counts = [1, 1] + [2 ** j for j in range(1, 14)]
    counts.append(PIECE // 2 - sum(counts))
    xs = np.concatenate([np.full(c, v, np.uint8) for v, c in enumerate(counts)])
    np.random.default_rng(1).shuffle(xs)
    return woven(xs, 192)


def deep_code_length_text(seed):
    """16384 bytes, all literals, whose literal code has 56, 34, 12, 9, 5 and 3 symbols of 9, 13, 14, 7, 4 and 10 bits (counts 2^(14 - bits),
    woven with 128 values of 64 each, which take 8 bits): with the run of 8s folded into about 21 repeat symbols the code-length
    alphabet's counts are a Fibonacci chain and its tree is deeper than 7 -- for most orders of the symbols; the callers pick a seed
    by asking the model."""
    import random
    lens = [L for c, L in zip((3, 5, 9, 12, 34, 56), (10, 4, 7, 14, 13, 9)) for _ in range(c)]
    random.Random(seed).shuffle(lens)                                  # symbol -> bits: no long runs of one length to fold
    xs = np.concatenate([np.full(2 ** (14 - L), v, np.uint8) for v, L in enumerate(lens)])
    np.random.default_rng(seed).shuffle(xs)
    return woven(xs, 128)


def limit_texts(model):
    """(the text whose literal/length tree is deeper than 15, the text whose code-length tree is deeper than 7), each asked of the model"""
    deep = deep_literal_text()
    model(deep)
    assert len(model.members) == 1 and model.members[0][0] > 15 and model.members[0][3] == len(deep), model.members
    for seed in range(40):
        t = deep_code_length_text(seed)
        model(t)
        if model.members[0][2] > 7:
            assert model.members[0][3] == len(t)
            return deep, t
    raise AssertionError("no order of the symbols makes the code-length tree deeper than 7")


def fibonacci_text():
    """65280 bytes of 24 values: Fibonacci counts 1, 1, 2, ... 17711 for 22 of them, 1 for the 23rd, the rest (18912) for the most
    frequent -- an unlimited Huffman tree over the first 22 alone is 21 levels deep.  Shuffled by a fixed seed."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    fib += [1, PIECE - sum(fib) - 1]
    a = np.concatenate([np.full(c, 65 + i, np.uint8) for i, c in enumerate(fib)])
    np.random.default_rng(11).shuffle(a)
    assert len(a) == PIECE and max(fib) == fib[-1]
    return a.tobytes()


def test_model_members_inflate(model):
    rng = np.random.default_rng(3)
    tst7 = gzip.open(os.path.join(HERE, "golden", "tst7.fq.gz")).read()[:3 * PIECE + 17]
    texts = [tst7, b"x", b"abc", b"abcd", bytes(range(256)) * 4, b"A" * PIECE, fibonacci_text(),
             bytes(rng.integers(0, 256, 70000, dtype=np.uint8)), bytes(rng.permutation(np.repeat(np.arange(40, dtype=np.uint8) + 48, 500)))]
    for t in texts:
        assert bgzf_check.check(model(t)) == t


def test_model_both_limits_act(model):
    """the texts the GPU tests use: Huffman's own trees are deeper than 15 and than 7, and zlib takes what the folds make of them"""
    for t in limit_texts(model):
        assert bgzf_check.check(model(t)) == t


def test_model_length_limit_acts(model):
    """The limit folds too-deep leaves back into a COMPLETE code (zlib refuses anything else) at 15 bits and, so that it acts on many
    symbols, at 9, 10 and 12.  The fold is a heuristic (a limit of 12 may beat 15 by a few bytes); what holds is that nine bits
    cost more than fifteen."""
    t = fibonacci_text()
    sizes = [len(model(t, b)) for b in (9, 10, 12, 15)]
    for b in (9, 10, 12, 15):
        assert bgzf_check.check(model(t, b)) == t
    assert sizes[0] > sizes[-1], sizes

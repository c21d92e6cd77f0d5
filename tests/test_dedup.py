"""Distinct records on the GPU (dd.hip, slimfastq_amd.h "distinct records"): sfq_dedup_records against a restatement of the header's
rule in Python -- a dict over test_pairs.records() -- on the smallest texts, with keys that differ in one byte at every position and
alignment, under probe collisions and contention, with pairs, ranges, in buffers at every alignment between guard bytes, with the
context's set across calls, and every refusal.  Every comparison is exact byte equality.  Every output is filled with a marker: a
call writes its result and nothing else, a refused call nothing at all."""
import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Dedup
from test_pairs import Buf, records, first_difference

pytestmark = pytest.mark.gpu
E_ARG, E_NOMEM, E_FORMAT, E_OVERFLOW, E_UNSUPPORTED = -1, -3, -4, -5, -7
TO_END = 0xFFFFFFFFFFFFFFFF
ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---- the rule --------------------------------------------------------------------------------------------------------------------

def key(rec):
    return rec.split(b"\n")[1].upper()                                # (bytes.upper folds 'a'..'z' alone)


def distinct(fq, d, seen=None):
    """(the kept units' record numbers, n_units, n_dup_set, n_dup_call, the keys the call adds); seen: the set's keys, not changed"""
    rs, G = records(fq), 2 if d.pairs else 1
    hi = len(rs) if d.n_records == TO_END else d.first_record + d.n_records
    assert hi <= len(rs) and (hi - d.first_record) % G == 0
    mine, kept, in_set, in_call = {}, [], 0, 0
    for r in range(d.first_record, hi, G):
        k = tuple(key(rs[r + g]) for g in range(G))
        if seen is not None and k in seen:
            in_set += 1
        elif k in mine:
            in_call += 1
        else:
            mine[k] = r
            kept += list(range(r, r + G))
    return kept, (hi - d.first_record) // G, in_set, in_call, mine


def key_bytes(keys):
    return sum(len(x) for k in keys for x in k)


def check(ctx, fq, d, offs=(0, 0), msg="", slack=37, seen=None):
    """sfq_dedup_records against the rule; returns the kept records' numbers.  seen: the set's keys, which a call with use_set extends"""
    assert (seen is not None) == bool(d.use_set)
    rs = records(fq)
    kept, units, in_set, in_call, mine = distinct(fq, d, seen)
    want = b"".join(rs[r] for r in kept)
    T, out = Buf(len(fq), offs[0], fq), Buf(len(want) + slack, offs[1])
    n, rep = ctx.dedup_records(T.ptr, len(fq), d, out.ptr, out.n)
    got = out.back("the output")
    assert T.back("the text") == fq, "the text was written"
    what = "%s, offsets %s" % (msg, offs)
    assert n == len(want), (what, n, len(want))
    first_difference(got[:n], want, what)
    assert got[n:] == b"I" * (out.n - n), what + ": bytes behind the result were written"
    G = 2 if d.pairs else 1
    if seen is not None:
        seen.update(mine)
    after = (len(seen), key_bytes(seen)) if seen is not None else (0, 0)
    assert (rep.n_in_range, rep.n_units, rep.n_kept, rep.n_dup_set, rep.n_dup_call, rep.text_bytes, rep.kept_bytes, rep.set_keys, rep.set_key_bytes) == \
        (units * G, units, len(kept) // G, in_set, in_call, len(fq), len(want)) + after, what
    if seen is not None:
        assert ctx.dedup_set_info()[:2] == after, what
    return kept


def refused(ctx, code, fq, d, cap=None, needs=None):
    T, out = Buf(max(len(fq), 1), 3, fq if fq else None), Buf(max(len(fq), 1) + 16, 5)
    before = ctx.dedup_set_info()
    with pytest.raises(capi.SfqError) as e:
        ctx.dedup_records(T.ptr, len(fq), d, out.ptr, out.n if cap is None else cap)
    assert e.value.code == code, str(e.value)
    assert out.back("the output of a refused call") == b"I" * out.n, "a refused call wrote to its output"
    if fq:
        assert T.back("the text") == fq
    if needs is not None:
        assert e.value.needed == needs
    assert ctx.dedup_set_info() == before
    return str(e.value)


def rec(bases, quals=None, hdr=b"@r", plus=b"+"):
    return hdr + b"\n" + bases + b"\n" + plus + b"\n" + (b"I" * len(bases) if quals is None else quals) + b"\n"


def bases(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


@pytest.fixture
def dset(ctx):
    """The session's context without a set, before and after."""
    ctx.dedup_set_destroy()
    try:
        yield ctx
    finally:
        ctx.dedup_set_destroy()


# ---- the smallest texts --------------------------------------------------------------------------------------------------------------

def test_smallest_texts(ctx):
    one = rec(b"ACGT")
    assert check(ctx, one, Dedup(), msg="one record") == [0]
    assert check(ctx, one[:-1], Dedup(), msg="one record without its final line end") == [0]
    assert check(ctx, one + rec(b"ACGT", hdr=b"@other", quals=b"#!#!"), Dedup(), msg="two equal records") == [0]
    assert check(ctx, rec(b"acgT") + rec(b"AcGt"), Dedup(), msg="equal but for case") == [0]
    assert check(ctx, rec(b"ACGT") + rec(b"ACGA"), Dedup(), msg="the last byte differs") == [0, 1]
    assert check(ctx, rec(b"ACGT") + rec(b"CCGT"), Dedup(), msg="the first byte differs") == [0, 1]
    assert check(ctx, rec(b"ACG") + rec(b"ACGT") + rec(b"ACG"), Dedup(), msg="a prefix") == [0, 1]
    assert check(ctx, rec(b"") + rec(b"A") + rec(b"", hdr=b"@e"), Dedup(), msg="two empty base lines") == [0, 1]
    # every byte but 'a'..'z' stands: '@' is not '`', '[' is not '{', 'N' 'n' fold, '.' and '\r' are bytes
    assert check(ctx, rec(b"@[AZ") + rec(b"`{az") + rec(b"@[az"), Dedup(), msg="the fold's edges") == [0, 1]
    assert check(ctx, rec(b"AN.\r") + rec(b"an.\r") + rec(b"AN."), Dedup(), msg="N, '.', '\\r'") == [0, 2]
    # the text's last record, without a final '\n': a duplicate there, and a first occurrence there
    assert check(ctx, rec(b"ACGT") + rec(b"GG") + rec(b"ACGT", hdr=b"@last")[:-1], Dedup(), msg="a duplicate at the open end") == [0, 1]
    assert check(ctx, rec(b"ACGT") + rec(b"ACGT") + rec(b"GG", hdr=b"@last")[:-1], Dedup(), msg="a first occurrence at the open end") == [0, 2]


def test_only_line_two_counts(ctx):
    base = rec(b"ACGTTGCA", quals=b"IIIIIIII", hdr=b"@name", plus=b"+name")
    fq = base + rec(b"ACGTTGCA", quals=b"IIIIIIII", hdr=b"@namf", plus=b"+name") + rec(b"ACGTTGCA", quals=b"IIIIIIII", hdr=b"@name", plus=b"+namf") + \
        rec(b"ACGTTGCA", quals=b"IIIIIII#", hdr=b"@name", plus=b"+name") + rec(b"ACGTTGCC", quals=b"IIIIIIII", hdr=b"@name", plus=b"+name")
    assert check(ctx, fq, Dedup(), msg="a byte of line 1, 3 or 4 differs") == [0, 4]


# ---- key borders ---------------------------------------------------------------------------------------------------------------------

def one_byte_apart(lengths, seed, shifted):
    """per length L: a key, then per position the key with that byte changed (all distinct), then a copy of each, some in lower case;
    shifted: the names grow and shrink so that the base lines begin at every offset mod 16"""
    rng = np.random.default_rng(seed)
    out, i = [], 0
    for L in lengths:
        k = bytearray(bases(rng, L))
        firsts = [bytes(k)]
        for p in range(L):
            v = bytearray(k)
            v[p] = b"ACGT"[(b"ACGT".index(bytes([k[p]])) + 1 + p % 3) % 4]
            firsts.append(bytes(v))
        for again in (False, True):
            for j, v in enumerate(firsts):
                i += 1
                hdr = b"@" + b"x" * ((i * 7 + j) % 16 if shifted else 2)
                out.append(rec(v.lower() if again and j % 2 else v, hdr=hdr))
    return b"".join(out)


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("lengths", [range(1, 41), range(120, 137)])
def test_keys_one_byte_apart(ctx, lengths, shifted):
    fq = one_byte_apart(lengths, 5, shifted)
    kept = check(ctx, fq, Dedup(), offs=(5, 0) if shifted else (0, 0), msg="one byte apart")
    assert len(kept) == sum(L + 1 for L in lengths) and 2 * len(kept) == len(records(fq))


# ---- collisions ----------------------------------------------------------------------------------------------------------------------

def test_probe_collisions(ctx):
    """30 000 keys in a table of 2^17 slots: probe sequences of thousands of keys run into one another"""
    rng = np.random.default_rng(11)
    keys = list({bases(rng, int(rng.integers(12, 21))) for _ in range(30000)})
    order = list(range(len(keys))) + [int(x) for x in rng.integers(0, len(keys) // 3, 10000)]
    rng.shuffle(order)
    fq = b"".join(rec(keys[k], hdr=b"@%d" % i) for i, k in enumerate(order))
    kept = check(ctx, fq, Dedup(), msg="random keys and repeats")
    assert len(kept) == len(keys)


@pytest.mark.parametrize("K", [1, 2, 64, 1000])
def test_a_set_filled_to_its_last_key(dset, K):
    ctx = dset
    rng = np.random.default_rng(K)
    keys = list({bases(rng, 16) for _ in range(K + 10)})[:K + 1]
    ctx.dedup_set_create(K, 16 * K, 0)
    seen = {}
    d = Dedup(use_set=True)
    cuts = sorted({0, K // 3, K // 2, K})
    for a, b in zip(cuts, cuts[1:]):
        fq = b"".join(rec(k) for k in keys[a:b]) + b"".join(rec(k.lower()) for k in keys[:b:3])
        check(ctx, fq, d, seen=seen, msg="keys %d..%d of %d" % (a, b, K))
    assert ctx.dedup_set_info() == (K, 16 * K, K, 16 * K)
    whole = b"".join(rec(k) for k in keys[:K])
    assert check(ctx, whole, d, seen=seen, msg="a full set, every key known") == []
    assert "1 keys" in refused(ctx, E_NOMEM, whole + rec(keys[K]), d)
    assert check(ctx, rec(keys[0]) + b"".join(rec(k.lower()) for k in keys[:K]), d, seen=seen, msg="after the refusal") == []


# ---- contention and order ------------------------------------------------------------------------------------------------------------

def test_one_key_everywhere(ctx):
    fq = b"".join(rec(b"ACGTACGTAC", hdr=b"@%d" % i) for i in range(70000))
    T, out = Buf(len(fq), 0, fq), Buf(64, 0)
    for _ in range(2):
        n, rep = ctx.dedup_records(T.ptr, len(fq), Dedup(), out.ptr, out.n)
        assert out.back("the output")[:n] == rec(b"ACGTACGTAC", hdr=b"@0")
        assert (rep.n_units, rep.n_kept, rep.n_dup_call, rep.n_dup_set) == (70000, 1, 69999, 0)


def test_the_first_occurrence_wins(ctx):
    rng = np.random.default_rng(3)
    hot = bases(rng, 33)
    which = set(int(x) for x in rng.choice(np.arange(100, 20000), 5000, replace=False))
    fq = b"".join(rec(hot if i in which else bases(rng, 33), hdr=b"@%d" % i) for i in range(20000))
    kept = check(ctx, fq, Dedup(), msg="one key 5000 times")
    assert min(which) in kept and len(which & set(kept)) == 1
    assert check(ctx, fq, Dedup(), offs=(9, 2), msg="again") == kept


# ---- pairs ---------------------------------------------------------------------------------------------------------------------------

def test_pairs(ctx):
    X, Y = b"ACGTAC", b"GGTTA"
    pair = lambda x, y: rec(x, hdr=b"@p/1") + rec(y, hdr=b"@p/2")
    d = Dedup(pairs=1)
    assert check(ctx, pair(X, Y) + pair(Y, X) + pair(X, Y), d, msg="(X,Y) against (Y,X)") == [0, 1, 2, 3]
    assert check(ctx, pair(X, Y) + pair(X, X) + pair(Y, Y) + pair(X.lower(), Y), d, msg="the same X, another Y") == [0, 1, 2, 3, 4, 5]
    assert check(ctx, pair(b"AC", b"G") + pair(b"A", b"CG") + pair(b"ACG", b"") + pair(b"", b"ACG") + pair(b"ac", b"g"), d, msg="where X ends") == list(range(8))
    assert check(ctx, pair(b"", b"") + pair(b"", b""), d, msg="empty mates") == [0, 1]
    # as records every mate here has been seen before; as pairs only the last pair has
    fq = pair(X, Y) + pair(Y, X) + pair(X, X) + pair(Y, X)
    assert check(ctx, fq, d, msg="pairs") == list(range(6)) and check(ctx, fq, Dedup(), msg="the same text as records") == [0, 1]
    refused(ctx, E_FORMAT, fq + rec(X), d)
    refused(ctx, E_FORMAT, fq, Dedup(pairs=1, n_records=3))
    assert check(ctx, fq + rec(X), Dedup(pairs=1, first_record=2, n_records=6), msg="an even range of an odd text") == [2, 3, 4, 5]
    rng = np.random.default_rng(8)
    ks = [bases(rng, int(rng.integers(0, 70))) for _ in range(40)]
    fq = b"".join(pair(ks[int(a)], ks[int(b)]) for a, b in rng.integers(0, 40, (3000, 2)))
    assert 2 * 1000 < len(check(ctx, fq, d, offs=(3, 11), msg="3000 pairs of 40 keys")) <= 2 * 1600


# ---- the range -----------------------------------------------------------------------------------------------------------------------

def test_a_range_of_records(dset):
    ctx = dset
    rng = np.random.default_rng(9)
    ks = [bases(rng, 25) for _ in range(60)]
    fq = b"".join(rec(ks[int(k)], hdr=b"@%d" % i) for i, k in enumerate(rng.integers(0, 60, 400)))
    for a, n in ((0, 400), (1, 399), (100, 200), (399, 1), (37, None)):
        kept = check(ctx, fq, Dedup(first_record=a, n_records=n), msg="records %d..+%s" % (a, n))
        assert kept[0] == a                                           # a record seen in front of the range is no earlier unit
    # records outside the range never enter the set: a following call keeps what only they held
    ctx.dedup_set_create(100, 4000, 0)
    seen = {}
    first = check(ctx, fq, Dedup(first_record=100, n_records=50, use_set=True), seen=seen, msg="into the set")
    assert 0 < len(seen) < 60 and len(first) == len(seen)
    rest = check(ctx, fq, Dedup(use_set=True), seen=seen, msg="the whole text behind it")
    assert len(first) + len(rest) == len(seen) == 60 and not set(first) & set(rest)


# ---- placement -----------------------------------------------------------------------------------------------------------------------

def test_text_and_output_anywhere(ctx):
    rng = np.random.default_rng(2)
    ks = [bases(rng, int(rng.integers(1, 50))) for _ in range(30)]
    fq = b"".join(rec(ks[int(k)]) for k in rng.integers(0, 30, 90))
    for off in range(16):
        check(ctx, fq, Dedup(), offs=(off, (5 * off + 3) % 16), msg="placement", slack=off)
        check(ctx, fq[:-1], Dedup(), offs=((3 * off + 1) % 16, off), msg="placement, an open end", slack=1)


# ---- the set -------------------------------------------------------------------------------------------------------------------------

def duplicated_text(seed, n=900, nkeys=300, lo=0, hi=90):
    rng = np.random.default_rng(seed)
    ks = [bases(rng, int(rng.integers(lo, hi))) for _ in range(nkeys)]
    return [rec(ks[int(k)], hdr=b"@%d" % i) for i, k in enumerate(rng.integers(0, nkeys, n))]


@pytest.mark.parametrize("pairs", [0, 1])
def test_calls_that_share_the_set_are_one_call(dset, pairs):
    ctx = dset
    rs = duplicated_text(21, nkeys=300 if not pairs else 25)
    fq = b"".join(rs)
    whole = check(ctx, fq, Dedup(pairs=pairs), msg="stateless")
    assert len(whole) < len(rs)
    ctx.dedup_set_create(1000, 90 * 1000, pairs)
    for cuts in ((300, 600), (2, 898), (450, 452), (100, 100)):
        ctx.dedup_set_clear()
        assert ctx.dedup_set_info() == (0, 0, 1000, 90 * 1000)
        seen, got = {}, []
        for a, b in zip((0,) + cuts, cuts + (len(rs),)):
            if a == b:
                continue
            got += [a + r for r in check(ctx, b"".join(rs[a:b]), Dedup(pairs=pairs, use_set=True), seen=seen, msg="part %d..%d" % (a, b))]
        assert got == whole
    T, out = Buf(len(fq), 0, fq), Buf(len(fq), 0)
    rep = ctx.dedup_records(T.ptr, len(fq), Dedup(pairs=pairs, use_set=True), out.ptr, len(fq))[1]
    assert (rep.n_kept, rep.n_dup_call, rep.n_dup_set) == (0, 0, rep.n_units)


def test_a_refused_call_leaves_the_set_as_it_was(dset):
    ctx = dset
    rs = duplicated_text(22, n=600, nkeys=200, lo=10, hi=40)
    t1, t2 = b"".join(rs[:300]), b"".join(rs[300:])
    d = Dedup(use_set=True)
    _, _, _, _, k1 = distinct(t1, d, {})
    kept2, _, _, _, k2 = distinct(t2, d, k1)
    want2 = b"".join(records(t2)[r] for r in kept2)
    assert len(k2) > 10
    # room for the first part and exactly what the second part adds
    ctx.dedup_set_create(len(k1) + len(k2), key_bytes(k1) + key_bytes(k2), 0)
    seen = {}
    check(ctx, t1, d, seen=seen, msg="the first part")
    refused(ctx, E_OVERFLOW, t2, d, cap=len(want2) - 1, needs=len(want2))
    refused(ctx, E_FORMAT, t2 + b"extra\n", d)
    refused(ctx, E_ARG, t2, Dedup(use_set=True, first_record=250, n_records=100))
    assert check(ctx, t2, d, seen=dict(seen), msg="what the second part would have given") == kept2
    assert ctx.dedup_set_info()[:2] == (len(k1) + len(k2), key_bytes(k1) + key_bytes(k2))
    # one key more than fits; one byte more than fits
    for dk, db in ((-1, 0), (0, -1)):
        ctx.dedup_set_destroy()
        ctx.dedup_set_create(len(k1) + len(k2) + dk, key_bytes(k1) + key_bytes(k2) + db, 0)
        seen = {}
        check(ctx, t1, d, seen=seen, msg="the first part")
        said = refused(ctx, E_NOMEM, t2, d)
        assert "%d keys of %d bytes" % (len(k2), key_bytes(k2)) in said and "%d keys and %d bytes are free" % (len(k2) + dk, key_bytes(k2) + db) in said
        # without one of its new keys (ten bytes at least) the text fits
        gone = key(records(t2)[max(k2.values())])
        short = b"".join(r for r in records(t2) if key(r) != gone)
        check(ctx, short, d, seen=seen, msg="one key fewer")


def test_the_set_entries(dset):
    ctx = dset
    fq = b"".join(duplicated_text(23, n=50, nkeys=20))
    assert ctx.dedup_set_info() is None
    refused(ctx, E_ARG, fq, Dedup(use_set=True))                      # no set
    for bad in ((0, 10, 0), (10, 0, 0), (10, 10, 2), (1 << 39, 10, 0), (10, 1 << 46, 0), (10, TO_END, 0), (10, TO_END - 30, 0)):
        with pytest.raises(capi.SfqError) as e:
            ctx.dedup_set_create(*bad)
        assert e.value.code == E_ARG and ctx.dedup_set_info() is None
    with pytest.raises(capi.SfqError) as e:
        ctx.dedup_set_clear()
    assert e.value.code == E_ARG
    ctx.dedup_set_create(50, 5000, 1)
    with pytest.raises(capi.SfqError) as e:
        ctx.dedup_set_create(50, 5000, 1)                             # a second one
    assert e.value.code == E_ARG and ctx.dedup_set_info() == (0, 0, 50, 5000)
    refused(ctx, E_ARG, fq, Dedup(use_set=True))                      # a set of pairs, a rule of records
    seen = {}
    check(ctx, fq, Dedup(use_set=True, pairs=1), seen=seen, msg="pairs into a set of pairs")
    assert len(seen) > 0
    check(ctx, fq, Dedup(), msg="a stateless call beside the set")
    assert ctx.dedup_set_info()[0] == len(seen)
    ctx.dedup_set_clear()
    assert ctx.dedup_set_info() == (0, 0, 50, 5000)
    assert len(check(ctx, fq, Dedup(use_set=True, pairs=1), seen={}, msg="after clear")) == 2 * len(seen)
    ctx.dedup_set_destroy()
    ctx.dedup_set_destroy()
    assert ctx.dedup_set_info() is None
    ctx.dedup_set_create(50, 5000, 0)
    check(ctx, fq, Dedup(use_set=True), seen={}, msg="a new set of records")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    rs = duplicated_text(24, n=200, nkeys=150, lo=20, hi=40)
    fq = b"".join(rs)
    refused(ctx, E_FORMAT, fq + b"extra\n", Dedup())
    refused(ctx, E_FORMAT, fq + b"a\nb\n", Dedup())
    refused(ctx, E_ARG, b"", Dedup())
    for bad in (Dedup(n_records=0), Dedup(pairs=2), Dedup(pairs=1, first_record=1)):
        assert capi.dedup_check(bad) == E_ARG
        refused(ctx, E_ARG, fq, bad)
    for a, n in ((200, None), (201, None), (0, 201), (200, 1), (150, 51), (1 << 63, 1 << 63)):
        refused(ctx, E_ARG, fq, Dedup(first_record=a, n_records=n))
    L = capi.lib()
    n64 = capi.C.c_uint64()
    T, out = Buf(len(fq), 0, fq), Buf(len(fq), 0)
    for args in ((None, len(fq), capi.C.byref(Dedup()), out.ptr, len(fq), capi.C.byref(n64), None),
                 (T.ptr, len(fq), None, out.ptr, len(fq), capi.C.byref(n64), None),
                 (T.ptr, len(fq), capi.C.byref(Dedup()), None, len(fq), capi.C.byref(n64), None),
                 (T.ptr, len(fq), capi.C.byref(Dedup()), out.ptr, len(fq), None, None)):
        assert L.sfq_dedup_records(ctx._h, *args) == E_ARG
    kept = distinct(fq, Dedup())[0]
    want = b"".join(rs[r] for r in kept)
    assert 0 < len(kept) < 200
    refused(ctx, E_OVERFLOW, fq, Dedup(), cap=len(want) - 1, needs=len(want))
    refused(ctx, E_OVERFLOW, fq, Dedup(), cap=0, needs=len(want))
    out = Buf(len(want), 0)                                           # ... and with exactly that size it succeeds
    assert ctx.dedup_records(T.ptr, len(fq), Dedup(), out.ptr, len(want))[0] == len(want)
    assert out.back("an output of exactly the size needed") == want
    check(ctx, fq, Dedup(), msg="after the refusals")


def test_a_record_of_4_gib_is_refused(dset):
    """The text is built on the device: one record of 4 GiB of bases; then two records of 2 GiB of bases each, which are refused as a
    pair alone (their keys together hold 4 GiB) -- and before a key of that size is read: the call returns at once."""
    import torch
    ctx = dset
    L = 1 << 32
    t = torch.full((L + 64,), ord("A"), dtype=torch.uint8, device="cuda")
    base = (-t.data_ptr()) % 16

    def put(at, b):
        t[base + at:base + at + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()

    def call(n, d, cap=64):
        out = Buf(64, 0)
        with pytest.raises(capi.SfqError) as e:
            ctx.dedup_records(t.data_ptr() + base, n, d, out.ptr, cap)
        assert out.back("the output of a refused call") == b"I" * 64
        return e.value

    put(0, b"@\n")
    put(2 + L, b"\n+\n\n")
    assert call(2 + L + 4, Dedup()).code == E_UNSUPPORTED
    t.fill_(ord("A"))
    H = L // 2
    put(0, b"@\n")
    put(2 + H, b"\n+\n\n@\n")
    put(8 + 2 * H, b"\n+\n\n")
    ctx.dedup_set_create(4, 64, 1)
    for d in (Dedup(pairs=1), Dedup(pairs=1, use_set=True)):
        assert call(12 + 2 * H, d).code == E_UNSUPPORTED
    assert ctx.dedup_set_info()[:2] == (0, 0)

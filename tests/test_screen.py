"""Screened records on the GPU (scr.hip, slimfastq_amd.h "screened records"): sfq_screen_records and the set's entries against the
restatement of the header's rule in screen_rule.py -- canonical k-mers as Python integers in a Python set, built independently of
the C code.  Every comparison is exact.  Every output is filled with a marker: a call writes its result and nothing else, a refused
call nothing at all.  The report of a text of ONE record gives that record's H and W, which is how they are pinned per record."""
import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Screen
from screen_rule import TO_END, canon, windows, kmer_set, home_slot, slots_of, records, hw, screen
from test_pairs import Buf, first_difference

pytestmark = pytest.mark.gpu
E_ARG, E_NOMEM, E_FORMAT, E_OVERFLOW, E_UNSUPPORTED = -1, -3, -4, -5, -7
ACGT = np.frombuffer(b"ACGT", np.uint8)
PIECE = 4 << 20                                                        # sfq_screen_set_add's piece (slimfastq_amd.h states it)
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return s.translate(COMP)[::-1]


def bases(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def rec(b, quals=None, hdr=b"@r", plus=b"+"):
    return hdr + b"\n" + b + b"\n" + plus + b"\n" + (b"I" * len(b) if quals is None else quals) + b"\n"


@pytest.fixture
def sctx(ctx):
    """The session's context without a set, before and after."""
    ctx.screen_set_destroy()
    try:
        yield ctx
    finally:
        ctx.screen_set_destroy()


def new_set(ctx, k, max_kmers, *texts):
    """a fresh set of the texts' k-mers on the context; returns the same set in Python"""
    ctx.screen_set_destroy()
    ctx.screen_set_create(k, max_kmers)
    for t in texts:
        ctx.screen_set_add(t)
    kset = kmer_set(k, *texts)
    assert ctx.screen_set_info() == (k, len(kset), max_kmers)
    return kset


def check(ctx, fq, rule, k, kset, offs=(0, 0), msg="", slack=37):
    """sfq_screen_records against the rule; returns the kept records' numbers and the report"""
    rs = records(fq)
    kept, units, nm, sw, sh = screen(fq, rule, k, kset)
    want = b"".join(rs[r] for r in kept)
    T, out = Buf(len(fq), offs[0], fq), Buf(len(want) + slack, offs[1])
    n, rep = ctx.screen_records(T.ptr, len(fq), rule, out.ptr, out.n)
    got = out.back("the output")
    assert T.back("the text") == fq, "the text was written"
    what = "%s, k %d, offsets %s" % (msg, k, offs)
    assert n == len(want), (what, n, len(want))
    first_difference(got[:n], want, what)
    assert got[n:] == b"I" * (out.n - n), what + ": bytes behind the result were written"
    G = 2 if rule.pairs else 1
    assert (rep.n_in_range, rep.n_units, rep.n_kept, rep.n_matched_records, rep.n_windows, rep.n_hits, rep.text_bytes, rep.kept_bytes, rep.set_kmers) == \
        (units * G, units, len(kept) // G, nm, sw, sh, len(fq), len(want), len(kset)), what
    assert ctx.screen_set_info()[1] == len(kset), what + ": a screening call changed the set"
    return kept, rep


def gpu_hw(ctx, record, off=0):
    """(H, W) of one record: the report of a text that holds it alone"""
    T, out = Buf(len(record), off, record), Buf(len(record), 0)
    rep = ctx.screen_records(T.ptr, len(record), Screen(), out.ptr, out.n)[1]
    return rep.n_hits, rep.n_windows


def refused(ctx, code, fq, rule, cap=None, needs=None):
    T, out = Buf(max(len(fq), 1), 3, fq if fq else None), Buf(max(len(fq), 1) + 16, 5)
    before = ctx.screen_set_info()
    with pytest.raises(capi.SfqError) as e:
        ctx.screen_records(T.ptr, len(fq), rule, out.ptr, out.n if cap is None else cap)
    assert e.value.code == code, str(e.value)
    assert out.back("the output of a refused call") == b"I" * out.n, "a refused call wrote to its output"
    if fq:
        assert T.back("the text") == fq
    if needs is not None:
        assert e.value.needed == needs
    assert ctx.screen_set_info() == before
    return str(e.value)


# ---- lengths and k ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 5, 16, 27, 31])
def test_line_lengths(sctx, k):
    ctx = sctx
    rng = np.random.default_rng(k)
    lengths = [0, k - 1, k, k + 1, 63, 64, 65, 150, 1000, 5000]
    reads = [bases(rng, L) for L in lengths]
    # the reference: stretches of every read, some as they are, some as the other strand, one in lower case
    ref = b"\n".join([reads[2], revcomp(reads[3]), reads[4][10:50], revcomp(reads[6])[5:60].lower(), reads[7][:80], reads[8][300:700],
                      revcomp(reads[9][:2500]), reads[9][4000:]])
    kset = new_set(ctx, k, len(ref), ref)
    for i, (L, b) in enumerate(zip(lengths, reads)):
        r = rec(b, hdr=b"@" + b"h" * i)
        H, W = hw(r, k, kset)
        assert W == max(0, L - k + 1)
        assert gpu_hw(ctx, r, off=i) == (H, W), "a line of %d bases" % L
    fq = b"".join(rec(b, hdr=b"@%d" % i) for i, b in enumerate(reads))
    for keep in (False, True):
        kept, _ = check(ctx, fq, Screen(keep_matched=keep), k, kset, msg="ten lengths")
        assert 0 < len(kept) < len(reads)
        check(ctx, fq[:-1], Screen(keep_matched=keep, min_hits=3, min_pct=50), k, kset, offs=(7, 3), msg="ten lengths, an open end")


@pytest.mark.parametrize("k,pal", [(4, b"ACGT"), (4, b"AATT"), (16, b"ACGTACGTACGTACGT"), (16, b"AAAACCCCGGGGTTTT")])
def test_palindromes(sctx, k, pal):
    assert revcomp(pal) == pal
    kset = new_set(sctx, k, 8, pal)
    assert len(kset) == 1                                              # one window, one k-mer
    read = pal + b"A" + pal.lower() + b"C"
    H, W = hw(rec(read), k, kset)
    assert H >= 2
    assert gpu_hw(sctx, rec(read)) == (H, W)


# ---- breaks, case, strands -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 31])
def test_a_break_at_every_position(sctx, k):
    ctx = sctx
    rng = np.random.default_rng(100 + k)
    read = bases(rng, 2 * k)
    kset = new_set(ctx, k, 4 * k, read)
    assert gpu_hw(ctx, rec(read)) == (k + 1, k + 1)
    for brk in (b"N", b"n", b".", b"\r"):
        broken = [read[:p] + brk + read[p + 1:] for p in range(2 * k)]
        for p, b in enumerate(broken):
            want = max(0, p - k + 1) + max(0, 2 * k - 1 - p - k + 1)   # the windows left of the break and right of it
            assert hw(rec(b), k, kset) == (want, want)
            assert gpu_hw(ctx, rec(b, hdr=b"@" + b"x" * (p % 9)), off=p % 16) == (want, want), "a %r at %d" % (brk, p)
        check(ctx, b"".join(rec(b) for b in broken), Screen(min_hits=k // 2), k, kset, msg="breaks")


def test_lower_case_and_the_other_strand(sctx):
    ctx, k = sctx, 27
    rng = np.random.default_rng(5)
    a, b, c = bases(rng, 90), bases(rng, 90), bases(rng, 90)
    kset = new_set(ctx, k, 300, a.lower() + b"\n" + revcomp(b))       # a in lower case; of b only the reverse complement
    fq = rec(a) + rec(a.lower()) + rec(revcomp(a)) + rec(b) + rec(b.lower()) + rec(revcomp(b).lower()) + rec(c) + rec(a[:50] + c[:40])
    for r in records(fq)[:6]:
        assert gpu_hw(ctx, r) == (64, 64)
    assert gpu_hw(ctx, rec(c)) == (0, 64)
    assert gpu_hw(ctx, rec(a[:50] + c[:40])) == (24, 64)
    assert check(ctx, fq, Screen(), k, kset, msg="case and strands")[0] == [6]
    assert check(ctx, fq, Screen(keep_matched=True, min_pct=50), k, kset, msg="case and strands")[0] == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("k,hdr", [(27, 3), (5, 8), (16, 14)])
def test_one_kmer_of_the_read_at_every_position(sctx, k, hdr):
    """A set that holds the k-mer at position p of a read of 200 bases alone: H is the number of positions with that canonical value,
    for EVERY p -- a lane that warms up wrongly at the border of its stretch loses or doubles one of them."""
    ctx = sctx
    rng = np.random.default_rng(k)
    read = bases(rng, 200)
    r = rec(read, hdr=b"@" + b"h" * hdr)
    vals = windows(read, k)
    T, out = Buf(len(r), 0, r), Buf(len(r), 0)
    ctx.screen_set_create(k, 4)
    for p in range(200 - k + 1):
        ctx.screen_set_clear()
        ctx.screen_set_add(read[p:p + k])
        rep = ctx.screen_records(T.ptr, len(r), Screen(), out.ptr, out.n)[1]
        assert (rep.n_hits, rep.n_windows, rep.set_kmers) == (vals.count(vals[p]), len(vals), 1), "the k-mer at %d" % p


# ---- placement -------------------------------------------------------------------------------------------------------------------

def test_text_and_lines_anywhere(sctx):
    ctx, k = sctx, 16
    rng = np.random.default_rng(2)
    reads = [bases(rng, int(rng.integers(10, 80))) for _ in range(32)]
    ref = b"\n".join(reads[::3])
    kset = new_set(ctx, k, len(ref), ref)
    # the names grow by a byte a record: the base lines begin at every offset mod 16
    fq = b"".join(rec(b, hdr=b"@" + b"x" * (i % 17)) for i, b in enumerate(reads))
    for off in range(16):
        check(ctx, fq, Screen(), k, kset, offs=(off, (5 * off + 3) % 16), msg="placement", slack=off)
        check(ctx, fq[:-1], Screen(keep_matched=True), k, kset, offs=((3 * off + 1) % 16, off), msg="placement, an open end", slack=1)
    for i, b in enumerate(reads):
        r = rec(b, hdr=b"@" + b"x" * (i % 17))
        assert gpu_hw(ctx, r, off=i % 16) == hw(r, k, kset)


# ---- the thresholds ----------------------------------------------------------------------------------------------------------------

def test_min_hits_and_min_pct_at_their_boundaries(sctx):
    ctx, k = sctx, 27
    rng = np.random.default_rng(6)
    read = bases(rng, k + 99)
    kset = new_set(ctx, k, 200, read[:k + 24])
    r = rec(read)
    assert hw(r, k, kset) == (25, 100)
    other = rec(bases(rng, 60))
    assert hw(other, k, kset)[0] == 0
    fq = other + r + other
    for hits in range(1, 27):
        assert check(ctx, fq, Screen(min_hits=hits), k, kset, msg="min_hits %d" % hits)[0] == ([0, 2] if hits <= 25 else [0, 1, 2])
    for pct in (0, 1, 24, 25, 26, 100):                                # 100 H = 25 W exactly
        assert check(ctx, fq, Screen(min_pct=pct), k, kset, msg="min_pct %d" % pct)[0] == ([0, 2] if pct <= 25 else [0, 1, 2])
    assert check(ctx, fq, Screen(min_hits=25, min_pct=25, keep_matched=True), k, kset, msg="both at the boundary")[0] == [1]
    assert check(ctx, fq, Screen(min_hits=26, min_pct=25, keep_matched=True), k, kset, msg="one hit short")[0] == []
    # a read without a window is never matched, whatever min_pct says: 100 * 0 >= 0 * 0 holds, min_hits does not
    short = rec(b"ACGT") + rec(b"") + rec(b"N" * 40)
    assert check(ctx, short, Screen(min_pct=0), k, kset, msg="no window")[0] == [0, 1, 2]
    n, rep = check(ctx, short, Screen(keep_matched=True), k, kset, msg="no window, keep")
    assert n == [] and rep.kept_bytes == 0


# ---- pairs and ranges ------------------------------------------------------------------------------------------------------------

def test_pairs_and_ranges(sctx):
    ctx, k = sctx, 16
    rng = np.random.default_rng(7)
    hit, miss = bases(rng, 70), [bases(rng, 70) for _ in range(40)]
    kset = new_set(ctx, k, 100, hit)
    m = lambda i: rec(hit[i % 20:i % 20 + 40], hdr=b"@m%d" % i)
    u = lambda i: rec(miss[i], hdr=b"@u%d" % i)
    fq = u(0) + u(1) + m(2) + u(3) + u(4) + m(5) + m(6) + m(7) + u(8) + u(9)      # pairs: neither, first, second, both, neither
    assert check(ctx, fq, Screen(), k, kset, msg="records")[0] == [0, 1, 3, 4, 8, 9]
    assert check(ctx, fq, Screen(pairs=1), k, kset, msg="either mate")[0] == [0, 1, 8, 9]
    assert check(ctx, fq, Screen(pairs=2), k, kset, msg="both mates")[0] == [0, 1, 2, 3, 4, 5, 8, 9]
    assert check(ctx, fq, Screen(pairs=1, keep_matched=True), k, kset, msg="either mate, kept")[0] == [2, 3, 4, 5, 6, 7]
    assert check(ctx, fq, Screen(pairs=2, keep_matched=True), k, kset, msg="both mates, kept")[0] == [6, 7]
    assert check(ctx, fq, Screen(first_record=2, n_records=4, pairs=1), k, kset, msg="a range of pairs")[0] == []
    assert check(ctx, fq, Screen(first_record=6, n_records=4, pairs=2), k, kset, msg="a range of pairs")[0] == [8, 9]
    refused(ctx, E_FORMAT, fq + u(10), Screen(pairs=1))
    refused(ctx, E_FORMAT, fq, Screen(pairs=2, n_records=3))
    assert check(ctx, fq + u(10), Screen(pairs=1, first_record=2, n_records=8), k, kset, msg="an even range of an odd text")[0] == [8, 9]
    for a, n in ((0, 10), (1, 9), (3, 4), (9, 1), (5, None), (5, 3)):
        kept, rep = check(ctx, fq, Screen(first_record=a, n_records=n), k, kset, msg="records %d..+%s" % (a, n))
        check(ctx, fq, Screen(first_record=a, n_records=n, keep_matched=True), k, kset, msg="records %d..+%s, kept" % (a, n))
    # nothing kept: SFQ_OK, 0 bytes, nothing written (check() looks at every byte of the output)
    kept, rep = check(ctx, fq, Screen(first_record=5, n_records=3), k, kset, msg="nothing kept")
    assert kept == [] and (rep.kept_bytes, rep.n_kept, rep.n_units, rep.n_matched_records) == (0, 0, 3, 3)
    many = b"".join(m(i) if rng.integers(0, 3) == 0 else rec(bases(rng, int(rng.integers(0, 120))), hdr=b"@%d" % i) for i in range(3000))
    for pairs in (0, 1, 2):
        check(ctx, many, Screen(pairs=pairs, min_hits=2), k, kset, offs=(3, 11), msg="3000 records, pairs %d" % pairs)


# ---- the set ---------------------------------------------------------------------------------------------------------------------

def test_all_canonical_4_mers(sctx):
    ctx = sctx
    every = [bytes(b"ACGT"[(i >> s) & 3] for s in (6, 4, 2, 0)) for i in range(256)]
    assert len({canon(w) for w in every}) == 136
    text = b"\n".join(every)
    kset = new_set(ctx, 4, 136, text)
    assert len(kset) == 136
    fq = b"".join(rec(w) for w in every[::5])
    assert check(ctx, fq, Screen(), 4, kset, msg="every 4-mer is known")[0] == []
    ctx.screen_set_add(text)                                           # the same sequences again: a set
    assert ctx.screen_set_info() == (4, 136, 136)
    ctx.screen_set_destroy()
    ctx.screen_set_create(4, 135)
    with pytest.raises(capi.SfqError) as e:
        ctx.screen_set_add(text)
    assert e.value.code == E_NOMEM
    assert ctx.screen_set_info() == (4, 0, 135)                        # a refused add leaves the set EMPTY
    assert check(ctx, fq, Screen(keep_matched=True), 4, set(), msg="an emptied set")[0] == []
    kset = kmer_set(4, b"\n".join(every[:100]))
    assert len(kset) <= 135
    ctx.screen_set_add(b"\n".join(every[:100]))                        # ... and takes what fits afterwards
    assert ctx.screen_set_info() == (4, len(kset), 135)
    check(ctx, fq, Screen(), 4, kset, msg="after the refusal")


def test_kmers_that_share_a_home_slot(sctx):
    """The documented table: a k-mer's home slot is the top bits of value * 0x9E3779B97F4A7C15.  40 k-mers of ONE home slot in a table
    of 128 slots probe through one another; others of that slot, not in the set, walk the whole run and must miss."""
    ctx, k, max_kmers = sctx, 16, 64
    slots = slots_of(max_kmers)
    assert slots == 128
    rng = np.random.default_rng(12)
    cands = list({bases(rng, k) for _ in range(12000)})
    home = home_slot(canon(cands[0]), slots)
    same = [c for c in cands if home_slot(canon(c), slots) == home]
    assert len(same) >= 60
    inside, outside = same[:40], same[40:60]
    text = b"\n".join(inside)
    kset = new_set(ctx, k, max_kmers, text)
    assert len(kset) == 40
    fq = b"".join(rec(w if i % 3 else revcomp(w)) for i, w in enumerate(inside + outside))
    kept, rep = check(ctx, fq, Screen(), k, kset, msg="one home slot")
    assert kept == list(range(40, 60)) and rep.n_hits == 40
    # filled to exactly max_kmers, whatever the order of the inserts: the same set
    more = [c for c in cands if c not in same][:24]
    ctx.screen_set_add(b"\n".join(more[::-1]))
    kset |= kmer_set(k, *more)
    assert ctx.screen_set_info() == (k, 64, 64)
    fq = b"".join(rec(w) for w in outside + more + inside)
    assert check(ctx, fq, Screen(), k, kset, msg="a full set")[0] == list(range(20))
    with pytest.raises(capi.SfqError) as e:
        ctx.screen_set_add(outside[0])
    assert e.value.code == E_NOMEM and ctx.screen_set_info() == (k, 0, 64)


def test_several_adds_are_one_add(sctx):
    ctx, k = sctx, 27
    rng = np.random.default_rng(13)
    parts = [bases(rng, int(n)) for n in (300, 26, 27, 1000, 5, 64)]
    reads = b"".join(rec(p[:60] + q[:60]) for p in parts for q in parts)
    one = new_set(ctx, k, 4000, b"\n".join(parts))
    want = check(ctx, reads, Screen(min_hits=40), k, one, msg="one add")[0]
    many = new_set(ctx, k, 4000, *parts)
    assert many == one
    assert check(ctx, reads, Screen(min_hits=40), k, many, msg="six adds")[0] == want
    # windows never span two calls: the concatenation WITHOUT the break holds more
    glued = kmer_set(k, b"".join(parts))
    assert len(glued) > len(one)
    ctx.screen_set_clear()
    assert ctx.screen_set_info() == (k, 0, 4000)
    assert check(ctx, reads, Screen(), k, set(), msg="after clear")[0] == list(range(36))
    ctx.screen_set_add(b"".join(parts))
    assert ctx.screen_set_info() == (k, len(glued), 4000)


def test_a_sequence_text_of_more_than_one_piece(sctx):
    """The piece is a constant (4 MiB, as the header says) and no knob shrinks it, so the text is a piece and 5000 bytes: 'N' but for
    its first 500 bytes and the 15 000 around the piece's end.  The windows that cross the cut are those of the text."""
    ctx, k = sctx, 31
    rng = np.random.default_rng(14)
    text = bytearray(b"N" * (PIECE + 5000))
    text[:500] = bases(rng, 500)
    text[PIECE - 10000:] = bases(rng, 15000)
    text = bytes(text)
    assert len(text) == PIECE + 5000
    kset = kmer_set(k, text[:500], text[PIECE - 10000:])
    ctx.screen_set_create(k, 30000)
    ctx.screen_set_add(text)
    assert ctx.screen_set_info() == (k, len(kset), 30000)
    for a in range(PIECE - 70, PIECE + 10, 7):                         # reads across the cut
        assert gpu_hw(ctx, rec(text[a:a + 64])) == (34, 34)
    assert gpu_hw(ctx, rec(text[-64:])) == (34, 34) and gpu_hw(ctx, rec(text[:64])) == (34, 34)
    assert gpu_hw(ctx, rec(bases(rng, 64))) == (0, 34)
    fq = b"".join(rec(text[a:a + 100], hdr=b"@%d" % a) for a in range(PIECE - 10100, PIECE + 4900, 500))
    check(ctx, fq, Screen(min_pct=100), k, kset, msg="reads along the cut")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_the_set_entries(sctx):
    ctx = sctx
    fq = rec(b"ACGTACGTACGT") + rec(b"GGGGGGGGGGGGG")
    assert ctx.screen_set_info() is None
    refused(ctx, E_ARG, fq, Screen())                                  # no set
    for bad in ((3, 10), (32, 10), (0, 10), (27, 0), (27, 1 << 39), (27, TO_END)):
        with pytest.raises(capi.SfqError) as e:
            ctx.screen_set_create(*bad)
        assert e.value.code == E_ARG and ctx.screen_set_info() is None
    for call in (ctx.screen_set_clear, lambda: ctx.screen_set_add(b"ACGTACGT")):
        with pytest.raises(capi.SfqError) as e:
            call()
        assert e.value.code == E_ARG
    ctx.screen_set_create(5, 50)
    with pytest.raises(capi.SfqError) as e:
        ctx.screen_set_create(5, 50)                                   # a second one
    assert e.value.code == E_ARG and ctx.screen_set_info() == (5, 0, 50)
    with pytest.raises(capi.SfqError) as e:
        ctx.screen_set_add(b"")
    assert e.value.code == E_ARG
    ctx.screen_set_add(b"ACG")                                         # shorter than k: no window
    ctx.screen_set_add(b"ACGNACGT\n")
    assert ctx.screen_set_info() == (5, 0, 50)
    ctx.screen_set_add(b"ACGTA")
    assert ctx.screen_set_info() == (5, 1, 50)
    assert check(ctx, fq, Screen(), 5, kmer_set(5, b"ACGTA"), msg="one k-mer")[0] == [1]
    ctx.screen_set_destroy()
    ctx.screen_set_destroy()
    assert ctx.screen_set_info() is None


def test_refusals(sctx):
    ctx, k = sctx, 16
    rng = np.random.default_rng(24)
    ref = bases(rng, 400)
    kset = new_set(ctx, k, 400, ref)
    rs = [rec(ref[i:i + 50] if i % 3 == 0 else bases(rng, 30 + i % 20), hdr=b"@%d" % i) for i in range(200)]
    fq = b"".join(rs)
    refused(ctx, E_FORMAT, fq + b"extra\n", Screen())
    refused(ctx, E_FORMAT, fq + b"a\nb\n", Screen())
    refused(ctx, E_ARG, b"", Screen())
    for bad in (Screen(n_records=0), Screen(pairs=3), Screen(pairs=1, first_record=1), Screen(min_hits=0), Screen(min_pct=101)):
        assert capi.screen_check(bad) == E_ARG
        refused(ctx, E_ARG, fq, bad)
    for a, n in ((200, None), (201, None), (0, 201), (200, 1), (150, 51), (1 << 63, 1 << 63)):
        refused(ctx, E_ARG, fq, Screen(first_record=a, n_records=n))
    L = capi.lib()
    n64 = capi.C.c_uint64()
    T, out = Buf(len(fq), 0, fq), Buf(len(fq), 0)
    for args in ((None, len(fq), capi.C.byref(Screen()), out.ptr, len(fq), capi.C.byref(n64), None),
                 (T.ptr, len(fq), None, out.ptr, len(fq), capi.C.byref(n64), None),
                 (T.ptr, len(fq), capi.C.byref(Screen()), None, len(fq), capi.C.byref(n64), None),
                 (T.ptr, len(fq), capi.C.byref(Screen()), out.ptr, len(fq), None, None)):
        assert L.sfq_screen_records(ctx._h, *args) == E_ARG
    kept = screen(fq, Screen(), k, kset)[0]
    want = b"".join(rs[r] for r in kept)
    assert 0 < len(kept) < 200
    refused(ctx, E_OVERFLOW, fq, Screen(), cap=len(want) - 1, needs=len(want))
    refused(ctx, E_OVERFLOW, fq, Screen(), cap=0, needs=len(want))
    out = Buf(len(want), 0)                                            # ... and with exactly that size it succeeds
    assert ctx.screen_records(T.ptr, len(fq), Screen(), out.ptr, len(want))[0] == len(want)
    assert out.back("an output of exactly the size needed") == want
    check(ctx, fq, Screen(), k, kset, msg="after the refusals")


def test_a_record_of_4_gib_is_refused(sctx):
    """The text is built on the device: one record of 4 GiB of bases.  It is refused before its line is walked: the call returns at once."""
    import torch
    ctx = sctx
    ctx.screen_set_create(27, 100)
    ctx.screen_set_add(b"A" * 40)
    L = 1 << 32
    t = torch.full((L + 64,), ord("A"), dtype=torch.uint8, device="cuda")
    base = (-t.data_ptr()) % 16

    def put(at, b):
        t[base + at:base + at + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()

    put(0, b"@\n")
    put(2 + L, b"\n+\n\n")
    out = Buf(64, 0)
    with pytest.raises(capi.SfqError) as e:
        ctx.screen_records(t.data_ptr() + base, 2 + L + 4, Screen(), out.ptr, 64)
    assert e.value.code == E_UNSUPPORTED
    assert out.back("the output of a refused call") == b"I" * 64
    assert ctx.screen_set_info() == (27, 1, 100)

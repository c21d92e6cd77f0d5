"""Selected records on the GPU (sel.hip, slimfastq_amd.h "selected records"): sfq_select_records against a restatement of the header's
rule in Python over test_pairs.records(), on the smallest texts, with every term at its boundary, with motif occurrences on every
border of the kernels, in buffers at every alignment between guard bytes; the refusals; the decode switch (sfq_ctx_set_select) behind
every decoder, with checksums, the pair split and the picks.  Every comparison is exact byte equality.  Every output is filled with a
marker: a call writes its result and nothing else, a refused call nothing at all."""
import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Select
from test_pairs import Buf, reads, record, records, first_difference

pytestmark = pytest.mark.gpu
UNIT, ROW, SPAN, WG_TILE = 16, 1024, 16 << 10, 64 << 10
E_ARG, E_FORMAT, E_OVERFLOW, E_UNSUPPORTED = -1, -4, -5, -7
OFF32, TO_END, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, (1 << 64) - 1
COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


# ---- the rule --------------------------------------------------------------------------------------------------------------------

def sample_hash(seed, i):
    h = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M64
    h ^= h >> 30; h = h * 0xBF58476D1CE4E5B9 & M64
    h ^= h >> 27; h = h * 0x94D049BB133111EB & M64
    return h ^ (h >> 31)


def fails(rec, s):
    """which of the four terms the record fails (a term that is off fails nothing)"""
    l2, l4 = rec.split(b"\n")[1], rec.split(b"\n")[3]
    f = [False] * 4
    if s.min_len != 0 or s.max_len != OFF32:
        f[0] = not s.min_len <= len(l2) <= s.max_len
    if s.max_n != OFF32:
        f[1] = l2.count(b"N") + l2.count(b"n") > s.max_n
    if s.min_mean_q_x100:
        f[2] = 100 * (sum(l4) - s.qual_base * len(l4)) < s.min_mean_q_x100 * len(l4)
    if s.motif_len:
        m, u = bytes(s.motif[:s.motif_len]), l2.upper()
        f[3] = not (m in u or (bool(s.motif_rc) and m.translate(COMPLEMENT)[::-1] in u))
    return f


def selected(fq, s):
    """(the kept records' numbers, the report's counts)"""
    rs = records(fq)
    hi = len(rs) if s.n_records == TO_END else s.first_record + s.n_records
    rng = range(s.first_record, hi)
    f = {r: fails(rs[r], s) for r in rng}
    ok = {r: (not any(f[r])) != bool(s.invert) for r in rng}
    if s.pairs:
        ok = {r: (ok[r & ~1] and ok[r | 1]) if s.pairs == 1 else (ok[r & ~1] or ok[r | 1]) for r in rng}
    shift = 1 if s.pairs else 0
    kept = [r for r in rng if ok[r] and (not s.sample or (sample_hash(s.sample_seed, (s.index_base + r) >> shift) >> 32) < s.sample)]
    return kept, [sum(f[r][i] for r in rng) for i in range(4)], len(rng)


def check(ctx, fq, s, offs=(0, 0), msg="", slack=37):
    """sfq_select_records against the rule; returns the kept records' numbers"""
    rs = records(fq)
    kept, nfail, nrange = selected(fq, s)
    want = b"".join(rs[r] for r in kept)
    T, out = Buf(len(fq), offs[0], fq), Buf(len(want) + slack, offs[1])
    n, rep = ctx.select_records(T.ptr, len(fq), s, out.ptr, out.n)
    got = out.back("the output")
    assert T.back("the text") == fq, "the text was written"
    what = "%s, offsets %s" % (msg, offs)
    assert n == len(want), (what, n, len(want))
    first_difference(got[:n], want, what)
    assert got[n:] == b"I" * (out.n - n), what + ": bytes behind the result were written"
    assert (rep.n_in_range, rep.n_kept, rep.text_bytes, rep.kept_bytes, list(rep.n_fail)) == (nrange, len(kept), len(fq), len(want), nfail), what
    return kept


def refused(ctx, code, fq, s, cap=None, needs=None):
    T, out = Buf(max(len(fq), 1), 3, fq if fq else None), Buf(max(len(fq), 1) + 16, 5)
    with pytest.raises(capi.SfqError) as e:
        ctx.select_records(T.ptr, len(fq), s, out.ptr, out.n if cap is None else cap)
    assert e.value.code == code, str(e.value)
    assert out.back("the output of a refused call") == b"I" * out.n, "a refused call wrote to its output"
    if fq:
        assert T.back("the text") == fq
    if needs is not None:
        assert e.value.needed == needs


def rec(bases, quals=None, hdr=b"@r", plus=b"+"):
    return hdr + b"\n" + bases + b"\n" + plus + b"\n" + (b"I" * len(bases) if quals is None else quals) + b"\n"


# ---- the smallest texts --------------------------------------------------------------------------------------------------------------

SMALLEST = [b"@\nA\n+\nI\n", b"@h\n\n+\n\n", b"@\nA\n+\nI"]
# every single term, once so that b"@\nA\n+\nI\n" passes and once so that it fails
SINGLE = [dict(), dict(min_len=1), dict(min_len=2), dict(max_len=1), dict(max_len=0), dict(max_n=0), dict(motif=b"A"), dict(motif=b"C"),
          dict(motif=b"T", motif_rc=True), dict(min_mean_q_x100=4000), dict(min_mean_q_x100=4001), dict(sample=1 << 31, sample_seed=1),
          dict(sample=1 << 31, sample_seed=3), dict(invert=True), dict(invert=True, min_len=2)]


@pytest.mark.parametrize("fq", SMALLEST)
def test_smallest_texts(ctx, fq):
    seen = set()
    for kw in SINGLE:
        seen.add(len(check(ctx, fq, Select(**kw), msg="%r under %r" % (fq, kw))))
    assert seen == {0, 1}
    assert sample_hash(1, 0) >> 63 != sample_hash(3, 0) >> 63          # the two seeds of SINGLE: one keeps record 0, one drops it
    check(ctx, b"@\nN\n+\nI\n" + fq, Select(max_n=0), msg="an N in front")
    check(ctx, b"@\nn\n+\nI\n" + fq, Select(max_n=0, invert=True), msg="an n in front")


# ---- each scalar term at its boundary -----------------------------------------------------------------------------------------------

def test_length_at_its_boundary(ctx):
    fq = b"".join(rec(b"A" * k) for k in (0, 1, 9, 10, 11, 19, 20, 21, 40))
    for lo, hi in ((10, OFF32), (11, OFF32), (0, 20), (0, 19), (10, 20), (10, 10), (1, 9)):
        kept = check(ctx, fq, Select(min_len=lo, max_len=hi), msg="length %d..%d" % (lo, hi))
        assert kept == [i for i, k in enumerate((0, 1, 9, 10, 11, 19, 20, 21, 40)) if lo <= k <= hi]


def test_n_count_at_its_boundary(ctx):
    bases = [b"ACGT" * 10, b"ACNT" * 10, b"AnNT" * 5 + b"ACGT" * 5, b"N" * 11 + b"A" * 20, b"n" * 10 + b"A", b"N" * 40, b"nNnNn" * 2 + b"C" * 30 + b"N"]
    fq = b"".join(rec(b) for b in bases)
    ns = [b.count(b"N") + b.count(b"n") for b in bases]
    assert ns == [0, 10, 10, 11, 10, 40, 11]
    for mx in (0, 9, 10, 11, 39, 40):
        assert check(ctx, fq, Select(max_n=mx), msg="max_n %d" % mx) == [i for i, k in enumerate(ns) if k <= mx]


def test_quality_at_its_boundary(ctx):
    # sum - 33 L = 20 L exactly; one byte lowered by 1; an empty quality line passes whatever the bound
    exact = rec(b"A" * 30, b"5" * 30)
    lower = rec(b"A" * 30, b"5" * 17 + b"4" + b"5" * 12)
    mixed = rec(b"A" * 30, b"!" * 15 + b"I" * 15)                      # (0 + 40) / 2 = 20: equality again
    empty = rec(b"", b"")
    fq = exact + lower + mixed + empty + b"@x\nACGT\n+\n" + b"~~~~"  # the last line without its '\n'
    assert check(ctx, fq, Select(min_mean_q_x100=2000), msg="mean quality 20") == [0, 2, 3, 4]
    assert check(ctx, fq, Select(min_mean_q_x100=2001), msg="mean quality 20.01") == [3, 4]
    assert check(ctx, fq, Select(min_mean_q_x100=1999), msg="mean quality 19.99") == [0, 2, 3, 4]
    assert check(ctx, fq, Select(min_mean_q_x100=1997), msg="mean quality 19.97") == [0, 2, 3, 4]      # lower: 19.9666
    assert check(ctx, fq, Select(min_mean_q_x100=1996), msg="mean quality 19.96") == [0, 1, 2, 3, 4]
    assert check(ctx, fq, Select(min_mean_q_x100=9300, qual_base=33), msg="93") == [3, 4]
    assert check(ctx, fq, Select(min_mean_q_x100=100, qual_base=126), msg="a base above every byte") == [3]
    assert check(ctx, fq, Select(min_mean_q_x100=5300, qual_base=0), msg="base 0: '5' is 53") == [0, 2, 3, 4]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_record_longer_than_a_tile(ctx, where):
    """70 000 bases: the line's sums come from many spans and several workgroups"""
    rng = np.random.default_rng(4)
    short = [record(rng, int(rng.integers(20, 60))) for _ in range(40)]
    bases = np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, 70000)].tobytes()
    long_ = rec(bases, b"I" * 70000, hdr=b"@long")
    at = {"first": 0, "middle": 20, "last": 40}[where]
    fq = b"".join(short[:at]) + long_ + b"".join(short[at:])
    nn = bases.count(b"N")
    for off in (0, 9):
        assert at in check(ctx, fq, Select(max_n=nn, min_len=70000), offs=(off, 0), msg="its N count")
        assert check(ctx, fq, Select(max_n=nn - 1, min_len=70000), offs=(off, 0), msg="one N fewer allowed") == []
        assert at in check(ctx, fq, Select(min_mean_q_x100=4000, max_len=70000), offs=(off, 3), msg="its mean quality")
    low = rec(bases, b"I" * 33333 + b"H" + b"I" * 36666, hdr=b"@long")
    fq = b"".join(short[:at]) + low + b"".join(short[at:])
    assert at not in check(ctx, fq, Select(min_mean_q_x100=4000), msg="one quality byte lowered by 1")
    assert at in check(ctx, fq, Select(min_mean_q_x100=3999), msg="... and the bound with it")


# ---- the motif ---------------------------------------------------------------------------------------------------------------------------

MOTIF32 = b"ACGGTCATTGACCGTAAGCTTGCAGGATCCAT"
assert len(MOTIF32) == 32 and MOTIF32.translate(COMPLEMENT)[::-1] not in MOTIF32 * 2


def rc(m):
    return m.translate(COMPLEMENT)[::-1]


@pytest.mark.parametrize("mlen", [1, 2, 15, 16, 17, 31, 32])
def test_motif_lengths_and_places(ctx, mlen):
    m, h = MOTIF32[:mlen], mlen // 2
    fill = b"T" * 40
    mixed = bytes(c | 0x20 if i & 1 else c for i, c in enumerate(m))
    cases = [(rec(m + fill), True),                                    # at the base line's first byte
             (rec(fill + m), True),                                    # ... at its last
             (rec(fill[:7] + m + fill), True),
             (rec(fill), False),
             (rec(fill, hdr=b"@" + m), False),                         # in the header only
             (rec(fill, hdr=b"@" + m, plus=b"+" + m), False),          # ... and in a '+' line that repeats it
             (rec(fill, quals=m + b"I" * 8), False),                   # in the quality line only
             (rec((fill + m + fill).lower()), True),
             (rec(fill + mixed), True)]
    if mlen > 1:
        cases += [(rec(fill + m[:h], quals=m[h:] + b"II"), False),     # its halves at the end of the base line and the start of the quality line
                  (rec(fill + m[:h], quals=m[h:] + b"II", plus=b""), False),
                  (rec(fill + m[:h], quals=b"II" + m[:h]), False),     # ... at the record's end and the start of the next header
                  (rec(fill, hdr=m[h:]), False),
                  (rec(fill + m[:h] + b"N" + m[h:] + fill), False)]    # broken by one N
    fq = b"".join(c[0] for c in cases)
    want = [i for i, c in enumerate(cases) if c[1]]
    assert check(ctx, fq, Select(motif=m), msg="motif of %d" % mlen) == want
    assert check(ctx, fq, Select(motif=m, invert=True), msg="motif of %d, inverted" % mlen) == [i for i in range(len(cases)) if i not in want]
    # every offset mod 16 of the text: the same records behind a header that grows byte by byte
    for k in range(16):
        assert check(ctx, b"@" + b"h" * k + b"\n" + fq[3:], Select(motif=m), offs=(k % 3, 0), msg="motif of %d, shifted by %d" % (mlen, k)) == want


BORDERS = [20 * UNIT, ROW, SPAN, WG_TILE]


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("mlen", [2, 17, 32])
@pytest.mark.parametrize("off", [0, 7])
def test_motif_across_every_border(ctx, border, mlen, off):
    """off: where the text begins behind a 16-byte boundary; the kernels' borders count from that boundary"""
    m = MOTIF32[:mlen]
    tail = b"".join(rec(b"T" * 30) for _ in range(5))
    for left in sorted({1, mlen // 2, mlen - 1}):                      # bytes of the occurrence in front of the border
        start = border - off - left                                    # where it begins in the text
        hdr = b"@" + b"h" * (start - 7)
        fq = rec(b"TTTTT" + m + b"TTTTT", hdr=hdr) + tail
        assert fq.find(m) == start and (start + off) // border == 0 and (start + off + mlen - 1) // border == 1
        assert check(ctx, fq, Select(motif=m), offs=(off, 0), msg="motif of %d, %d bytes in front of %d" % (mlen, left, border)) == [0]
        # the same place, a line end in the occurrence: the base line ends at the border, what follows is the '+' and the quality line
        cut = rec(b"TTTTT" + m[:left], quals=m[left:] + b"II", hdr=hdr, plus=b"") + tail
        assert cut.find(m[:left] + b"\n\n" + m[left:]) == start
        assert check(ctx, cut, Select(motif=m), offs=(off, 0), msg="a line end in it, at %d" % border) == []


def test_reverse_complement(ctx):
    m = MOTIF32[:20]
    pal = b"ACGTACGT"
    assert rc(pal) == pal and rc(m) != m
    fill = b"T" * 25
    fq = b"".join([rec(fill + m + fill), rec(fill + rc(m) + fill), rec(fill + m + fill + rc(m)), rec(fill), rec(b"GG" + pal + b"GG"),
                   rec(fill + rc(m).lower()), rec(fill + m[::-1])])
    assert check(ctx, fq, Select(motif=m), msg="forward only") == [0, 2]
    assert check(ctx, fq, Select(motif=m, motif_rc=True), msg="either strand") == [0, 1, 2, 5]
    assert check(ctx, fq, Select(motif=m, motif_rc=True, invert=True), msg="either strand, inverted") == [3, 4, 6]
    assert check(ctx, fq, Select(motif=pal, motif_rc=True), msg="a palindrome") == [4]
    assert check(ctx, fq, Select(motif=pal), msg="a palindrome, forward") == [4]


# ---- compaction and copy ------------------------------------------------------------------------------------------------------------

TEXTS = {"reads": (700, 1, 70, 2), "tiny": (2100, 1, 8, 3)}      # tiny: more than two scan blocks of records
_text = {}


def text(name):
    if name not in _text:
        _text[name] = reads(*TEXTS[name])
    return _text[name]


def alternating(fq, base=0):
    n = len(records(fq))
    for seed in range(1, 50):
        share = sum((sample_hash(seed, base + i) >> 32) < (1 << 31) for i in range(n)) / n
        if 0.3 <= share <= 0.7:
            return Select(sample=1 << 31, sample_seed=seed, index_base=base)
    raise AssertionError("no seed keeps between 30 % and 70 %")


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_compaction(ctx, name):
    fq = text(name)
    n = len(records(fq))
    assert check(ctx, fq, Select(), msg="all kept") == list(range(n))
    assert check(ctx, fq, Select(min_len=1000), msg="none kept") == []
    assert check(ctx, fq, Select(first_record=0, n_records=1), msg="the first") == [0]
    assert check(ctx, fq, Select(first_record=n - 1), msg="the last") == [n - 1]
    s = alternating(fq)
    kept = check(ctx, fq, s, msg="alternating")
    assert 0.3 * n <= len(kept) <= 0.7 * n
    for to in (0, 1, 7, 15):
        for oo in (0, 1, 7, 15):
            check(ctx, fq, s, offs=(to, oo), msg="alternating")
    for o in (1, 15):
        check(ctx, fq, Select(), offs=(o, 16 - o), msg="all kept")
        check(ctx, fq, Select(min_len=1000), offs=(o, 16 - o), msg="none kept")


def test_ranges(ctx):
    fq = text("reads")
    n = len(records(fq))
    for r0, nr in ((1, 1), (n - 1, 1), (333, 200), (0, n), (5, None), (n - 1, None)):
        for kw in (dict(max_n=3), dict(min_len=30, invert=True), dict(motif=b"ACG", motif_rc=True), dict(min_mean_q_x100=4600)):
            kept = check(ctx, fq, Select(first_record=r0, n_records=nr, **kw), msg="records %s..+%s, %r" % (r0, nr, kw))
            assert all(r0 <= r < (n if nr is None else r0 + nr) for r in kept)
    refused(ctx, E_ARG, fq, Select(first_record=n - 9, n_records=10))
    refused(ctx, E_ARG, fq, Select(first_record=n))
    refused(ctx, E_ARG, fq, Select(first_record=n + 5, n_records=1))


# ---- pairs -----------------------------------------------------------------------------------------------------------------------------------

def test_pairs(ctx):
    good, bad = b"ACGT" * 10, b"ACNT" * 10
    pairs = [(good, good), (good, bad), (bad, good), (bad, bad)] * 30
    fq = b"".join(rec(a, hdr=b"@p%d/1" % i) + rec(b, hdr=b"@p%d/2" % i) for i, (a, b) in enumerate(pairs))
    both = check(ctx, fq, Select(max_n=0, pairs=capi.SELECT_BOTH), msg="both")
    assert both == [r for p in range(0, 120, 4) for r in (2 * p, 2 * p + 1)]
    either = check(ctx, fq, Select(max_n=0, pairs=capi.SELECT_EITHER), msg="either")
    assert either == [r for p in range(120) if p % 4 != 3 for r in (2 * p, 2 * p + 1)]
    # after invert: the mates that fail
    assert check(ctx, fq, Select(max_n=0, invert=True, pairs=capi.SELECT_BOTH), msg="both, inverted") == [r for p in range(3, 120, 4) for r in (2 * p, 2 * p + 1)]
    check(ctx, fq, Select(max_n=0, invert=True, pairs=capi.SELECT_EITHER), msg="either, inverted")
    for mode in (capi.SELECT_BOTH, capi.SELECT_EITHER):
        kept = check(ctx, fq, Select(pairs=mode, sample=1 << 31, sample_seed=3, first_record=10, n_records=200, index_base=6), msg="a sample of pairs")
        assert 40 < len(kept) < 160 and all(r ^ 1 in kept for r in kept)
    refused(ctx, E_FORMAT, fq, Select(pairs=1, first_record=0, n_records=7))
    refused(ctx, E_FORMAT, fq + rec(good), Select(pairs=1))                 # odd to the end
    refused(ctx, E_ARG, fq, Select(pairs=1, first_record=1, n_records=8))
    refused(ctx, E_ARG, fq, Select(pairs=2, index_base=1))


# ---- sampling ----------------------------------------------------------------------------------------------------------------------------------

def test_sampling(ctx):
    fq = text("reads")
    rs = records(fq)
    sets = set()
    for seed in (11, 12):
        for base in (0, 1 << 40):
            kept = check(ctx, fq, Select(sample=0x40000000, sample_seed=seed, index_base=base), msg="seed %d, base %d" % (seed, base))
            assert kept == [i for i in range(len(rs)) if (sample_hash(seed, base + i) >> 32) < 0x40000000]
            sets.add(tuple(kept))
    assert len(sets) == 4
    # a range of the text is the text cut to the range, numbered from where it began
    a, b = 123, 555
    s = Select(first_record=a, n_records=b - a, sample=0x60000000, sample_seed=5)
    whole = b"".join(rs[r] for r in check(ctx, fq, s, msg="records a .. b"))
    cut = b"".join(rs[a:b])
    part = records(cut)
    assert whole == b"".join(part[r] for r in check(ctx, cut, Select(sample=0x60000000, sample_seed=5, index_base=a), msg="the text cut to a .. b"))
    # invert does not touch the sample
    assert check(ctx, fq, Select(sample=0x60000000, sample_seed=5, invert=True), msg="inverted") == []


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    fq = reads(200, 20, 40, seed=8)
    refused(ctx, E_FORMAT, fq + b"extra\n", Select())
    refused(ctx, E_ARG, b"", Select())
    s = Select(max_n=5)
    kept, _, _ = selected(fq, s)
    rs = records(fq)
    want = b"".join(rs[r] for r in kept)
    assert 0 < len(kept) < 200
    refused(ctx, E_OVERFLOW, fq, s, cap=len(want) - 1, needs=len(want))
    T, out = Buf(len(fq), 0, fq), Buf(len(want), 0)                   # ... and with exactly that size it succeeds
    assert ctx.select_records(T.ptr, len(fq), s, out.ptr, len(want))[0] == len(want)
    assert out.back("an output of exactly the size needed") == want
    for bad in (Select(motif=b"ACGN"), Select(motif=b"acgt"), Select(motif=b"A", motif_len=33), Select(min_len=5, max_len=4), Select(qual_base=127),
                Select(pairs=3), Select(n_records=0), Select(pairs=1, first_record=1), Select(pairs=2, index_base=3)):
        assert capi.select_check(bad) == E_ARG
        refused(ctx, E_ARG, fq, bad)
    check(ctx, fq, s, msg="after the refusals")


# ---- the switch ----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def sctx(ctx):
    """The session's context; afterwards no selection, no pick, no split, checksums off."""
    try:
        yield ctx
    finally:
        ctx.set_select(None)
        ctx.set_pick(0)
        ctx.set_pair_split(False)
        ctx.set_checksums(False)


def keep(fq, s):
    rs = records(fq)
    return b"".join(rs[r] for r in selected(fq, s)[0])


def picked(fq, what):
    ls = fq.split(b"\n")[:-1]
    out = []
    for i in range(0, len(ls), 4):
        out.append({capi.PICK_FASTA: b">" + ls[i][1:] + b"\n" + ls[i + 1], capi.PICK_NAMES: ls[i][1:], capi.PICK_BASES: ls[i + 1],
                    capi.PICK_QUALS: ls[i + 3]}[what] + b"\n")
    return b"".join(out)


MODES = {"adaptive": dict(tables=capi.TABLES_ADAPTIVE), "frozen": dict(prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN),
         "auto": dict(prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_AUTO)}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_the_switch_behind_decode_host(sctx, mode):
    ctx = sctx
    fq = capi.synth_fastq(1500, 100, seed=31)
    ctx.set_checksums(True)                                           # decode_host installs the blocks' CRCs: those of the full text
    enc = ctx.encode_host(fq, level=3, block_reads=256, **MODES[mode])
    ctx.set_checksums(False)
    assert len(enc.blocks) >= 4 and len(enc.crcs) == len(enc.blocks)
    cap = len(fq) + 4096
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_select() is None
    s = Select(first_record=100, n_records=1200, min_mean_q_x100=2500, motif=b"ACG", motif_rc=True, sample=0xC0000000, sample_seed=9)
    want = keep(fq, s)
    assert 0 < len(want) < len(fq) // 2
    ctx.set_select(s)
    first_difference(ctx.decode_host(enc, level=3, out_cap=cap), want, mode)
    rep = ctx.get_select()
    assert (rep.n_in_range, rep.n_kept, rep.text_bytes, rep.kept_bytes) == (1200, len(records(want)), len(fq), len(want))
    for w in (capi.PICK_FASTA, capi.PICK_NAMES, capi.PICK_BASES, capi.PICK_QUALS):
        ctx.set_pick(w)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(want, w), "%s, pick %d" % (mode, w))
        assert ctx.get_pick() == (w, len(want), len(records(want)))
    # nothing kept: no bytes, no error, and the pick did not run
    ctx.set_select(Select(min_len=1000))
    assert ctx.decode_host(enc, level=3, out_cap=cap) == b"" and ctx.get_select().n_kept == 0 and ctx.get_pick() is None
    ctx.set_pick(0)
    with pytest.raises(capi.SfqError) as e:
        ctx.set_select(Select(qual_base=200))
    assert e.value.code == E_ARG
    ctx.set_select(None)
    assert ctx.decode_host(enc, level=3, out_cap=cap) == fq and ctx.get_select() is None


def test_the_switch_behind_a_window_of_blocks(sctx):
    ctx = sctx
    fq = capi.synth_fastq(1500, 100, seed=32)
    rs = records(fq)
    ctx.set_checksums(True)
    enc = ctx.encode_host(fq, level=3, block_reads=256, **MODES["frozen"])
    ctx.set_checksums(False)
    cap = len(fq) + 4096
    window = b"".join(rs[256:1024])
    s = Select(first_record=10, n_records=700, max_n=0, min_mean_q_x100=2400, index_base=256)
    ctx.set_select(s)
    got, _ = ctx.decode_range_host(enc, 1, 3, level=3, out_cap=cap)
    first_difference(got, keep(window, s), "blocks 1..+3")
    assert 0 < len(got) < len(window) and ctx.get_select().text_bytes == len(window)
    ctx.set_select(None)
    assert ctx.decode_range_host(enc, 1, 3, level=3, out_cap=cap)[0] == window


def test_the_switch_with_pairs(sctx):
    ctx = sctx
    a, b = reads(900, 30, 60, seed=21), reads(900, 30, 60, seed=22)
    ra, rb = records(a), records(b)
    inter = b"".join(x + y for x, y in zip(ra, rb))
    ctx.set_checksums(True)
    enc = ctx.encode_pairs_host(a, b, level=3, block_reads=14, **MODES["frozen"])
    ctx.set_checksums(False)
    cap = len(inter) + 4096
    for mode in (capi.SELECT_BOTH, capi.SELECT_EITHER):
        s = Select(max_n=9, pairs=mode, sample=0xB0000000, sample_seed=4)
        kept = selected(inter, s)[0]
        assert 0 < len(kept) < 1800
        wa, wb = b"".join(ra[r // 2] for r in kept[0::2]), b"".join(rb[r // 2] for r in kept[1::2])
        ctx.set_select(s)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), keep(inter, s), "interleaved")
        ctx.set_pair_split(True)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), wa + wb, "split")
        assert ctx.pair_split() == (len(wa), len(kept) // 2)
        ctx.set_pick(capi.PICK_NAMES)
        first_difference(ctx.decode_host(enc, level=3, out_cap=cap), picked(wa, capi.PICK_NAMES) + picked(wb, capi.PICK_NAMES), "split and picked")
        ctx.set_pick(0)
        ctx.set_select(Select(max_n=9))                               # pairs = 0 under the split: the mates would fall out of step
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_host(enc, level=3, out_cap=cap)
        assert e.value.code == E_ARG
        ctx.set_pair_split(False)
        # a window of pairs: the entry supplies the range, numbered in the decoded blocks
        ctx.set_select(s)
        w0, wn = capi.pair_window_blocks(enc.blocks, 300, 200)
        t0, t1 = int(enc.blocks[w0].first_record), int(enc.blocks[w0 + wn - 1].first_record) + int(enc.blocks[w0 + wn - 1].n_records)
        assert t0 % 2 == 0 and t0 <= 600 and t1 >= 1000
        blocks = b"".join(x for p in zip(ra[t0 // 2:(t1 + 1) // 2], rb[t0 // 2:(t1 + 1) // 2]) for x in p)
        blocks = b"".join(records(blocks)[:t1 - t0])
        sw = Select(max_n=9, pairs=mode, sample=0xB0000000, sample_seed=4, first_record=600 - t0, n_records=400)
        keptw = [r + t0 for r in selected(blocks, sw)[0]]
        assert 0 < len(keptw) < 400
        first, second, _ = ctx.decode_pair_range_host(enc, 300, 200, out_cap=cap)
        first_difference(first, b"".join(ra[r // 2] for r in keptw[0::2]), "a window of pairs, first mates")
        first_difference(second, b"".join(rb[r // 2] for r in keptw[1::2]), "a window of pairs, second mates")
        assert ctx.pair_split() == (len(first), len(keptw) // 2) and ctx.get_select().n_in_range == 400
        ctx.set_select(Select(max_n=9, pairs=mode, first_record=2, n_records=4))
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_pair_range_host(enc, 300, 200, out_cap=cap)
        assert e.value.code == E_ARG
        ctx.set_select(Select(max_n=9))
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_pair_range_host(enc, 300, 200, out_cap=cap)
        assert e.value.code == E_ARG
        ctx.set_select(Select(min_len=1000, pairs=mode))
        assert ctx.decode_pair_range_host(enc, 300, 200, out_cap=cap)[:2] == (b"", b"") and ctx.pair_split() is None
    ctx.set_select(None)
    first, second, _ = ctx.decode_pair_range_host(enc, 300, 200, out_cap=cap)
    assert (first, second) == (b"".join(ra[300:500]), b"".join(rb[300:500])) and ctx.get_select() is None

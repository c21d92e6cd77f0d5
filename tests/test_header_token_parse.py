"""The token step of the header chains (chains.hip k_rec_tokens) walks a round's changed fields once for the wave: a lane parses its own field -- a
short decimal four digits a step (rec_digits.h), anything else through field_type --, and a changed field's previous value is what the lane to
the left has just parsed, or, for lane 0, what lane 63 parsed the round before.  Every case here goes against the oracle byte for byte and back
to its text.  A header chain has max(128, chain_reads) records and a block's last chain what is left, so blocks of 200 in chains of 136 / 135 / 129
end with chains of 64, 65 and 71 records, and blocks of 130 in chains of 129 with a chain of one: rounds of 64 lanes begin at, one past and one
short of a chain's start (a block's first chain does not code its first record, the base)."""
import numpy as np
import pytest

from test_frozen_tables import check_against_oracle

pytestmark = pytest.mark.gpu

GEOS = ((200, 136), (200, 135), (200, 129), (130, 129))            # (block_reads, chain_reads)


def _fastq(headers, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for h in headers:
        ln = 24
        seq = "".join("ACGT"[int(v)] for v in rng.integers(0, 4, ln))
        q = "".join(chr(33 + int(v)) for v in rng.integers(2, 41, ln))
        out.append("@%s\n%s\n+\n%s\n" % (h, seq, q))
    return "".join(out).encode("latin-1")


def _fields(h):
    """map_space (recs.cpp:141-157): the fields of a header and the separators behind them"""
    f, seps, cur = [], [], ""
    for c in h + "\n":
        if c.isascii() and c.isalnum():
            cur += c
        else:
            f.append(cur); seps.append(c); cur = ""
    return f, seps


def _types_as_hex(t):
    """field_type (dev_rec.h) with a cold previous type: does the field come out hexadecimal?"""
    z = t[:1] == "0"
    if z and t[1:2] == "0":
        return False
    body = t[1:] if z else t
    if all(c in "0123456789" for c in body):
        return False                                                 # decimal, or -- where it wraps or would not print back -- a string
    if len(t) > 16 or any(c not in "0123456789abcdefABCDEF" for c in body):
        return False
    return not (any(c in "abcdef" for c in body) and any(c in "ABCDEF" for c in body))


def _for_the_token_step(headers, br):
    """What k_rec_tokens keeps for itself: at most 16 fields, at most 127 bytes, no NUL, no CHANGED field that types as hexadecimal (against the record
    before, or against the block's first record, which a chain starts from)."""
    parsed = [_fields(h) for h in headers]
    for i, h in enumerate(headers):
        f, seps = parsed[i]
        if len(f) > 16 or len(h) > 127 or "\0" in h:
            return False
        for j in {i - 1, i // br * br} - {i, -1}:
            pf, pseps = parsed[j]
            if pseps == seps and any(a != b and _types_as_hex(a) for a, b in zip(f, pf)):
                return False
    return True


def _run(ctx, headers, br, cr, token_step=True, what=""):
    assert len(headers) <= 3000
    if token_step is not None:
        assert _for_the_token_step(headers, br) == token_step, what
    fq = _fastq(headers)
    enc = check_against_oracle(ctx, fq, 3, br=br, cr=cr, step=1, what=what)
    assert ctx.decode_host(enc, level=3, out_cap=2 * len(fq) + 4096) == fq, what


# ---- widths and classes ---------------------------------------------------------------------------------------------------------
def _width_values():
    up = []
    for p in range(1, 10):                                           # 9 -> 10, 99 -> 100, .. 999 999 999 -> 1 000 000 000 (ten bytes: field_type)
        up += [10 ** p - 2, 10 ** p - 1, 10 ** p, 10 ** p + 1]
    vals = [str(v) for v in up + up[::-1]]                           # and back down: the _LT types
    vals += ["7", "0", "05", "00", "007", "", "3", "0", "1", "00", "2", "", "", "9",
             "123456789012345678", "1234567890123456789", "12345678901234567890", "99999999999999999999", "18446744073709551615", "5"]
    b = 100
    for gap in (0x7f, 0x80, 0x7ffd, 0x7ffe, (1 << 32) - 1, 1 << 32):  # exact gaps, up and down
        vals += [str(b), str(b + gap), str(b), str(gap), "0", str(gap)]
    return vals


@pytest.mark.parametrize("br,cr", GEOS)
def test_one_field_through_every_width_and_class(ctx, br, cr):
    vals = _width_values()
    headers = []
    for rep, pad in enumerate((0, 37, 5, 61, 20)):                   # the same walk at other lanes of the rounds
        seq = ["55"] * pad + vals
        headers += ["W%d:%s:k:%d" % (rep, v, 1000 + len(headers) + i) for i, v in enumerate(seq)]
    _run(ctx, headers, br, cr, what="widths")


# ---- where `was` comes from -----------------------------------------------------------------------------------------------------
def _was_block(b, br, k):
    """A block whose record k sees: field A change after two still records (it has changed before where the chain is old enough), field B change
    for the first time in the chain, field C change, sit still for 70 records and change again; a counter and a 4 / 5 digit number change always."""
    out = []
    for i in range(br):
        fa = 5000 + (3 if i >= k - 3 else 0) + (1000 if i >= k else 0)
        fb = 42 if i < k else 40000 + 9 * i
        fc = 100 + (7 if i >= k - 71 else 0) + (50000 if i >= k else 0)
        x = (i * 7919 + b * 13) % 12000 + 900
        out.append("T.%d M7:%d:%d:%d:%d:%d 1:N" % (b * 1000 + 3 * i, fa, fb, fc, x, (x * 31) % 100000))
    return out


@pytest.mark.parametrize("br,cr", GEOS)
def test_previous_values_arrive_at_lane_0_lane_1_and_lane_63(ctx, br, cr):
    rcr = max(128, cr)
    # record k on lane 0, 1 and 63 of the first chain's first round (records 1 .. 64) and of its later ones; of the last chain's rounds
    ks = {1, 2, 64, 65, 66, 128, 129, 130, rcr - 1, rcr, rcr + 1, rcr + 63, rcr + 64, br - 1}
    ks = sorted(k for k in ks if 1 <= k < br)
    headers = []
    for b, k in enumerate(ks):
        headers += _was_block(b, br, k)
    _run(ctx, headers, br, cr, what="was, chains of %d" % rcr)


# ---- left neighbours that have no number to give --------------------------------------------------------------------------------
def _no_number_headers(strings, n=1100):
    cyc = [("5", 0), ("6", 0), ("9", 1), ("12", 1), ("13", 1),          # a shape change spells the record out; then numeric changes
           (strings[0], 1), (strings[0], 1), ("17", 1), ("18", 1), (strings[1], 1), ("25", 1), ("26", 1),
           ("1234567890123456789", 1), ("55", 1), ("56", 1), ("30", 0), ("31", 0)]
    out = []
    for i in range(n):
        v, extra = cyc[i % len(cyc)]
        out.append("N%d:%s:%d%s" % (i // 300, v, 7 * i, ":x" if extra else ""))
    return out


@pytest.mark.parametrize("br,cr", GEOS[:3])
def test_a_left_neighbour_without_a_number_gives_zero(ctx, br, cr):
    _run(ctx, _no_number_headers(("xyz", "Qrs")), br, cr, what="no number to the left")


def test_a_left_string_that_types_as_hexadecimal_hands_the_chain_on(ctx):
    """`abc` is a string to the reader and three hex digits to field_type: the token step flags the chain, k_rec_encode_f codes it."""
    _run(ctx, _no_number_headers(("abc", "abc")), 200, 136, token_step=False, what="abc")


# ---- many fields ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("br,cr", GEOS[:2])
def test_sixteen_fields_all_changing_and_records_past_the_staged_symbols(ctx, br, cr):
    headers = []
    for i in range(1000):
        if (i // br) % 3 == 2:                                       # twelve fields, a few of them changing: the first walk alone
            headers.append(":".join(str(100 + j + (i if j % 4 == 0 else 0)) for j in range(12)))
        else:                                                        # 1 + 6 + 16 * 2 = 39 symbols a record: more than are staged, the second walk
            headers.append(":".join(str(1000 * j + i * (j % 5 + 1)) for j in range(16)))
    _run(ctx, headers, br, cr, what="sixteen fields")


def test_chains_past_forty_symbols_a_record_are_handed_on(ctx):
    """Sixteen fields with gaps of two symbols each: 1 + 6 + 16 * 3 = 55 symbols a record, more than a chain's token room (k_rec_encode_f takes it);
    every third block keeps small gaps and stays."""
    headers = []
    for i in range(1000):
        step = 1 if (i // 200) % 3 == 2 else 1000
        headers.append(":".join(str(100000 * j + i * step * (j % 5 + 1)) for j in range(16)))
    _run(ctx, headers, 200, 136, what="more than forty symbols")


# ---- edges of the column --------------------------------------------------------------------------------------------------------
def _edge_headers(top, n=420):
    """A changing number as the header's first bytes and as its last, a still string between them: `top` bytes where the last number has its five
    digits (nine records in ten), fewer where it is shorter.  (The '@' in front is not part of the header.)"""
    out = []
    for i in range(n):
        first, last = str(1000 + 3 * i), str((i * 104729) % 100003)
        out.append("%s:M%s::%s" % (first, "Z" * (top - 4 - 5 - len(":M::")), last))
    return out


@pytest.mark.parametrize("top", (62, 63, 94, 95, 127, 128))
def test_headers_at_the_edges_of_every_column_size(ctx, top):
    headers = _edge_headers(top)
    assert max(len(h) for h in headers) == top and sum(len(h) == top for h in headers) >= 50
    _run(ctx, headers, 130, 129, token_step=top <= 127, what="headers of %d bytes" % top)

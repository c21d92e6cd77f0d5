"""The host-only entries of the demultiplexing (slimfastq_amd.h "demultiplexed records"): sfq_demux_check, sfq_demux_parse and
sfq_demux_sheet.  No GPU.  The check is held against demux_rule.check, the restatement of the header's list of refusals."""
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Demux, DemuxPart, DEMUX_HEADER as H, DEMUX_BASES as B
import demux_rule

E_ARG = -1
TO_END = 2 ** 64 - 1


def good():
    return Demux([DemuxPart(H, 0, 0, 0, 6)], n_samples=2, max_mm=1), [b"ATCACG", b"TTAGGC"]


def both(rule, rows, want):
    """the library and the restated rule agree, and say want"""
    rc = capi.demux_check(rule, rows)
    assert rc in (0, E_ARG)
    assert (rc == 0) == want, rc
    assert demux_rule.check(rule, rows) == want


# ---- sfq_demux_check ---------------------------------------------------------------------------------------------------------------

def test_check_accepts():
    both(*good(), True)
    both(Demux([DemuxPart(H, 0, 0, 0, 16), DemuxPart(H, 0, 1, 0, 16)], n_samples=1, max_mm=32), [b"ACGT" * 8], True)
    both(Demux([DemuxPart(B, 0, 0, 0xFFFFFFFF - 8, 8)], n_samples=1), [b"ACGTACGT"], True)              # pos + len == 2^32 - 1
    both(Demux([DemuxPart(B, 0, 0, 3, 4), DemuxPart(B, 1, 0, 0, 4)], n_samples=1, pairs=1, split_mates=1, clip=1), [b"ACGTACGT"], True)
    both(Demux([DemuxPart(H, 0, 0, 0, 1)], n_samples=4, max_mm=1), [b"A", b"C", b"G", b"T"], True)      # B == 1
    both(Demux([DemuxPart(H, 0, 0, 0, 6), DemuxPart(99, 7, 7, 7, 0)], n_samples=2), good()[1], True)    # part 1 absent: not looked at
    both(Demux([DemuxPart(H, 0, 0, 0, 6)], n_samples=2, first_record=3, n_records=1), good()[1], True)  # an odd first record without pairs


def test_check_null_pointers():
    rule, rows = good()
    assert capi.demux_check(None, rows) == E_ARG
    assert capi.demux_check(rule, None) == E_ARG
    assert not demux_rule.check(None, rows) and not demux_rule.check(rule, None)


@pytest.mark.parametrize("what,change", [
    ("n_records == 0", lambda r: setattr(r, "n_records", 0)),
    ("pairs > 1", lambda r: setattr(r, "pairs", 2)),
    ("an odd first_record with pairs", lambda r: (setattr(r, "pairs", 1), setattr(r, "first_record", 1))),
    ("split_mates without pairs", lambda r: setattr(r, "split_mates", 1)),
    ("mate != 0 without pairs", lambda r: setattr(r.part[0], "mate", 1)),
    ("mate > 1", lambda r: (setattr(r, "pairs", 1), setattr(r.part[0], "mate", 2))),
    ("sub > 1", lambda r: setattr(r.part[0], "sub", 2)),
    ("sub != 0 on a BASES part", lambda r: (setattr(r.part[0], "src", B), setattr(r.part[0], "sub", 1))),
    ("an unknown src", lambda r: setattr(r.part[0], "src", 3)),
    ("src 0 on part 0", lambda r: setattr(r.part[0], "src", 0)),
    ("pos + len overflows 32 bits", lambda r: setattr(r.part[0], "pos", 0xFFFFFFFF - 5)),
    ("max_mm > B", lambda r: setattr(r, "max_mm", 7)),
    ("n_samples == 0", lambda r: setattr(r, "n_samples", 0)),
])
def test_check_refuses(what, change):
    rule, rows = good()
    change(rule)
    both(rule, rows[:rule.n_samples], False)


def test_check_refuses_lengths():
    both(Demux([DemuxPart(H, 0, 0, 0, 0)], n_samples=1), [b""], False)                                  # B == 0
    both(Demux([DemuxPart(H, 0, 0, 0, 0), DemuxPart(H, 0, 1, 0, 6)], n_samples=1), [b"ATCACG"], False)  # len0 == 0
    both(Demux([DemuxPart(H, 0, 0, 0, 33)], n_samples=1), [b"A" * 33], False)                           # B == 33
    both(Demux([DemuxPart(H, 0, 0, 0, 17), DemuxPart(H, 0, 1, 0, 16)], n_samples=1), [b"A" * 33], False)
    both(Demux([DemuxPart(H, 0, 0, 0, 16), DemuxPart(H, 0, 1, 0, 16)], n_samples=1), [b"A" * 32], True)


def test_check_sample_counts():
    rows = [bytes(b"ACGT"[(s >> (2 * i)) & 3] for i in range(7)) for s in range(4097)]
    both(Demux([DemuxPart(H, 0, 0, 0, 7)], n_samples=4096), rows[:4096], True)
    assert capi.demux_check(Demux([DemuxPart(H, 0, 0, 0, 7)], n_samples=4097), rows) == E_ARG
    assert not demux_rule.check(Demux([DemuxPart(H, 0, 0, 0, 7)], n_samples=4097), rows)


@pytest.mark.parametrize("rows", [[b"ATCACG", b"ATCACN"], [b"ATCACG", b"atcacg"], [b"ATCACG", b"ATC.CG"], [b"ATCACG", b"ATCACG"],
                                  [b"TTAGGC", b"ATCACG", b"TTAGGC"]])
def test_check_refuses_barcodes(rows):
    both(Demux([DemuxPart(H, 0, 0, 0, 6)], n_samples=len(rows)), rows, False)


def test_rows_that_are_not_the_rules_never_reach_the_library():
    """the library reads n_samples * B bytes: the wrapper refuses rows of another size itself"""
    rule, rows = good()
    for bad in (rows[:1], rows + [b"ACGTAC"], [b"ATCAC", b"TTAGG"], b"ATCACGTTAGG", []):
        assert capi.demux_check(rule, bad) == E_ARG
        with pytest.raises(ValueError) as e:
            capi._barcode_rows(bad, rule)
        assert "2 samples of 6 bases" in str(e.value)
    assert capi._barcode_rows(rows, rule) == capi._barcode_rows(b"".join(rows), rule) == b"ATCACGTTAGGC"


def test_the_rules_own_shortcut():
    """demux_rule.verdict compares the upper-cased bytes at once: the same distances as distance(), byte by byte"""
    rows = [b"ACGTAC", b"ACGTTT", b"TTTTTT"]
    for obs in (b"ACGTAC", b"acgtac", b"ACGTAN", b"nCGTAC", b"ACGTT.", b"tttttt", b"GGGGGG", b"ACGTAT", b"ACGT\rC"):
        ds = [demux_rule.distance(obs, r) for r in rows]
        m = min(ds)
        want = "far" if m > 1 else "ambiguous" if ds.count(m) > 1 else (ds.index(m), m)
        assert demux_rule.verdict(obs, rows, 1) == want, obs


# ---- sfq_demux_parse ---------------------------------------------------------------------------------------------------------------

def fields(p):
    return (p.src, p.mate, p.sub, p.pos, p.len)


def test_parse_defaults():
    r = capi.demux_parse("sheet.tsv")
    assert (r.first_record, r.n_records, r.pairs, r.split_mates, r.max_mm, r.clip, r.n_samples) == (0, TO_END, 0, 0, 1, 0, 0)
    assert fields(r.part[0]) == (H, 0, 0, 0, 0) and fields(r.part[1]) == (H, 0, 1, 0, 0)
    r2 = capi.demux_parse("a/b=c.tsv,hdr")                             # the first term is the sheet, whatever it says
    assert fields(r2.part[0]) == fields(r.part[0]) and fields(r2.part[1]) == fields(r.part[1])


def test_parse_every_term():
    r = capi.demux_parse("s.tsv,mm=0,inline,clip,out=pre/fix_,counts=c.tsv")
    assert (r.max_mm, r.clip) == (0, 1)
    assert fields(r.part[0]) == (B, 0, 0, 0, 0) and r.part[1].len == 0 and r.part[1].src == 0
    r = capi.demux_parse("s.tsv,inline=3,inline2=5,mm=32")
    assert r.max_mm == 32 and fields(r.part[0]) == (B, 0, 0, 3, 0) and fields(r.part[1]) == (B, 1, 0, 5, 0)
    r = capi.demux_parse("s.tsv,inline=4294967295,hdr2")
    assert fields(r.part[0]) == (B, 0, 0, 0xFFFFFFFF, 0) and fields(r.part[1]) == (H, 0, 0, 0, 0)
    r = capi.demux_parse("s.tsv,inline,inline2")
    assert fields(r.part[1]) == (B, 1, 0, 0, 0)


@pytest.mark.parametrize("spec,says", [("", "empty"), (",hdr", "sheet"), ("s,mm=33", "mm=33"), ("s,mm=", "mm="), ("s,mm=x", "mm=x"),
                                       ("s,mm", "mm"), ("s,inline=-1", "inline=-1"), ("s,inline=4294967296", "4294967296"),
                                       ("s,inline2", "inline2"), ("s,hdr2", "hdr2"), ("s,hdr,inline", "hdr and inline"),
                                       ("s,inline,inline2,hdr2", "inline2 and hdr2"), ("s,out=", "out="), ("s,counts=", "counts="),
                                       ("s,bogus", "bogus"), ("s,clip=1", "clip=1"), ("s,", "no such term")])
def test_parse_refuses(spec, says):
    with pytest.raises(ValueError) as e:
        capi.demux_parse(spec)
    assert says in str(e.value)


# ---- sfq_demux_sheet ---------------------------------------------------------------------------------------------------------------

def test_sheet_forms():
    text = b"# a lane\n\nalpha\tATCACG+TTAGGC\n#beta\tAAAAAA+CCCCCC\nBeta.2\tttaggc\tatcacg\r\n\ngamma_-9\tAcGtAc+gTaCgT"      # no final line end
    names, rows, l0, l1 = capi.demux_sheet(text)
    assert names == ["alpha", "Beta.2", "gamma_-9"]
    assert rows == [b"ATCACGTTAGGC", b"TTAGGCATCACG", b"ACGTACGTACGT"] and (l0, l1) == (6, 6)
    names, rows, l0, l1 = capi.demux_sheet(b"s1\tACGTACGT\ns2\tacgtacga\n")
    assert names == ["s1", "s2"] and rows == [b"ACGTACGT", b"ACGTACGA"] and (l0, l1) == (8, 0)
    n64 = b"n" * 64
    assert capi.demux_sheet(n64 + b"\tA\n")[0] == [n64.decode()]
    assert capi.demux_sheet(b"x\t" + b"ACGT" * 4 + b"+" + b"TGCA" * 4 + b"\n")[2:] == (16, 16)


@pytest.mark.parametrize("text,line,says", [
    (b"", 0, "no sample"), (b"# only\n\n", 2, "no sample"),
    (b"a\tACGT\nb\tACG\n", 2, "lengths"), (b"a\tACGT+AC\nb\tACG+ACG\n", 2, "lengths"), (b"a\tACGT\nb\tACGT+A\n", 2, "lengths"),
    (b"a\tACGT\n\n# c\nb c\tAAAA\n", 4, "name"), (b"\tACGT\n", 1, "name"), (b"n" * 65 + b"\tACGT\n", 1, "name"), (b"a/b\tACGT\n", 1, "name"),
    (b"a\tACGT\na\tAAAA\n", 2, "earlier row"), (b"a\tACGT\nb\tacgt\n", 2, "earlier row"), (b"a\tAC+GT\nb\tAC\tGT\n", 2, "earlier row"),
    (b"ok\tACGT\nunassigned\tAAAA\n", 2, "unassigned"),
    (b"a ACGT\n", 1, "TAB"), (b"a\tACGN\n", 1, "ACGT"), (b"a\t\n", 1, "barcode"), (b"a\tAC+\n", 1, "second"), (b"a\tAC+GT+AA\n", 1, "ACGT"),
    (b"a\t+ACGT\n", 1, "barcode"), (b"a\t" + b"A" * 33 + b"\n", 1, "32"), (b"a\t" + b"A" * 17 + b"+" + b"C" * 16 + b"\n", 1, "32"),
])
def test_sheet_refuses(text, line, says):
    with pytest.raises(ValueError) as e:
        capi.demux_sheet(text)
    assert "line %d:" % line in str(e.value) and says in str(e.value), str(e.value)


def test_sheet_sample_counts():
    rows = [b"s%d\t" % s + bytes(b"ACGT"[(s >> (2 * i)) & 3] for i in range(7)) + b"\n" for s in range(4097)]
    names, codes, l0, l1 = capi.demux_sheet(b"".join(rows[:4096]))
    assert len(names) == 4096 and names[4095] == "s4095" and codes[4095] == rows[4095].split(b"\t")[1].strip() and (l0, l1) == (7, 0)
    rule = Demux([DemuxPart(H, 0, 0, 0, l0)], n_samples=4096)
    assert capi.demux_check(rule, codes) == 0
    with pytest.raises(ValueError) as e:
        capi.demux_sheet(b"".join(rows))
    assert "line 4097:" in str(e.value)
    with pytest.raises(ValueError) as e:                               # the caller's own limit
        capi.demux_sheet(b"".join(rows[:3]), max_samples=2)
    assert "line 3:" in str(e.value)

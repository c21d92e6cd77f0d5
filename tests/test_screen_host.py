"""The host-only entries of the screened records (no GPU): sfq_screen_check, sfq_screen_parse, sfq_fasta_sequences against
screen_rule.flat_fasta."""
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Screen
from screen_rule import flat_fasta, TO_END

E_ARG, E_OVERFLOW = -1, -5


def test_screen_check():
    assert capi.screen_check(Screen()) == 0
    for ok in (Screen(pairs=1), Screen(pairs=2, first_record=4, n_records=2), Screen(min_hits=0xFFFFFFFF, min_pct=100, keep_matched=True),
               Screen(first_record=3, n_records=1)):
        assert capi.screen_check(ok) == 0
    for bad in (Screen(n_records=0), Screen(pairs=3), Screen(pairs=1, first_record=1), Screen(pairs=2, first_record=7), Screen(min_hits=0),
                Screen(min_pct=101)):
        assert capi.screen_check(bad) == E_ARG
    assert capi.lib().sfq_screen_check(None) == E_ARG


def fields(r):
    return (r.first_record, r.n_records, r.pairs, r.min_hits, r.min_pct, r.keep_matched)


def test_screen_parse():
    assert (fields(capi.screen_parse("ref=a.fa")[0]), capi.screen_parse("ref=a.fa")[1]) == ((0, TO_END, 0, 1, 0, 0), 27)
    r, k = capi.screen_parse("ref=a.fa,ref=dir/b,k=31,hits=3,pct=100,keep,both")
    assert (fields(r), k) == ((0, TO_END, 2, 3, 100, 1), 31)
    r, k = capi.screen_parse("k=4,either,hits=4294967295")
    assert (fields(r), k) == ((0, TO_END, 1, 0xFFFFFFFF, 0, 0), 4)
    assert capi.screen_check(r) == 0
    for bad in ("", "k=3", "k=32", "k=", "k=x", "hits=0", "hits=4294967296", "pct=101", "pct=-1", "ref=", "keep=1", "nokeep", "ref=a,,k=5", "k=5,",
                "K=5", "both=1", "c.fa"):
        with pytest.raises(ValueError) as e:
            capi.screen_parse(bad)
        assert str(e.value)
    L = capi.lib()
    k = capi.C.c_uint32()
    assert L.sfq_screen_parse(None, capi.C.byref(Screen()), capi.C.byref(k), None, 0) == E_ARG
    assert L.sfq_screen_parse(b"k=5", None, capi.C.byref(k), None, 0) == E_ARG
    assert L.sfq_screen_parse(b"k=5", capi.C.byref(Screen()), None, None, 0) == E_ARG
    assert L.sfq_screen_parse(b"k=2", capi.C.byref(Screen()), capi.C.byref(k), None, 0) == E_ARG      # no room for a message: the code alone


FASTAS = [
    b">one\nACGT\nACGT\n>two\nGG\n",
    b">one\r\nACGT\r\nAC\rGT\r\n>two\r\nGG\r\n",                        # CRLF; a '\r' inside a line stays
    b">one\nACGT\nAC",                                                 # no final newline
    b">one\nACGT\nAC\r",                                               # ... where a last '\r' is no line end's
    b">one\n>two\n\n>three\nAC\n\nGT\n>four",                          # empty records, empty lines, a last header without a line end
    b"ACGT\n>x\nAC>GT\nTT >y\n",                                       # bases in front of the first header; '>' only counts at a line's start
    b"\n\n\n", b">", b"A", b"\r\n", b"",
]


@pytest.mark.parametrize("fa", FASTAS)
def test_fasta_sequences(fa):
    want = flat_fasta(fa)
    assert len(want) <= len(fa)
    assert capi.fasta_sequences(fa, size_only=True) == len(want)
    assert capi.fasta_sequences(fa) == want
    assert capi.fasta_sequences(fa, cap=len(want) + 9) == want
    if want:
        with pytest.raises(capi.SfqError) as e:
            capi.fasta_sequences(fa, cap=len(want) - 1)
        assert e.value.code == E_OVERFLOW
        out = capi.C.create_string_buffer(b"I" * len(fa), len(fa))     # a cap too small writes nothing
        assert capi.lib().sfq_fasta_sequences(fa, len(fa), capi.C.cast(out, capi.C.c_void_p), len(want) - 1) == E_OVERFLOW
        assert out.raw == b"I" * len(fa)


def test_fasta_sequences_by_hand():
    assert capi.fasta_sequences(b">one\nACGT\nACGT\n>two\nGG\n") == b"\nACGTACGT\nGG"
    assert capi.fasta_sequences(b">one\r\nAC\r\nGT\r\n") == b"\nACGT"
    assert capi.lib().sfq_fasta_sequences(None, 5, None, 0) == E_ARG

"""The host side of the selection (api.cpp): sfq_select_check on every rule it refuses, and the conversion of the CLI's list of terms
(sfq_select_parse).  No GPU."""
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Select

E_ARG = -1


def test_the_rule_that_keeps_everything_passes():
    s = Select()
    assert (s.first_record, s.n_records, s.min_len, s.max_len, s.max_n, s.min_mean_q_x100, s.motif_len, s.pairs, s.sample) == \
        (0, 0xFFFFFFFFFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0, 0, 0)
    assert capi.select_check(s) == 0
    assert capi.select_check(Select(motif=b"ACGT" * 8, motif_rc=True, pairs=2, first_record=4, index_base=6, qual_base=126, min_len=7, max_len=7)) == 0


@pytest.mark.parametrize("bad", [dict(motif=b"ACGN"), dict(motif=b"acgt"), dict(motif=b"AC\n"), dict(motif=b"A", motif_len=33),
                                 dict(min_len=5, max_len=4), dict(qual_base=127), dict(pairs=3), dict(n_records=0),
                                 dict(pairs=1, first_record=1), dict(pairs=2, index_base=1)])
def test_every_refusal(bad):
    assert capi.select_check(Select(**bad)) == E_ARG


def test_the_list_of_terms():
    s, either = capi.select_parse("sample=0.5")
    assert (s.sample, s.sample_seed, either) == (1 << 31, 0, False) and capi.select_check(s) == 0
    s, either = capi.select_parse("minlen=50,maxlen=151,maxn=2,meanq=20,seq=acGt,rc,invert,either,sample=0.25:77")
    assert (s.min_len, s.max_len, s.max_n, s.min_mean_q_x100, s.qual_base) == (50, 151, 2, 2000, 33)
    assert (bytes(s.motif[:s.motif_len]), s.motif_rc, s.invert, either) == (b"ACGT", 1, 1, True)
    assert (s.sample, s.sample_seed, s.pairs, s.first_record, s.n_records) == (1 << 30, 77, 0, 0, 0xFFFFFFFFFFFFFFFF)
    assert capi.select_parse("meanq=27.5")[0].min_mean_q_x100 == 2750 and capi.select_parse("meanq=7.05")[0].min_mean_q_x100 == 705
    for bad in ("bogus", "meanq=1.234", "seq=ACGU", "sample=1", "sample=0", "minlen=x"):
        with pytest.raises(ValueError):
            capi.select_parse(bad)

"""The host side of the mates' overlap (api.cpp): sfq_overlap_check at every bound, and the conversion of the CLI's list of terms
(sfq_overlap_parse) with its defaults and every refusal's words.  No GPU."""
import ctypes

import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Overlap

E_ARG = -1
TO_END = 0xFFFFFFFFFFFFFFFF


def rule(o):
    return (o.first_record, o.n_records, o.min_overlap, o.max_mm, o.max_mm_pct, o.cut)


def test_struct_sizes():
    assert capi.OVERLAP_MAX_LEN == 512
    assert ctypes.sizeof(capi.Overlap) == 32
    assert ctypes.sizeof(capi.OverlapReport) == 8 * (9 + 2 * 512 + 1)


def test_the_default_rule_passes():
    assert rule(Overlap()) == (0, TO_END, 30, 5, 20, 1)
    assert capi.overlap_check(Overlap()) == 0
    assert capi.lib().sfq_overlap_check(None) == E_ARG


@pytest.mark.parametrize("good", [dict(min_overlap=1), dict(min_overlap=512), dict(max_mm=0), dict(max_mm=0xFFFFFFFF), dict(max_mm_pct=0), dict(max_mm_pct=100),
                                  dict(cut=0), dict(first_record=7, n_records=2), dict(first_record=TO_END, n_records=1)])
def test_every_bound_met(good):
    assert capi.overlap_check(Overlap(**good)) == 0


@pytest.mark.parametrize("bad", [dict(min_overlap=0), dict(min_overlap=513), dict(max_mm_pct=101), dict(n_records=0)])
def test_every_refusal(bad):
    assert capi.overlap_check(Overlap(**bad)) == E_ARG


def test_the_list_of_terms():
    assert rule(capi.overlap_parse("default")) == (0, TO_END, 30, 5, 20, 1)
    assert rule(capi.overlap_parse("min=12")) == (0, TO_END, 12, 5, 20, 1)
    assert rule(capi.overlap_parse("mm=0")) == (0, TO_END, 30, 0, 20, 1)
    assert rule(capi.overlap_parse("pct=100")) == (0, TO_END, 30, 5, 100, 1)
    assert rule(capi.overlap_parse("nocut")) == (0, TO_END, 30, 5, 20, 0)
    assert rule(capi.overlap_parse("min=1,mm=4000000000,pct=0,nocut")) == (0, TO_END, 1, 4000000000, 0, 0)
    assert rule(capi.overlap_parse("nocut,min=512")) == (0, TO_END, 512, 5, 20, 0)
    assert capi.overlap_check(capi.overlap_parse("min=512,pct=100")) == 0
    assert capi.lib().sfq_overlap_parse(None, ctypes.byref(Overlap()), None, 0) == E_ARG
    assert capi.lib().sfq_overlap_parse(b"bogus", ctypes.byref(Overlap()), None, 0) == E_ARG      # err may be NULL


@pytest.mark.parametrize("spec, says", [("bogus", "bogus"), ("", "empty"), ("min", "min"), ("min=", "min="), ("min=0", "min="), ("min=513", "min="),
                                        ("min=x", "min="), ("min=-3", "min="), ("mm=", "mm="), ("mm=1.5", "mm="), ("mm=4294967296", "mm="),
                                        ("pct=101", "pct="), ("pct=x", "pct="), ("nocut=1", "nocut=1"), ("default,min=3", "default"),
                                        ("min=3,default", "default"), ("min=30,,mm=1", "no such term"), ("min=30,", "no such term"),
                                        ("hist=x.tsv", "hist=x.tsv")])
def test_every_refusal_of_the_list_names_its_term(spec, says):
    with pytest.raises(ValueError) as e:
        capi.overlap_parse(spec)
    assert says in str(e.value), str(e.value)

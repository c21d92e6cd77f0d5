"""The host side of the mates' merge (api.cpp): the structs' sizes and sfq_merge_check at every bound.  No GPU."""
import ctypes

import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Merge

E_ARG = -1
TO_END = 0xFFFFFFFFFFFFFFFF


def test_struct_sizes():
    assert ctypes.sizeof(capi.Merge) == 32
    assert ctypes.sizeof(capi.MergeReport) == 8 * (11 + 2 * 512 + 1)


def test_the_default_rule_passes():
    m = Merge()
    assert (m.first_record, m.n_records, m.min_overlap, m.max_mm, m.max_mm_pct, m.qual_base) == (0, TO_END, 30, 5, 20, 33)
    assert capi.merge_check(m) == 0
    assert capi.lib().sfq_merge_check(None) == E_ARG


@pytest.mark.parametrize("good", [dict(min_overlap=1), dict(min_overlap=512), dict(max_mm=0), dict(max_mm=0xFFFFFFFF), dict(max_mm_pct=0), dict(max_mm_pct=100),
                                  dict(qual_base=33), dict(qual_base=64), dict(qual_base=124), dict(first_record=7, n_records=2),
                                  dict(first_record=TO_END, n_records=1)])
def test_every_bound_met(good):
    assert capi.merge_check(Merge(**good)) == 0


@pytest.mark.parametrize("bad", [dict(min_overlap=0), dict(min_overlap=513), dict(max_mm_pct=101), dict(n_records=0), dict(qual_base=32), dict(qual_base=125),
                                 dict(qual_base=0), dict(qual_base=0xFFFFFFFF)])
def test_every_refusal(bad):
    assert capi.merge_check(Merge(**bad)) == E_ARG

"""The host side of the trim (api.cpp): sfq_trim_check at every bound, and the conversion of the CLI's list of terms (sfq_trim_parse)
with every refusal's words.  No GPU."""
import ctypes

import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Trim

E_ARG = -1
OFF32 = 0xFFFFFFFF


def test_struct_sizes():
    assert ctypes.sizeof(capi.Trim) == 76
    assert ctypes.sizeof(capi.TrimReport) == 8 * 11


def test_the_rule_that_changes_nothing_passes():
    t = Trim()
    assert (t.head, t.tail, t.max_len, t.lead_q, t.trail_q, t.win_len, t.win_q_x100, t.qual_base, t.adapter_len, t.adapter_mm, t.adapter_min) == \
        (0, 0, OFF32, 0, 0, 0, 0, 33, 0, 0, 0)
    assert capi.trim_check(t) == 0
    assert capi.lib().sfq_trim_check(None) == E_ARG


@pytest.mark.parametrize("good", [dict(win_len=32, win_q_x100=OFF32), dict(adapter=b"ACGT" * 8, adapter_mm=32, adapter_min=32), dict(adapter=b"A", adapter_min=1),
                                  dict(qual_base=126), dict(qual_base=0), dict(max_len=0), dict(head=OFF32, tail=OFF32, lead_q=OFF32, trail_q=OFF32),
                                  dict(adapter_mm=0, adapter_min=7), dict(adapter=b"ACG", adapter_mm=3, adapter_min=3)])
def test_every_bound_met(good):
    assert capi.trim_check(Trim(**good)) == 0


@pytest.mark.parametrize("bad", [dict(win_len=33), dict(adapter=b"A", adapter_len=33), dict(adapter=b"ACGN"), dict(adapter=b"acgt"), dict(adapter=b"AC\n"),
                                 dict(adapter=b"ACG", adapter_mm=4), dict(adapter_mm=1), dict(adapter=b"ACG", adapter_min=0), dict(adapter=b"ACG", adapter_min=4),
                                 dict(qual_base=127)])
def test_every_refusal(bad):
    assert capi.trim_check(Trim(**bad)) == E_ARG


def test_the_list_of_terms():
    t = capi.trim_parse("head=5")
    assert (t.head, t.tail, t.max_len, t.lead_q, t.trail_q, t.win_len, t.qual_base, t.adapter_len, t.adapter_mm, t.adapter_min) == (5, 0, OFF32, 0, 0, 0, 33, 0, 0, 0)
    assert capi.trim_check(t) == 0
    t = capi.trim_parse("head=1,tail=2,maxlen=100,q5=3,q3=20,win=4:17.25,adapter=agatCGGAAGAGC,mm=1,overlap=5")
    assert (t.head, t.tail, t.max_len, t.lead_q, t.trail_q, t.win_len, t.win_q_x100, t.qual_base) == (1, 2, 100, 3, 20, 4, 1725, 33)
    assert (bytes(t.adapter[:t.adapter_len]), t.adapter_mm, t.adapter_min) == (b"AGATCGGAAGAGC", 1, 5) and capi.trim_check(t) == 0
    assert capi.trim_parse("maxlen=0").max_len == 0
    assert [capi.trim_parse("adapter=" + "ACGT"[:k]).adapter_min for k in (1, 2, 3, 4)] == [1, 2, 3, 3]      # overlap = min(3, adapter_len)
    assert capi.trim_parse("adapter=ACGT").adapter_mm == 0
    assert capi.trim_parse("win=32:20").win_q_x100 == 2000 and capi.trim_parse("win=1:7.5").win_q_x100 == 750 and capi.trim_parse("win=1:7.05").win_q_x100 == 705


@pytest.mark.parametrize("spec, says", [("bogus", "bogus"), ("head", "head"), ("", "empty"), ("head=x", "head="), ("tail=-1", "tail="), ("maxlen=1.5", "maxlen="),
                                        ("q5=", "q5="), ("q3=2q", "q3="), ("win=4", "win="), ("win=0:20", "win="), ("win=33:20", "win="),
                                        ("win=4:1.234", "win="), ("win=4:x", "win="), ("adapter=", "adapter="), ("adapter=ACGU", "adapter="),
                                        ("adapter=" + "A" * 33, "adapter="), ("mm=1", "mm="), ("overlap=3", "overlap="), ("adapter=ACG,mm=4", "mm="),
                                        ("adapter=ACG,overlap=0", "overlap="), ("adapter=ACG,overlap=4", "overlap="), ("adapter=ACG,mm=x", "mm="),
                                        ("head=1,,tail=1", "no such term")])
def test_every_refusal_of_the_list_names_its_term(spec, says):
    with pytest.raises(ValueError) as e:
        capi.trim_parse(spec)
    assert says in str(e.value), str(e.value)

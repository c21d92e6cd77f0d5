"""The host side of the dedup (api.cpp): sfq_dedup_check on every rule it refuses, and the bindings' struct sizes.  No GPU."""
import ctypes

from slimfastq_amd import capi
from slimfastq_amd.capi import Dedup

E_ARG = -1
TO_END = 0xFFFFFFFFFFFFFFFF


def test_the_structs_are_the_headers():
    assert ctypes.sizeof(capi.Dedup) == 8 + 8 + 4 + 4
    assert ctypes.sizeof(capi.DedupReport) == 8 * 9
    assert [f[0] for f in capi.DedupReport._fields_] == ["n_in_range", "n_units", "n_kept", "n_dup_set", "n_dup_call", "text_bytes", "kept_bytes",
                                                         "set_keys", "set_key_bytes"]
    for name in ("sfq_dedup_check", "sfq_dedup_records", "sfq_dedup_set_create", "sfq_dedup_set_clear", "sfq_dedup_set_destroy", "sfq_dedup_set_info",
                 "sfq_ctx_set_dedup", "sfq_get_dedup"):
        assert name in capi.EXPORTS and getattr(capi.lib(), name)


def test_the_default_rule_and_what_passes():
    d = Dedup()
    assert (d.first_record, d.n_records, d.pairs, d.use_set) == (0, TO_END, 0, 0)
    assert capi.dedup_check(d) == 0
    for good in (dict(first_record=7), dict(first_record=7, n_records=1), dict(pairs=1), dict(pairs=1, first_record=6, n_records=3),
                 dict(use_set=True), dict(pairs=1, use_set=True, first_record=2)):
        assert capi.dedup_check(Dedup(**good)) == 0, good


def test_what_the_check_refuses():
    assert capi.lib().sfq_dedup_check(None) == E_ARG
    for bad in (dict(n_records=0), dict(pairs=2), dict(pairs=0xFFFFFFFF), dict(pairs=1, first_record=1), dict(pairs=1, first_record=2 ** 40 + 1),
                dict(pairs=1, n_records=0)):
        assert capi.dedup_check(Dedup(**bad)) == E_ARG, bad


def test_entries_without_a_context():
    L = capi.lib()
    assert L.sfq_dedup_set_create(None, 1, 1, 0) == E_ARG and L.sfq_dedup_set_clear(None) == E_ARG and L.sfq_dedup_set_destroy(None) == E_ARG
    assert L.sfq_dedup_set_info(None, None, None, None, None) == E_ARG
    assert L.sfq_ctx_set_dedup(None, None) == E_ARG and L.sfq_get_dedup(None, None) == E_ARG

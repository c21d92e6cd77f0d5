"""Quality binning, the host side: the preset tables, the check of a caller's table, the -Q option's argument
errors -- found before any GPU is touched, like -R's -- and the resources of the kernels of qmap.hip."""
import subprocess

import pytest

from slimfastq_amd import capi
from test_gpu_parity import _cli
from test_kernel_resources import kernel_metadata

# Phred+33 bins (lowest Q, highest Q, the Q they become); Q0 and Q1 stay
ILLUMINA8 = ((2, 9, 6), (10, 19, 15), (20, 24, 22), (25, 29, 27), (30, 34, 33), (35, 39, 37), (40, 93, 40))
NOVASEQ4 = ((2, 2, 2), (3, 14, 12), (15, 29, 23), (30, 93, 37))
PRESETS = {"illumina8": (capi.QMAP_ILLUMINA8, ILLUMINA8), "novaseq4": (capi.QMAP_NOVASEQ4, NOVASEQ4)}


def table_of(bins) -> bytes:
    t = list(range(256))
    for lo, hi, to in bins:
        for q in range(lo, hi + 1):
            t[33 + q] = 33 + to
    return bytes(t)


@pytest.mark.parametrize("name", sorted(PRESETS))
def test_preset_tables_entry_by_entry(name):
    pid, bins = PRESETS[name]
    want = table_of(bins)
    got = capi.quality_map_preset(name)
    assert len(got) == 256 and got == capi.quality_map_preset(pid)
    for b in range(256):
        assert got[b] == want[b], (name, b, got[b], want[b])
    assert sorted(set(got[35:127])) == sorted(33 + to for _, _, to in bins)       # Q2 .. Q93 fall on the bins' values, all of them used


@pytest.mark.parametrize("name", sorted(PRESETS))
def test_presets_pass_the_check_and_are_idempotent(name):
    t = capi.quality_map_preset(name)
    assert capi.quality_map_check(t) == 0
    assert bytes(t[t[b]] for b in range(256)) == t


@pytest.mark.parametrize("name", sorted(PRESETS))
def test_presets_keep_everything_that_is_no_quality_and_the_no_call_marks(name):
    t = capi.quality_map_preset(name)
    for b in list(range(33)) + list(range(127, 256)) + [ord("!"), ord('"')]:
        assert t[b] == b, (name, b)


def _with(b, v):
    t = bytearray(range(256))
    t[b] = v
    return bytes(t)


@pytest.mark.parametrize("what,table", [("moves the line end", _with(10, ord("I"))), ("moves the carriage return", _with(13, ord("I"))),
                                        ("moves byte 127", _with(127, ord("I"))), ("maps 'I' to a space", _with(ord("I"), 32)),
                                        ("maps 'I' to a line end", _with(ord("I"), 10)), ("maps '~' to byte 127", _with(126, 127))])
def test_check_refuses(what, table):
    assert capi.quality_map_check(bytes(range(256))) == 0
    assert capi.quality_map_check(table) == -1, what


def test_an_unknown_preset_is_an_argument_error():
    import ctypes as C
    buf = C.create_string_buffer(256)
    assert capi.lib().sfq_quality_map_preset(99, buf) == -1            # SFQ_E_ARG
    assert capi.lib().sfq_quality_map_preset(0, buf) == -1
    with pytest.raises(capi.SfqError) as e:
        capi.quality_map_preset("nosuch")
    assert e.value.code == -1


RECORD = b"@r\nACGT\n+\nIIII\n"


def test_cli_refuses_an_unknown_map_before_touching_a_gpu(tmp_path):
    out = tmp_path / "x.sfq"
    p = subprocess.run([_cli(), "-Q", "nosuch", "-f", str(out)], input=RECORD, capture_output=True, timeout=60)
    assert p.returncode == 1 and b"-Q nosuch" in p.stderr and b"illumina8" in p.stderr and not out.exists()
    assert b"HIP" not in p.stderr and p.stdout == b""


def test_cli_refuses_a_map_with_a_decode_before_touching_a_gpu(tmp_path):
    for args in (["-Q", "illumina8", "-d"], ["-d", "-Q", "illumina8"]):
        p = subprocess.run([_cli()] + args + ["-f", str(tmp_path / "nowhere.sfq")], capture_output=True, timeout=60)
        assert p.returncode == 1 and b"-Q" in p.stderr and b"compress" in p.stderr, (args, p.stderr)
        assert b"HIP" not in p.stderr and b"nowhere" not in p.stderr and p.stdout == b""


def test_cli_usage_names_the_switch():
    p = subprocess.run([_cli(), "-h"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"\n-Q illumina8|novaseq4" in p.stdout


def test_quality_map_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata("qmap.hip", tmp_path)
    assert len(meta) == 2, sorted(meta)
    for want in ("k_qmap_count", "k_qmap_apply"):
        assert [k for k in meta if want in k], want
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0 and vgprs <= 128, (name, vgprs, scratch)

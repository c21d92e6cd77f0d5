"""The argument errors of -o ...,merge=PATH (cli.cpp): found before any GPU is touched, and before any output file is opened."""
import subprocess

import pytest

from test_gpu_parity import _cli

REC = b"@r/1\nACGT\n+\nIIII\n@r/2\nACGT\n+\nIIII\n"


def refused(args, tmp_path, outputs, **kw):
    p = subprocess.run([_cli()] + [str(a) for a in args], capture_output=True, **kw)
    assert p.returncode == 1 and b"-o" in p.stderr, (p.returncode, p.stderr)
    for o in outputs:
        assert not (tmp_path / o).exists(), o
    return p.stderr


@pytest.fixture
def files(tmp_path):
    (tmp_path / "r.fq").write_bytes(REC)
    return tmp_path


def test_merge_without_d(files):
    refused(["-o", "merge=" + str(files / "m.fq"), "-u", files / "r.fq", "-f", files / "x.sfq"], files, ["x.sfq", "m.fq"])
    refused(["-s", "-o", "merge=" + str(files / "m.fq"), "-f", files / "nowhere.sfq", "-u", files / "o.txt"], files, ["o.txt", "m.fq"])


def test_merge_without_a_file_name(files):
    for spec in ("merge=", "min=20,merge=", "merge=,hist=" + str(files / "h.tsv")):
        err = refused(["-d", "-o", spec, "-f", files / "nowhere.sfq", "-u", files / "o.fq"], files, ["o.fq", "h.tsv"])
        assert b"merge=" in err and b"no file" in err, err


def test_merge_with_nocut(files):
    for spec in ("nocut,merge=%s", "merge=%s,nocut", "min=20,nocut,merge=%s,mm=1"):
        err = refused(["-d", "-o", spec % (files / "m.fq"), "-f", files / "nowhere.sfq", "-u", files / "o.fq"], files, ["o.fq", "m.fq"])
        assert b"nocut" in err and b"merge=" in err, err


@pytest.mark.parametrize("rng", ["1:10", "0:11", "3:7"])
def test_merge_with_a_range_that_is_no_pairs(files, rng):
    err = refused(["-d", "-R", rng, "-o", "merge=" + str(files / "m.fq"), "-f", files / "nowhere.sfq", "-u", files / "o.fq"], files, ["o.fq", "m.fq"])
    assert b"-W" in err and b"-R" in err, err


def test_a_bad_list_beside_a_merge_leaves_no_file(files):
    err = refused(["-d", "-o", "merge=" + str(files / "m.fq") + ",min=0", "-f", files / "nowhere.sfq", "-u", files / "o.fq"], files, ["o.fq", "m.fq"])
    assert b"min=" in err, err
    err = refused(["-d", "-o", "merge=" + str(files / "m.fq") + ",bogus", "-f", files / "nowhere.sfq", "-u", files / "o.fq"], files, ["o.fq", "m.fq"])
    assert b"bogus" in err, err

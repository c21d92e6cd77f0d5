"""The -o option's argument errors (cli.cpp): found before any GPU is touched, and before any output file is opened."""
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


def test_overlap_without_d(files):
    refused(["-o", "default", "-u", files / "r.fq", "-f", files / "x.sfq"], files, ["x.sfq"])
    refused(["-o", "hist=" + str(files / "h.tsv"), "-u", files / "r.fq", "-f", files / "x.sfq"], files, ["x.sfq", "h.tsv"])


def test_overlap_with_s(files):
    refused(["-s", "-o", "min=20", "-f", files / "nowhere.sfq", "-u", files / "o.txt"], files, ["o.txt"])
    refused(["-o", "min=20", "-s", "-f", files / "nowhere.sfq", "-u", files / "o.txt"], files, ["o.txt"])


@pytest.mark.parametrize("spec, says", [("bogus=1", b"bogus"), ("min=0", b"min="), ("min=600", b"min="), ("pct=101", b"pct="), ("mm=x", b"mm="), ("", b"empty"),
                                        ("default,nocut", b"default"), ("hist=", b"hist="), ("min=20,hist=", b"hist="), ("min=20,,nocut", b"no such term")])
def test_overlap_a_bad_list_of_terms(files, spec, says):
    err = refused(["-d", "-o", spec, "-f", files / "nowhere.sfq", "-u", files / "o.fq"], files, ["o.fq"])
    assert says in err, err


def test_a_bad_list_beside_a_histogram_leaves_no_file(files):
    refused(["-d", "-o", "hist=" + str(files / "h.tsv") + ",min=0", "-f", files / "nowhere.sfq", "-u", files / "o.fq"], files, ["o.fq", "h.tsv"])

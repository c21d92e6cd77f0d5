"""The -k option's argument errors (cli.cpp): found before any GPU is touched, and before any output file is opened."""
import subprocess

import pytest

from test_gpu_parity import _cli

REC = b"@r\nACGT\n+\nIIII\n"


def refused(args, tmp_path, outputs, **kw):
    p = subprocess.run([_cli()] + [str(a) for a in args], capture_output=True, **kw)
    assert p.returncode == 1 and b"-k" in p.stderr, (p.returncode, p.stderr)
    for o in outputs:
        assert not (tmp_path / o).exists(), o


@pytest.fixture
def files(tmp_path):
    (tmp_path / "r.fq").write_bytes(REC)
    return tmp_path


def test_select_without_d(files):
    refused(["-k", "minlen=2", "-u", files / "r.fq", "-f", files / "x.sfq"], files, ["x.sfq"])


def test_select_with_s(files):
    refused(["-s", "-k", "minlen=2", "-f", files / "nowhere.sfq", "-u", files / "o.txt"], files, ["o.txt"])
    refused(["-k", "minlen=2", "-s", "-f", files / "nowhere.sfq", "-u", files / "o.txt"], files, ["o.txt"])


@pytest.mark.parametrize("spec", ["bogus", "minlen", "minlen=", "minlen=x", "minlen=-1", "maxlen=5000000000", "maxn=1.5", "meanq=20.123", "meanq=.5",
                                  "meanq=2e1", "seq=ACGN", "seq=", "seq=" + "ACGT" * 8 + "A", "sample=0", "sample=1", "sample=1.5", "sample=0.5:x",
                                  "sample=-0.5", "minlen=5,maxlen=4", "minlen=2,,maxn=1", "", "rc=1", "minlen=2,bogus"])
def test_select_a_bad_list_of_terms(files, spec):
    refused(["-d", "-k", spec, "-f", files / "nowhere.sfq", "-u", files / "o.fq"], files, ["o.fq"])

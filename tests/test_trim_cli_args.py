"""The -c option's argument errors (cli.cpp): found before any GPU is touched, and before any output file is opened."""
import subprocess

import pytest

from test_gpu_parity import _cli

REC = b"@r\nACGT\n+\nIIII\n"


def refused(args, tmp_path, outputs, **kw):
    p = subprocess.run([_cli()] + [str(a) for a in args], capture_output=True, **kw)
    assert p.returncode == 1 and b"-c" in p.stderr, (p.returncode, p.stderr)
    for o in outputs:
        assert not (tmp_path / o).exists(), o
    return p.stderr


@pytest.fixture
def files(tmp_path):
    (tmp_path / "r.fq").write_bytes(REC)
    return tmp_path


def test_trim_without_d(files):
    refused(["-c", "head=1", "-u", files / "r.fq", "-f", files / "x.sfq"], files, ["x.sfq"])


def test_trim_with_s(files):
    refused(["-s", "-c", "q3=20", "-f", files / "nowhere.sfq", "-u", files / "o.txt"], files, ["o.txt"])
    refused(["-c", "q3=20", "-s", "-f", files / "nowhere.sfq", "-u", files / "o.txt"], files, ["o.txt"])


@pytest.mark.parametrize("spec, says", [("bogus=1", b"bogus"), ("win=40:20", b"win="), ("mm=2", b"mm="), ("adapter=ACGN", b"adapter="), ("", b"empty")])
def test_trim_a_bad_list_of_terms(files, spec, says):
    err = refused(["-d", "-c", spec, "-f", files / "nowhere.sfq", "-u", files / "o.fq"], files, ["o.fq"])
    assert says in err, err

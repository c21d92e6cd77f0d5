"""The -x option's argument errors (cli.cpp): found before any GPU is touched, and before any output file is opened."""
import subprocess

import pytest

from test_gpu_parity import _cli

REC = b"@r\nACGT\n+\nIIII\n"


def refused(args, tmp_path, outputs, **kw):
    p = subprocess.run([_cli()] + [str(a) for a in args], capture_output=True, **kw)
    assert p.returncode == 1 and b"-x" in p.stderr, (p.returncode, p.stderr)
    for o in outputs:
        assert not (tmp_path / o).exists(), o


@pytest.fixture
def files(tmp_path):
    (tmp_path / "r.fq").write_bytes(REC)
    return tmp_path


def test_pick_without_d(files):
    refused(["-x", "fasta", "-u", files / "r.fq", "-f", files / "x.sfq"], files, ["x.sfq"])


def test_pick_an_unknown_word(files):
    refused(["-d", "-x", "bogus", "-f", files / "nowhere.sfq", "-u", files / "o.fa"], files, ["o.fa"])


def test_pick_with_s(files):
    refused(["-s", "-x", "names", "-f", files / "nowhere.sfq", "-u", files / "o.txt"], files, ["o.txt"])
    refused(["-x", "names", "-s", "-f", files / "nowhere.sfq", "-u", files / "o.txt"], files, ["o.txt"])

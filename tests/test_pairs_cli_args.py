"""The -p option's argument errors (cli.cpp): found before any GPU is touched, and before any output file is opened."""
import subprocess

import pytest

from test_gpu_parity import _cli

REC = b"@r\nACGT\n+\nIIII\n"


def refused(args, tmp_path, outputs, **kw):
    p = subprocess.run([_cli()] + [str(a) for a in args], capture_output=True, **kw)
    assert p.returncode == 1 and b"-p" in p.stderr, (p.returncode, p.stderr)
    for o in outputs:
        assert not (tmp_path / o).exists(), o


@pytest.fixture
def files(tmp_path):
    (tmp_path / "r1.fq").write_bytes(REC)
    (tmp_path / "r2.fq").write_bytes(REC)
    return tmp_path


def test_pairs_without_u_on_encode(files):
    refused(["-p", files / "r2.fq", "-f", files / "x.sfq"], files, ["x.sfq"], input=REC)


def test_pairs_without_u_on_decode(files):
    refused(["-d", "-p", files / "o2.fq", "-f", files / "nowhere.sfq"], files, ["o2.fq"])


def test_pairs_with_batch(files):
    jobs = b"%s\t%s\n" % (str(files / "r1.fq").encode(), str(files / "x.sfq").encode())
    refused(["-b", "-p", files / "r2.fq"], files, ["x.sfq"], input=jobs)


def test_pairs_with_a_range(files):
    refused(["-d", "-R", "0:1", "-f", files / "nowhere.sfq", "-u", files / "o1.fq", "-p", files / "o2.fq"], files, ["o1.fq", "o2.fq"])

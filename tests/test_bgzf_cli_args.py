"""The -Z option's refusals (cli.cpp): found before any GPU is touched, and before any output file is opened."""
import subprocess

import pytest

from test_gpu_parity import _cli

REC = b"@r\nACGT\n+\nIIII\n"


def refused(args, tmp_path, outputs, says):
    p = subprocess.run([_cli()] + [str(a) for a in args], capture_output=True)
    assert p.returncode == 1 and b"-Z" in p.stderr and says in p.stderr, (p.returncode, p.stderr)
    for o in outputs:
        assert not (tmp_path / o).exists(), o


@pytest.fixture
def files(tmp_path):
    (tmp_path / "r.fq").write_bytes(REC)
    return tmp_path


def test_bgzf_without_d(files):
    refused(["-Z", "-u", files / "r.fq", "-f", files / "x.sfq"], files, ["x.sfq"], b"goes with -d")


def test_bgzf_with_s(files):
    refused(["-s", "-Z", "-f", files / "nowhere.sfq"], files, [], b"-s writes no text")


def test_bgzf_with_a_range_of_records(files):
    refused(["-d", "-Z", "-R", "0:1", "-f", files / "nowhere.sfq", "-u", files / "o.gz"], files, ["o.gz"], b"does not go with -R")


def test_usage_names_the_switch_and_its_refusal():
    p = subprocess.run([_cli(), "-h"], capture_output=True)
    assert b"-Z  " in p.stdout and b"with -R, which cuts the decoded text on the host" in p.stdout

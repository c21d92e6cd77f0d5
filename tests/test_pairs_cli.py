"""-p on the command line (cli.cpp): two files in, one archive of whole pairs, two files out; every comparison
is exact byte equality."""
import os
import subprocess

import numpy as np
import pytest

from slimfastq_amd import capi
from test_pairs import interleaved, numpy_mapped, records, ILLUMINA8

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


def _info(path):
    out = _run(["-s", "-f", path]).stderr.decode()
    return dict(l.split("=", 1) for l in out.partition("\n:::: Files")[0].replace(" ", "").splitlines() if "=" in l)


@pytest.fixture(scope="module")
def mates():
    """R1 of 50-base reads, R2 of 250-base reads, about 5 MB in all: with -S 1 several slabs, which hold unequal record counts of the
    two files, so both tails are carried"""
    n = 7600
    a, b = capi.synth_fastq(n, 50, seed=70), capi.synth_fastq(n, 250, seed=71)
    assert 4.5e6 < len(a) + len(b) < 6e6 and len(b) > 3 * len(a)
    return a, b


@pytest.fixture
def files(tmp_path, mates):
    (tmp_path / "r1.fq").write_bytes(mates[0])
    (tmp_path / "r2.fq").write_bytes(mates[1])
    return tmp_path


@pytest.mark.parametrize("extra", ([], ["-K", "-Y", "-Q", "illumina8"], ["-B", 0]), ids=("plain", "KYQ", "one_block"))
def test_round_trip(files, mates, extra):
    t = files
    a, b = mates
    p = _run(["-q", "-S", 1, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / "x.sfq"] + extra)
    assert p.returncode == 0, p.stderr
    if "-Q" in extra:
        a, b = numpy_mapped(a, ILLUMINA8), numpy_mapped(b, ILLUMINA8)
    info = _info(t / "x.sfq")
    assert info["usr.pair"] == "1", info                              # -s shows the key
    if 0 not in extra:
        assert int(info["seg.count"]) > 2, info                           # several slabs
    p = _run(["-d", "-f", t / "x.sfq", "-u", t / "o1.fq", "-p", t / "o2.fq"])
    assert p.returncode == 0, p.stderr
    assert (t / "o1.fq").read_bytes() == a and (t / "o2.fq").read_bytes() == b
    # without -p: standard interleaved FASTQ
    p = _run(["-d", "-f", t / "x.sfq"])
    assert p.returncode == 0 and p.stdout == interleaved(a, b), p.stderr
    assert (t / "r1.fq").read_bytes() == mates[0] and (t / "r2.fq").read_bytes() == mates[1]     # the inputs are read, never written


def test_unequal_files(files, mates):
    t = files
    n = len(records(mates[0]))
    (t / "short.fq").write_bytes(b"".join(records(mates[1])[:-1]))
    p = _run(["-q", "-S", 1, "-u", t / "r1.fq", "-p", t / "short.fq", "-f", t / "x.sfq"])
    assert p.returncode == 1 and str(n).encode() in p.stderr and str(n - 1).encode() in p.stderr, p.stderr
    assert not (t / "x.sfq").exists()
    # the other way round, and in one slab
    p = _run(["-q", "-u", t / "short.fq", "-p", t / "r1.fq", "-f", t / "x.sfq"])
    assert p.returncode == 1 and str(n).encode() in p.stderr and str(n - 1).encode() in p.stderr, p.stderr
    assert not (t / "x.sfq").exists()


def test_an_archive_written_without_p(files):
    t = files
    assert _run(["-q", "-u", t / "r1.fq", "-f", t / "plain.sfq"]).returncode == 0
    assert "usr.pair" not in _info(t / "plain.sfq")
    p = _run(["-d", "-f", t / "plain.sfq", "-u", t / "o1.fq", "-p", t / "o2.fq"])
    assert p.returncode == 1 and b"-p" in p.stderr, p.stderr

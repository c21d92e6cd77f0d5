"""-x on the command line (cli.cpp): a decode that writes FASTA, the names, the base lines or the quality lines;
with -R (the host's cut at two lines and at one line a record) and with -p.  Every comparison is exact byte equality."""
import os
import subprocess

import pytest

from slimfastq_amd import capi
from test_pairs import records
from test_pick import picked, FASTA, NAMES, BASES, QUALS

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")
WORDS = {"fasta": FASTA, "names": NAMES, "bases": BASES, "quals": QUALS}


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


@pytest.fixture(scope="module")
def text():
    return capi.synth_fastq(3000, 100, seed=81)


@pytest.fixture(scope="module")
def archive(tmp_path_factory, text):
    """-B 20: records 1000 .. 1036 lie in blocks 50 and 51"""
    t = tmp_path_factory.mktemp("pick_cli")
    (t / "in.fq").write_bytes(text)
    p = _run(["-q", "-K", "-B", 20, "-u", t / "in.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0, p.stderr
    return t / "x.sfq"


@pytest.mark.parametrize("word", sorted(WORDS))
def test_every_selection(tmp_path, archive, text, word):
    p = _run(["-d", "-x", word, "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out").read_bytes() == picked(text, WORDS[word])


@pytest.mark.parametrize("word", ("fasta", "quals"))
def test_with_a_range_of_records(tmp_path, archive, text, word):
    assert 1000 // 20 != 1036 // 20                                   # the range crosses a block border
    p = _run(["-d", "-R", "1000:37", "-x", word, "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out").read_bytes() == picked(text, WORDS[word], 1000, 37)


def test_with_paired_files(tmp_path):
    t = tmp_path
    a, b = capi.synth_fastq(1200, 50, seed=70), capi.synth_fastq(1200, 120, seed=71)
    (t / "r1.fq").write_bytes(a)
    (t / "r2.fq").write_bytes(b)
    p = _run(["-q", "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0, p.stderr
    p = _run(["-d", "-x", "names", "-f", t / "x.sfq", "-u", t / "o1.txt", "-p", t / "o2.txt"])
    assert p.returncode == 0, p.stderr
    assert (t / "o1.txt").read_bytes() == picked(a, NAMES) and (t / "o2.txt").read_bytes() == picked(b, NAMES)
    assert len(records(a)) == 1200
    p = _run(["-d", "-x", "bases", "-W", "100:50", "-f", t / "x.sfq", "-u", t / "w1.txt", "-p", t / "w2.txt"])
    assert p.returncode == 0, p.stderr
    assert (t / "w1.txt").read_bytes() == picked(a, BASES, 100, 50) and (t / "w2.txt").read_bytes() == picked(b, BASES, 100, 50)

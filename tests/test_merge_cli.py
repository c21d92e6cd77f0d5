"""-o ...,merge=PATH on the command line (cli.cpp): a decode that merges the mates of every pair that overlap, against
the Python rule of test_merge.py: the merged records in PATH, the rest in -u (and -p); with -W, -R, -x, -k and hist=, the line on stderr,
and the archives it refuses.  Every comparison is exact byte equality."""
import os
import subprocess

import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Merge, Select
from test_merge import merged
from test_merge_decode import files, split, parts
from test_pairs import records
from test_select import keep, picked

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


def line(rep):
    seen, median = 0, 0
    for ins in range(1, len(rep[11])):
        seen += rep[11][ins]
        if rep[2] and 2 * seen >= rep[2]:
            median = ins
            break
    return "merged %d of %d pairs (%d bases), median insert %d" % (rep[2], rep[0], rep[7], median)


@pytest.fixture(scope="module")
def inter():
    a, b = files()
    return b"".join(x + y for x, y in zip(records(a), records(b)))


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """the pairs of test_merge_decode.py, written with -p: blocks of 64 records, and of 15 (a block may begin at a second mate)"""
    t = tmp_path_factory.mktemp("merge_cli")
    a, b = files()
    (t / "r1.fq").write_bytes(a)
    (t / "r2.fq").write_bytes(b)
    for B in (64, 15):
        p = _run(["-q", "-B", B, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / ("b%d.sfq" % B)])
        assert p.returncode == 0, p.stderr
    return t


def test_the_three_output_files(tmp_path, archives, inter):
    front, rest, rep = parts(inter, Merge())
    assert 0 < rep[2] < rep[0]
    p = _run(["-d", "-o", "merge=%s" % (tmp_path / "m.fq"), "-f", archives / "b64.sfq", "-u", tmp_path / "o1", "-p", tmp_path / "o2"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "m.fq").read_bytes() == front
    assert ((tmp_path / "o1").read_bytes(), (tmp_path / "o2").read_bytes()) == split(rest)
    assert p.stderr.decode().splitlines()[-1] == line(rep)
    p = _run(["-q", "-d", "-o", "default,merge=%s" % (tmp_path / "m2.fq"), "-f", archives / "b15.sfq", "-u", tmp_path / "both"])    # without -p: interleaved
    assert p.returncode == 0 and b"merged" not in p.stderr, p.stderr
    assert (tmp_path / "m2.fq").read_bytes() == front and (tmp_path / "both").read_bytes() == rest
    p = _run(["-q", "-d", "-o", "merge=%s" % (tmp_path / "m2.fq"), "-f", archives / "b64.sfq", "-u", tmp_path / "again"])          # PATH exists: -O overwrites
    assert p.returncode != 0 and not (tmp_path / "again").exists()


def test_the_histogram_and_the_line_speak_of_the_merge(tmp_path, archives, inter):
    m = Merge(min_overlap=12, max_mm=2)
    front, rest, rep = parts(inter, m)
    p = _run(["-d", "-o", "min=12,hist=%s,mm=2,merge=%s" % (tmp_path / "h.tsv", tmp_path / "m.fq"), "-f", archives / "b15.sfq", "-u", tmp_path / "o"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "m.fq").read_bytes() == front and (tmp_path / "o").read_bytes() == rest
    assert p.stderr.decode().splitlines()[-1] == line(rep)
    rows = (tmp_path / "h.tsv").read_text().splitlines()
    assert rows[0] == "insert\tpairs"
    got = {int(r.split("\t")[0]): int(r.split("\t")[1]) for r in rows[1:]}
    assert got == {i: c for i, c in enumerate(rep[11]) if c}
    assert sum(got.values()) == rep[0] - rep[1] and sum(c for i, c in got.items() if i) == rep[2]


def test_with_a_window_of_pairs_and_a_range_of_records(tmp_path, archives, inter):
    rs = records(inter)
    front, rest, rep = parts(b"".join(rs[16:96]), Merge())
    p = _run(["-d", "-W", "8:40", "-o", "merge=%s" % (tmp_path / "m.fq"), "-f", archives / "b15.sfq", "-u", tmp_path / "w1", "-p", tmp_path / "w2"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "m.fq").read_bytes() == front and ((tmp_path / "w1").read_bytes(), (tmp_path / "w2").read_bytes()) == split(rest)
    assert p.stderr.decode().splitlines()[-1] == line(rep)
    front, rest, rep = parts(b"".join(rs[20:42]), Merge())            # a range of whole pairs that begins inside a block
    p = _run(["-d", "-R", "20:22", "-o", "merge=%s" % (tmp_path / "r.fq"), "-f", archives / "b15.sfq", "-u", tmp_path / "r"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "r.fq").read_bytes() == front and (tmp_path / "r").read_bytes() == rest
    assert p.stderr.decode().splitlines()[-1] == line(rep)


def test_with_a_pick_and_a_selection(tmp_path, archives, inter):
    front, rest, _ = parts(inter, Merge())
    ra, rb = split(rest)
    p = _run(["-q", "-d", "-x", "fasta", "-o", "merge=%s" % (tmp_path / "m.fa"), "-f", archives / "b64.sfq", "-u", tmp_path / "o1", "-p", tmp_path / "o2"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "m.fa").read_bytes() == picked(front, capi.PICK_FASTA)                                                       # -x applies to PATH too
    assert ((tmp_path / "o1").read_bytes(), (tmp_path / "o2").read_bytes()) == (picked(ra, capi.PICK_FASTA), picked(rb, capi.PICK_FASTA))
    kept = keep(inter, Select(motif=b"ACGT", pairs=capi.SELECT_EITHER))
    front, rest, _ = parts(kept, Merge())
    p = _run(["-q", "-d", "-k", "seq=ACGT,either", "-o", "merge=%s" % (tmp_path / "k.fq"), "-f", archives / "b64.sfq", "-u", tmp_path / "k"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "k.fq").read_bytes() == front and (tmp_path / "k").read_bytes() == rest


def test_an_archive_with_an_odd_segment_is_refused(tmp_path, inter):
    (tmp_path / "odd.fq").write_bytes(b"".join(records(inter)[:7]))
    assert _run(["-q", "-u", tmp_path / "odd.fq", "-f", tmp_path / "odd.sfq"]).returncode == 0
    p = _run(["-d", "-o", "merge=%s" % (tmp_path / "m.fq"), "-f", tmp_path / "odd.sfq", "-u", tmp_path / "out"])
    assert p.returncode != 0 and b"-o" in p.stderr and b"not whole pairs" in p.stderr, p.stderr
    assert not (tmp_path / "out").exists() and not (tmp_path / "m.fq").exists()

"""-o on the command line (cli.cpp): a decode that overlaps the mates of every pair, against the Python rule of
test_overlap.py and the library's own result; with -p, -R and hist=, the line on stderr, and the archives it refuses.  Every comparison
is exact byte equality."""
import os
import subprocess

import pytest

from slimfastq_amd.capi import Overlap
from test_overlap import Buf, fields, overlapped
from test_overlap_decode import files, split
from test_pairs import records

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


def line(rep):
    seen, median = 0, 0
    for ins in range(1, len(rep[9])):
        seen += rep[9][ins]
        if rep[2] and 2 * seen >= rep[2]:
            median = ins
            break
    return "overlapped %d of %d pairs, cut %d (%d bases removed), median insert %d" % (rep[2], rep[0], rep[3], rep[6] - rep[7], median)


@pytest.fixture(scope="module")
def inter():
    a, b = files()
    return b"".join(x + y for x, y in zip(records(a), records(b)))


@pytest.fixture(scope="module")
def archives(tmp_path_factory):
    """the pairs of test_overlap_decode.py, written with -p: blocks of 64 records, and of 15 (a block may begin at a second mate)"""
    t = tmp_path_factory.mktemp("overlap_cli")
    a, b = files()
    (t / "r1.fq").write_bytes(a)
    (t / "r2.fq").write_bytes(b)
    for B in (64, 15):
        p = _run(["-q", "-B", B, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / ("b%d.sfq" % B)])
        assert p.returncode == 0, p.stderr
    return t


def test_the_default_rule_is_the_librarys_result(ctx, tmp_path, archives, inter):
    want, rep, _ = overlapped(inter, Overlap())
    T, out = Buf(len(inter), 0, inter), Buf(len(inter), 0)
    n, lib_rep = ctx.overlap_pairs(T.ptr, len(inter), Overlap(), out.ptr, out.n)
    assert out.back("the output")[:n] == want and fields(lib_rep) == rep and 0 < rep[3] < rep[2] < rep[0]
    p = _run(["-d", "-o", "default", "-f", archives / "b64.sfq", "-u", tmp_path / "o1", "-p", tmp_path / "o2"])
    assert p.returncode == 0, p.stderr
    assert ((tmp_path / "o1").read_bytes(), (tmp_path / "o2").read_bytes()) == split(want)
    assert p.stderr.decode().splitlines()[-1] == line(rep)
    p = _run(["-q", "-d", "-o", "default", "-f", archives / "b64.sfq", "-u", tmp_path / "both"])
    assert p.returncode == 0 and b"overlapped" not in p.stderr and (tmp_path / "both").read_bytes() == want


def test_the_histogram_file_sums_to_the_report(tmp_path, archives, inter):
    o = Overlap(min_overlap=12, max_mm=2)
    want, rep, _ = overlapped(inter, o)
    p = _run(["-d", "-o", "min=12,hist=%s,mm=2" % (tmp_path / "h.tsv"), "-f", archives / "b15.sfq", "-u", tmp_path / "o"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "o").read_bytes() == want and p.stderr.decode().splitlines()[-1] == line(rep)
    rows = (tmp_path / "h.tsv").read_text().splitlines()
    assert rows[0] == "insert\tpairs"
    got = {int(r.split("\t")[0]): int(r.split("\t")[1]) for r in rows[1:]}
    assert got == {i: c for i, c in enumerate(rep[9]) if c}
    assert sum(got.values()) == rep[0] - rep[1] and sum(c for i, c in got.items() if i) == rep[2]
    p = _run(["-q", "-d", "-o", "hist=%s" % (tmp_path / "d.tsv"), "-f", archives / "b64.sfq", "-u", tmp_path / "d"])      # hist= alone: the default rule
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "d").read_bytes() == overlapped(inter, Overlap())[0] and (tmp_path / "d.tsv").exists()


def test_nocut_writes_what_a_plain_decode_writes(tmp_path, archives, inter):
    p = _run(["-q", "-d", "-f", archives / "b64.sfq", "-u", tmp_path / "plain"])
    assert p.returncode == 0, p.stderr
    p = _run(["-d", "-o", "nocut", "-f", archives / "b64.sfq", "-u", tmp_path / "counted"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "counted").read_bytes() == (tmp_path / "plain").read_bytes() == inter
    rep = overlapped(inter, Overlap(cut=0))[1]
    assert p.stderr.decode().splitlines()[-1] == line(rep) and rep[6] == rep[7]


def test_with_a_range_of_records(tmp_path, archives, inter):
    """the pairs are the archive's: a window of blocks that begins at a second mate is searched from its second record on"""
    want = records(overlapped(inter, Overlap())[0])
    p = _run(["-q", "-d", "-R", "20:21", "-o", "default", "-f", archives / "b15.sfq", "-u", tmp_path / "r"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "r").read_bytes() == b"".join(want[20:41])
    p = _run(["-q", "-d", "-W", "8:40", "-o", "default", "-f", archives / "b15.sfq", "-u", tmp_path / "w1", "-p", tmp_path / "w2"])
    assert p.returncode == 0, p.stderr
    assert ((tmp_path / "w1").read_bytes(), (tmp_path / "w2").read_bytes()) == split(b"".join(want[16:96]))


def test_an_archive_with_an_odd_segment_is_refused(tmp_path, inter):
    (tmp_path / "odd.fq").write_bytes(b"".join(records(inter)[:7]))
    assert _run(["-q", "-u", tmp_path / "odd.fq", "-f", tmp_path / "odd.sfq"]).returncode == 0
    p = _run(["-d", "-o", "default", "-f", tmp_path / "odd.sfq", "-u", tmp_path / "out"])
    assert p.returncode != 0 and b"-o" in p.stderr and b"not whole pairs" in p.stderr, p.stderr
    assert not (tmp_path / "out").exists()

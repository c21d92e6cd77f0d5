"""-D on the command line (cli.cpp): a decode that writes the first record of every base line, against the Python
rule of test_dedup.py over the WHOLE file -- the archive has several segments and the duplicates lie more than 1 MiB apart, so the
set that lasts the run is what finds them; with -p, -W, -R, -x, -k and -q, and the line on stderr.  Every comparison is exact byte
equality."""
import os
import subprocess

import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Dedup, Merge, Overlap, Select, Trim
from test_dedup_decode import dd, planted
from test_merge_decode import parts
from test_overlap import overlapped
from test_pairs import records
from test_select import keep, picked
from test_trim import trimmed

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


@pytest.fixture(scope="module")
def text():
    """14 000 reads of 100 bases; records 7500 + i, i even below 5000, repeat the bases of record i in lower case: 1.8 MB apart"""
    rs = [r.split(b"\n") for r in records(capi.synth_fastq(14000, 100, seed=91))]
    for i in range(0, 5000, 2):
        rs[7500 + i][1] = rs[i][1].lower()
    fq = b"".join(b"\n".join(r) for r in rs)
    assert len(fq) > 3 << 20 and sum(len(b"\n".join(r)) for r in rs[:7500]) > 1 << 20
    return fq


@pytest.fixture(scope="module")
def archive(tmp_path_factory, text):
    """-S 1: a segment per MiB of text"""
    t = tmp_path_factory.mktemp("dedup_cli")
    (t / "in.fq").write_bytes(text)
    p = _run(["-q", "-K", "-S", 1, "-u", t / "in.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0, p.stderr
    info = dict(l.split("=", 1) for l in _run(["-s", "-f", t / "x.sfq"]).stderr.decode().replace(" ", "").splitlines() if "=" in l)
    assert int(info["seg.count"]) >= 3                                # the duplicates lie in other segments than their first occurrences
    return t / "x.sfq"


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    t = tmp_path_factory.mktemp("dedup_cli_pairs")
    a, b, inter = planted()
    (t / "r1.fq").write_bytes(a)
    (t / "r2.fq").write_bytes(b)
    p = _run(["-q", "-B", 64, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0, p.stderr
    return inter, t / "x.sfq"


def line(kept, units, what="reads"):
    return "kept %d of %d %s (%d duplicates, %.2f %%)" % (kept, units, what, units - kept, 100.0 * (units - kept) / units)


def split(fq):
    rs = records(fq)
    return b"".join(rs[0::2]), b"".join(rs[1::2])


def test_the_whole_archive_and_the_line_on_stderr(tmp_path, archive, text):
    p = _run(["-d", "-D", "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    want = dd(text)
    assert len(records(want)) == 14000 - 2500 and (tmp_path / "out").read_bytes() == want
    assert p.stderr.decode().splitlines()[-1] == line(11500, 14000) == "kept 11500 of 14000 reads (2500 duplicates, 17.86 %)"
    p = _run(["-q", "-d", "-D", "-f", archive, "-u", tmp_path / "quiet"])
    assert p.returncode == 0 and b"kept" not in p.stderr and (tmp_path / "quiet").read_bytes() == want


def test_with_a_range_of_records(tmp_path, archive, text):
    p = _run(["-d", "-D", "-R", "1001:9000", "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    want = dd(text, Dedup(first_record=1001, n_records=9000))
    assert (tmp_path / "out").read_bytes() == want and 0 < 9000 - len(records(want)) < 2500
    assert p.stderr.decode().splitlines()[-1] == line(len(records(want)), 9000)


def test_with_picked_lines(tmp_path, archive, text):
    p = _run(["-d", "-D", "-x", "fasta", "-f", archive, "-u", tmp_path / "out.fa"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.fa").read_bytes() == picked(dd(text), capi.PICK_FASTA)


def test_behind_a_selection(tmp_path, archive, text):
    # -k in front: a duplicate whose first occurrence -k dropped is a first occurrence
    p = _run(["-d", "-D", "-k", "meanq=27.5,minlen=100", "-f", archive, "-u", tmp_path / "k"])
    assert p.returncode == 0, p.stderr
    kept = keep(text, Select(min_mean_q_x100=2750, min_len=100))
    want = dd(kept)
    assert (tmp_path / "k").read_bytes() == want and want != keep(dd(text), Select(min_mean_q_x100=2750, min_len=100))
    err = p.stderr.decode().splitlines()
    assert err[-1] == line(len(records(want)), len(records(kept))) and err[-2].startswith("kept %d of 14000 records" % len(records(kept)))
    p = _run(["-d", "-D", "-k", "minlen=101", "-f", archive, "-u", tmp_path / "none"])
    assert p.returncode == 0 and (tmp_path / "none").read_bytes() == b"" and p.stderr.decode().splitlines()[-1] == "kept 0 of 0 reads (0 duplicates, 0.00 %)"


def test_with_paired_files(tmp_path, pairs):
    inter, arch = pairs
    want = dd(inter, Dedup(pairs=1))
    n = len(records(want)) // 2
    assert 600 < n < 900
    p = _run(["-d", "-D", "-f", arch, "-u", tmp_path / "o1", "-p", tmp_path / "o2"])
    assert p.returncode == 0, p.stderr
    assert ((tmp_path / "o1").read_bytes(), (tmp_path / "o2").read_bytes()) == split(want)
    assert p.stderr.decode().splitlines()[-1] == line(n, 1200, "pairs")
    # without -p: the interleaved text, whole pairs all the same
    p = _run(["-d", "-D", "-f", arch, "-u", tmp_path / "both"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "both").read_bytes() == want and p.stderr.decode().splitlines()[-1] == line(n, 1200, "pairs")
    # -W: the window's pairs alone are judged
    win = dd(b"".join(records(inter)[200:1800]), Dedup(pairs=1))
    p = _run(["-d", "-D", "-W", "100:800", "-f", arch, "-u", tmp_path / "w1", "-p", tmp_path / "w2"])
    assert p.returncode == 0, p.stderr
    assert ((tmp_path / "w1").read_bytes(), (tmp_path / "w2").read_bytes()) == split(win)
    assert p.stderr.decode().splitlines()[-1] == line(len(records(win)) // 2, 800, "pairs")
    p = _run(["-d", "-D", "-x", "names", "-f", arch, "-u", tmp_path / "n1", "-p", tmp_path / "n2"])
    assert p.returncode == 0, p.stderr
    assert ((tmp_path / "n1").read_bytes(), (tmp_path / "n2").read_bytes()) == tuple(picked(x, capi.PICK_NAMES) for x in split(want))


def test_behind_a_trim_and_the_overlap_cut(tmp_path, pairs):
    inter, arch = pairs
    d = Dedup(pairs=1)
    # -c in front: pairs that differ in their last bases alone are duplicates behind it
    t_text = trimmed(inter, Trim(tail=2))[0]
    want = dd(t_text, d)
    assert len(records(want)) < len(records(dd(inter, d)))
    p = _run(["-d", "-D", "-c", "tail=2", "-f", arch, "-u", tmp_path / "c"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "c").read_bytes() == want and p.stderr.decode().splitlines()[-1] == line(len(records(want)) // 2, 1200, "pairs")
    # -o in front: the cut mates are the keys
    want = dd(overlapped(inter, Overlap())[0], d)
    p = _run(["-q", "-d", "-D", "-o", "default", "-f", arch, "-u", tmp_path / "o1", "-p", tmp_path / "o2"])
    assert p.returncode == 0, p.stderr
    assert ((tmp_path / "o1").read_bytes(), (tmp_path / "o2").read_bytes()) == split(want)


def test_in_front_of_the_merge_with_a_range(tmp_path, pairs):
    """-R cuts inside the first block and -D drops pairs in front of the merge: the merge takes the whole text it is handed"""
    inter, arch = pairs
    rs = records(inter)
    for a, n in ((0, 2400), (10, 1600), (200, 2200)):
        kept = dd(b"".join(rs[a:a + n]), Dedup(pairs=1))
        front, rest, rep = parts(kept, Merge())
        assert 0 < len(front) and 0 < len(rest) and len(records(kept)) < n
        p = _run(["-d", "-O", "-D", "-R", "%d:%d" % (a, n), "-o", "merge=%s" % (tmp_path / "m.fq"), "-f", arch, "-u", tmp_path / "r"])
        assert p.returncode == 0, p.stderr
        assert ((tmp_path / "m.fq").read_bytes(), (tmp_path / "r").read_bytes()) == (front, rest), (a, n)
        assert p.stderr.decode().splitlines()[-1] == line(len(records(kept)) // 2, n // 2, "pairs")
    # without -R, and split
    front, rest, _ = parts(dd(inter, Dedup(pairs=1)), Merge())
    p = _run(["-q", "-d", "-O", "-D", "-o", "merge=%s" % (tmp_path / "m.fq"), "-f", arch, "-u", tmp_path / "o1", "-p", tmp_path / "o2"])
    assert p.returncode == 0, p.stderr
    assert ((tmp_path / "m.fq").read_bytes(), (tmp_path / "o1").read_bytes(), (tmp_path / "o2").read_bytes()) == (front,) + split(rest)


def test_where_it_does_not_go(tmp_path, archive, text):
    (tmp_path / "in.fq").write_bytes(text[:10000])
    p = _run(["-D", "-u", tmp_path / "in.fq", "-f", tmp_path / "x.sfq"])
    assert p.returncode == 1 and b"-D" in p.stderr and not (tmp_path / "x.sfq").exists()
    p = _run(["-s", "-D", "-f", archive])
    assert p.returncode == 1 and b"-D" in p.stderr

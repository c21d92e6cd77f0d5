"""-c on the command line (cli.cpp): a decode that writes trimmed records, against the Python rule of test_trim.py;
with -R, -k, -x, -p and -W, an archive of several segments, and the line on stderr.  Every comparison is exact byte equality."""
import os
import subprocess

import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Select, Trim
from test_pairs import records
from test_select import keep, picked
from test_trim import trimmed

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")

SPEC = "head=1,q5=35,q3=20,win=4:17.25,adapter=agatcggaagagc,mm=1"
RULE = dict(head=1, lead_q=35, trail_q=20, win_len=4, win_q_x100=1725, adapter=b"AGATCGGAAGAGC", adapter_mm=1, adapter_min=3)


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


def line(rep):
    return "trimmed %d of %d records, %d to nothing (%d of %d bases left)" % (rep[1], rep[0], rep[2], rep[6], rep[5])


@pytest.fixture(scope="module")
def text():
    return capi.synth_fastq(3000, 100, seed=81)


@pytest.fixture(scope="module")
def whole(text):
    """the whole text trimmed by RULE, and the report"""
    return trimmed(text, Trim(**RULE))


@pytest.fixture(scope="module")
def archive(tmp_path_factory, text):
    """-B 20: records 1000 .. 1036 lie in blocks 50 and 51; -K: the blocks' checksums are those of the untrimmed text"""
    t = tmp_path_factory.mktemp("trim_cli")
    (t / "in.fq").write_bytes(text)
    p = _run(["-q", "-K", "-B", 20, "-u", t / "in.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0, p.stderr
    return t / "x.sfq"


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    t = tmp_path_factory.mktemp("trim_cli_pairs")
    a, b = capi.synth_fastq(1200, 50, seed=70), capi.synth_fastq(1200, 120, seed=71)
    (t / "r1.fq").write_bytes(a)
    (t / "r2.fq").write_bytes(b)
    p = _run(["-q", "-B", 64, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0, p.stderr
    return a, b, t / "x.sfq"


def test_the_whole_archive_and_the_line_on_stderr(tmp_path, archive, text, whole):
    want, rep = whole
    p = _run(["-d", "-c", SPEC, "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    assert 0 < rep[2] < 3000 and (tmp_path / "out").read_bytes() == want
    assert p.stderr.decode().splitlines()[-1] == line(rep)
    p = _run(["-q", "-d", "-c", SPEC, "-f", archive, "-u", tmp_path / "quiet"])
    assert p.returncode == 0 and b"trimmed" not in p.stderr and (tmp_path / "quiet").read_bytes() == want


def test_with_a_range_of_records(tmp_path, archive, text, whole):
    """without -k the host cuts the window's blocks to the records: they keep their four lines, so the cut still finds them"""
    assert 1000 // 20 != 1036 // 20                                   # the range crosses a block border
    rs = records(whole[0])
    p = _run(["-d", "-R", "1000:37", "-c", SPEC, "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out").read_bytes() == b"".join(rs[1000:1037])
    p = _run(["-d", "-R", "1000:37", "-c", "maxlen=0", "-f", archive, "-u", tmp_path / "empty"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "empty").read_bytes() == b"".join(records(trimmed(text, Trim(max_len=0))[0])[1000:1037])
    p = _run(["-d", "-R", "1000:37", "-c", SPEC, "-x", "bases", "-f", archive, "-u", tmp_path / "b"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "b").read_bytes() == picked(b"".join(rs[1000:1037]), capi.PICK_BASES)


def test_with_a_selection_and_picked_lines(tmp_path, archive, text, whole):
    want, rep = whole
    s = Select(min_len=50, max_n=1)
    kept = keep(want, s)
    assert 0 < len(kept) < len(want) and keep(text, s) != kept       # the trimmed length decides
    p = _run(["-d", "-c", SPEC, "-k", "minlen=50,maxn=1", "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out").read_bytes() == kept
    err = p.stderr.decode().splitlines()
    assert err[-2] == line(rep) and err[-1].startswith("kept %d of 3000 records" % len(records(kept)))
    p = _run(["-d", "-k", "minlen=50,maxn=1", "-x", "fasta", "-c", SPEC, "-f", archive, "-u", tmp_path / "out.fa"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.fa").read_bytes() == picked(kept, capi.PICK_FASTA)
    p = _run(["-d", "-R", "1000:37", "-c", SPEC, "-k", "minlen=50", "-f", archive, "-u", tmp_path / "r"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "r").read_bytes() == keep(want, Select(first_record=1000, n_records=37, min_len=50))


def test_with_paired_files(tmp_path, pairs):
    a, b, arch = pairs
    t = Trim(**RULE)
    (ta, repa), (tb, repb) = trimmed(a, t), trimmed(b, t)
    p = _run(["-d", "-c", SPEC, "-f", arch, "-u", tmp_path / "o1", "-p", tmp_path / "o2"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "o1").read_bytes() == ta and (tmp_path / "o2").read_bytes() == tb
    assert p.stderr.decode().splitlines()[-1] == line([x + y for x, y in zip(repa[:7], repb[:7])])
    # without -p: the interleaved text
    p = _run(["-q", "-d", "-c", SPEC, "-f", arch, "-u", tmp_path / "both"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "both").read_bytes() == b"".join(x + y for x, y in zip(records(ta), records(tb)))
    # -W: a window of pairs
    p = _run(["-q", "-d", "-W", "100:450", "-c", SPEC, "-f", arch, "-u", tmp_path / "w1", "-p", tmp_path / "w2"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "w1").read_bytes() == b"".join(records(ta)[100:550]) and (tmp_path / "w2").read_bytes() == b"".join(records(tb)[100:550])
    # ... selected by the trimmed lengths, both mates
    p = _run(["-q", "-d", "-c", SPEC, "-k", "minlen=30", "-f", arch, "-u", tmp_path / "k1", "-p", tmp_path / "k2"])
    assert p.returncode == 0, p.stderr
    ok = [i for i, (x, y) in enumerate(zip(records(ta), records(tb))) if len(x.split(b"\n")[1]) >= 30 and len(y.split(b"\n")[1]) >= 30]
    assert 0 < len(ok) < 1200
    assert (tmp_path / "k1").read_bytes() == b"".join(records(ta)[i] for i in ok) and (tmp_path / "k2").read_bytes() == b"".join(records(tb)[i] for i in ok)


def test_an_archive_of_several_segments(tmp_path):
    fq = capi.synth_fastq(14000, 100, seed=12)
    assert len(fq) > 3 << 20
    (tmp_path / "in.fq").write_bytes(fq)
    assert _run(["-q", "-S", 1, "-u", tmp_path / "in.fq", "-f", tmp_path / "seg.sfq"]).returncode == 0
    assert b"seg.count" in _run(["-s", "-f", tmp_path / "seg.sfq"]).stderr      # (the archive does hold several segments)
    want, rep = trimmed(fq, Trim(tail=5, trail_q=20))
    p = _run(["-d", "-c", "tail=5,q3=20", "-f", tmp_path / "seg.sfq", "-u", tmp_path / "seg.fq"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "seg.fq").read_bytes() == want
    assert p.stderr.decode().splitlines()[-1] == line(rep)            # summed over the segments

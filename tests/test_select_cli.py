"""-k on the command line (cli.cpp): a decode that writes the records a filter keeps, against the Python rule of
test_select.py; with -R, -p, -W, -x and -K, the line on stderr, nothing kept, and a sample that does not depend on how the archive
was cut into segments.  Every comparison is exact byte equality."""
import os
import subprocess

import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Select
from test_pairs import records
from test_select import keep, picked, selected

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


@pytest.fixture(scope="module")
def text():
    return capi.synth_fastq(3000, 100, seed=81)


@pytest.fixture(scope="module")
def archive(tmp_path_factory, text):
    """-B 20: records 1000 .. 1036 lie in blocks 50 and 51; -K: the blocks' checksums are those of the whole text"""
    t = tmp_path_factory.mktemp("select_cli")
    (t / "in.fq").write_bytes(text)
    p = _run(["-q", "-K", "-B", 20, "-u", t / "in.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0, p.stderr
    return t / "x.sfq"


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    t = tmp_path_factory.mktemp("select_cli_pairs")
    a, b = capi.synth_fastq(1200, 50, seed=70), capi.synth_fastq(1200, 120, seed=71)
    (t / "r1.fq").write_bytes(a)
    (t / "r2.fq").write_bytes(b)
    p = _run(["-q", "-B", 64, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0, p.stderr
    return a, b, t / "x.sfq"


SPEC = "meanq=27.5,seq=acg,rc,sample=0.75:9"
RULE = dict(min_mean_q_x100=2750, motif=b"ACG", motif_rc=True, sample=0xC0000000, sample_seed=9)


def test_the_whole_archive_and_the_line_on_stderr(tmp_path, archive, text):
    p = _run(["-d", "-k", SPEC, "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    want = keep(text, Select(**RULE))
    assert 0 < len(want) < len(text) and (tmp_path / "out").read_bytes() == want
    assert p.stderr.decode().splitlines()[-1] == "kept %d of 3000 records (%d of %d bytes)" % (len(records(want)), len(want), len(text))
    p = _run(["-q", "-d", "-k", SPEC, "-f", archive, "-u", tmp_path / "quiet"])
    assert p.returncode == 0 and b"kept" not in p.stderr and (tmp_path / "quiet").read_bytes() == want


def test_with_a_range_of_records(tmp_path, archive, text):
    assert 1000 // 20 != 1036 // 20                                   # the range crosses a block border
    p = _run(["-d", "-R", "1000:37", "-k", "maxn=0,invert", "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    want = keep(text, Select(first_record=1000, n_records=37, max_n=0, invert=True))
    assert (tmp_path / "out").read_bytes() == want
    assert b"kept %d of 37 records" % len(records(want)) in p.stderr
    # the sample counts records from the archive's first: a range is a cut of the whole selection
    p = _run(["-d", "-R", "990:400", "-k", "sample=0.5:3", "-f", archive, "-u", tmp_path / "s"])
    assert p.returncode == 0, p.stderr
    want = keep(text, Select(first_record=990, n_records=400, sample=1 << 31, sample_seed=3))
    assert 100 < len(records(want)) < 300 and (tmp_path / "s").read_bytes() == want


def test_with_picked_lines(tmp_path, archive, text):
    p = _run(["-d", "-x", "fasta", "-k", SPEC, "-f", archive, "-u", tmp_path / "out.fa"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.fa").read_bytes() == picked(keep(text, Select(**RULE)), capi.PICK_FASTA)
    p = _run(["-d", "-x", "quals", "-R", "1000:37", "-k", "minlen=100", "-f", archive, "-u", tmp_path / "q"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "q").read_bytes() == picked(keep(text, Select(first_record=1000, n_records=37, min_len=100)), capi.PICK_QUALS)


def test_nothing_kept(tmp_path, archive, pairs):
    p = _run(["-d", "-k", "minlen=101", "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out").read_bytes() == b"" and b"kept 0 of 3000 records (0 of " in p.stderr
    p = _run(["-d", "-k", "minlen=1000", "-f", pairs[2], "-u", tmp_path / "o1", "-p", tmp_path / "o2"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "o1").read_bytes() == b"" and (tmp_path / "o2").read_bytes() == b""


def mates(a, b, sel):
    ra, rb = records(a), records(b)
    inter = b"".join(x + y for x, y in zip(ra, rb))
    kept = selected(inter, sel)[0]
    return inter, kept, b"".join(ra[r // 2] for r in kept[0::2]), b"".join(rb[r // 2] for r in kept[1::2])


@pytest.mark.parametrize("either", [False, True])
def test_with_paired_files(tmp_path, pairs, either):
    a, b, arch = pairs
    spec = "meanq=27.8" + (",either" if either else "")
    mode = capi.SELECT_EITHER if either else capi.SELECT_BOTH
    inter, kept, wa, wb = mates(a, b, Select(min_mean_q_x100=2780, pairs=mode))
    assert 0 < len(kept) < 2400
    p = _run(["-d", "-k", spec, "-f", arch, "-u", tmp_path / "o1", "-p", tmp_path / "o2"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "o1").read_bytes() == wa and (tmp_path / "o2").read_bytes() == wb
    # without -p: the interleaved text, whole pairs all the same
    p = _run(["-d", "-k", spec, "-f", arch, "-u", tmp_path / "both"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "both").read_bytes() == b"".join(records(inter)[r] for r in kept)
    # -W: a window of pairs; its sample is the whole archive's
    _, keptw, wa, wb = mates(a, b, Select(min_mean_q_x100=2780, pairs=mode, first_record=200, n_records=900, sample=0xA0000000, sample_seed=2))
    assert 0 < len(keptw) < 900
    p = _run(["-d", "-W", "100:450", "-k", spec + ",sample=0.625:2", "-f", arch, "-u", tmp_path / "w1", "-p", tmp_path / "w2"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "w1").read_bytes() == wa and (tmp_path / "w2").read_bytes() == wb


def test_either_on_an_archive_that_is_not_paired(tmp_path, archive):
    p = _run(["-d", "-k", "maxn=0,either", "-f", archive, "-u", tmp_path / "out"])
    assert p.returncode == 1 and b"-k" in p.stderr and not (tmp_path / "out").exists()


def test_a_sample_does_not_depend_on_the_segments(tmp_path):
    fq = capi.synth_fastq(14000, 100, seed=12)
    assert len(fq) > 3 << 20
    (tmp_path / "in.fq").write_bytes(fq)
    assert _run(["-q", "-S", 1, "-u", tmp_path / "in.fq", "-f", tmp_path / "seg.sfq"]).returncode == 0
    assert _run(["-q", "-u", tmp_path / "in.fq", "-f", tmp_path / "whole.sfq"]).returncode == 0
    out = []
    for name in ("seg", "whole"):
        p = _run(["-d", "-k", "sample=0.3:5", "-f", tmp_path / (name + ".sfq"), "-u", tmp_path / (name + ".fq")])
        assert p.returncode == 0, p.stderr
        out.append((tmp_path / (name + ".fq")).read_bytes())
    want = keep(fq, Select(sample=int(0.3 * 2 ** 32), sample_seed=5))
    assert out[0] == want and out[1] == want
    s = _run(["-s", "-f", tmp_path / "seg.sfq"]).stderr
    assert b"seg.count" in s                                          # (the archive does hold several segments)

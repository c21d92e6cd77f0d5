"""-Z on the command line (cli.cpp): a decode whose files are BGZF.  Every file a -d -Z run writes passes
bgzf_check.py, ends in the end-of-file block and inflates to the file the same run writes without -Z: -u, -u with -p, -W, -x fasta,
merge=, the sample files of -X (named .fastq.gz); archives of several segments, so that several calls append to one file; a -k that
keeps nothing writes the 28 bytes of the end-of-file block alone."""
import os
import subprocess

import numpy as np
import pytest

from slimfastq_amd import capi
import bgzf_check

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")
NAMES = ["alpha", "beta", "gamma"]
ROWS = [b"ATCACGTT", b"TTAGGCAA", b"CGATGTCC"]


def _run(args, **kw):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)
    assert p.returncode == 0, p.stderr
    return p


def inflated(path):
    """the text of a BGZF file: members that chain to the file's end (a call's last member may be short), the last of them the
    end-of-file block and no other empty; gzip's own reader agrees"""
    import gzip
    raw = path.read_bytes()
    assert raw[-28:] == bgzf_check.EOF, "%s does not end in the end-of-file block" % path
    ms = bgzf_check.members(raw)
    assert all(len(m[3]) > 0 for m in ms[:-1]) and ms[-1][3] == b""
    text = b"".join(m[3] for m in ms)
    assert gzip.decompress(raw) == text
    return text


def walk_calls(path):
    """members of under 65280 bytes inside a file are the ends of calls: count them"""
    return sum(1 for m in bgzf_check.members(path.read_bytes()[:-28]) if len(m[3]) < bgzf_check.PIECE)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    t = tmp_path_factory.mktemp("bgzf_cli")
    fq = capi.synth_fastq(12000, 100, seed=31)
    assert len(fq) > (2 << 20)                                          # more than one segment at -S 1
    (t / "one.fq").write_bytes(fq)
    _run(["-q", "-S", 1, "-B", 500, "-u", t / "one.fq", "-f", t / "one.sfq"])
    from test_merge_decode import files
    a, b = files("mixed")
    (t / "r1.fq").write_bytes(a)
    (t / "r2.fq").write_bytes(b)
    _run(["-q", "-B", 100, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / "two.sfq"])
    return t


def test_one_file_of_several_calls(tmp_path, world):
    p = subprocess.run([CLI, "-d", "-Z", "-f", str(world / "one.sfq"), "-u", str(tmp_path / "o.fastq.gz")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr
    text = (world / "one.fq").read_bytes()
    assert inflated(tmp_path / "o.fastq.gz") == text
    assert walk_calls(tmp_path / "o.fastq.gz") >= 2                     # a short last member per call
    last = p.stderr.decode().strip().splitlines()[-1]
    assert last.startswith("deflated %d bytes of text to %d bytes in " % (len(text), (tmp_path / "o.fastq.gz").stat().st_size - 28)), last
    # gzip's own reader, EOF block and all
    import gzip
    assert gzip.decompress((tmp_path / "o.fastq.gz").read_bytes()) == text


def test_fasta_and_nothing_kept(tmp_path, world):
    _run(["-q", "-d", "-x", "fasta", "-f", world / "one.sfq", "-u", tmp_path / "plain.fa"])
    _run(["-q", "-d", "-Z", "-x", "fasta", "-f", world / "one.sfq", "-u", tmp_path / "z.fa.gz"])
    assert inflated(tmp_path / "z.fa.gz") == (tmp_path / "plain.fa").read_bytes()
    _run(["-q", "-d", "-Z", "-k", "minlen=100000", "-f", world / "one.sfq", "-u", tmp_path / "none.gz"])
    assert (tmp_path / "none.gz").read_bytes() == bgzf_check.EOF


def test_pairs_window_and_merge(tmp_path, world):
    t = tmp_path
    for tag, extra in (("p", []), ("w", ["-W", "130:200"])):
        _run(["-q", "-d"] + extra + ["-f", world / "two.sfq", "-u", t / (tag + "1"), "-p", t / (tag + "2")])
        _run(["-q", "-d", "-Z"] + extra + ["-f", world / "two.sfq", "-u", t / (tag + "1.gz"), "-p", t / (tag + "2.gz")])
        for k in "12":
            assert inflated(t / (tag + k + ".gz")) == (t / (tag + k)).read_bytes(), tag + k
    assert (t / "p1").read_bytes() == (world / "r1.fq").read_bytes()
    _run(["-q", "-d", "-o", "merge=%s" % (t / "m"), "-f", world / "two.sfq", "-u", t / "m1", "-p", t / "m2"])
    _run(["-q", "-d", "-Z", "-o", "merge=%s" % (t / "m.gz"), "-f", world / "two.sfq", "-u", t / "m1.gz", "-p", t / "m2.gz"])
    for k in ("m", "m1", "m2"):
        assert inflated(t / (k + ".gz")) == (t / k).read_bytes(), k
    assert len((t / "m").read_bytes()) > 0


def test_sample_files(tmp_path, world):
    from test_demux import lane
    t = tmp_path
    (t / "s.tsv").write_bytes(b"".join(b"%s\t%s\n" % (n.encode(), r) for n, r in zip(NAMES, ROWS)))
    fq = lane(np.random.default_rng(5), 3000, ROWS, 8, "hdr", lens=(30, 80))
    (t / "in.fq").write_bytes(fq)
    _run(["-q", "-B", 500, "-u", t / "in.fq", "-f", t / "x.sfq"])
    _run(["-q", "-d", "-X", "%s,out=%s" % (t / "s.tsv", t / "a_"), "-f", t / "x.sfq", "-u", t / "a_un.fastq"])
    _run(["-q", "-d", "-Z", "-X", "%s,out=%s" % (t / "s.tsv", t / "z_"), "-f", t / "x.sfq", "-u", t / "z_un.fastq.gz"])
    for n in NAMES + ["un"]:
        assert inflated(t / ("z_%s.fastq.gz" % n)) == (t / ("a_%s.fastq" % n)).read_bytes(), n
        assert not (t / ("z_%s.fastq" % n)).exists()
    assert sum(len((t / ("a_%s.fastq" % n)).read_bytes()) for n in NAMES) > 0

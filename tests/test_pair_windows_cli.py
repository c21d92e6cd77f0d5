"""-W (a window of pairs on decode) and -M (the mates' names compared on encode) on the command line (cli.cpp):
windows of an archive of several segments against slices of the two input files; files out of step in the second slab; and the
argument errors of both options, found before any GPU is touched or any file is opened."""
import os
import subprocess

import pytest

from slimfastq_amd import capi
from test_gpu_parity import _cli
from test_pairs import mates, records

gpu = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")
REC = b"@r\nACGT\n+\nIIII\n"


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


def _info(path):
    out = _run(["-s", "-f", path]).stderr.decode()
    return dict(l.split("=", 1) for l in out.partition("\n:::: Files")[0].replace(" ", "").splitlines() if "=" in l)


# ---- -W ------------------------------------------------------------------------------------------------------------------------------

N = 7600


@pytest.fixture(scope="module")
def paired(tmp_path_factory):
    """R1 of 50-base reads, R2 of 250-base reads, about 5 MB: with -S 1 several segments; (the directory, R1's records, R2's, the
    number of segments)"""
    t = tmp_path_factory.mktemp("pairs")
    a, b = capi.synth_fastq(N, 50, seed=70), capi.synth_fastq(N, 250, seed=71)
    (t / "r1.fq").write_bytes(a)
    (t / "r2.fq").write_bytes(b)
    p = _run(["-q", "-K", "-S", 1, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0, p.stderr
    info = _info(t / "x.sfq")
    assert info["usr.pair"] == "1" and int(info["seg.count"]) > 2, info
    return t, records(a), records(b), int(info["seg.count"])


def window(t, arg, o1="o1.fq", o2="o2.fq"):
    p = _run(["-d", "-O", "-W", arg, "-f", t / "x.sfq", "-u", t / o1, "-p", t / o2])
    assert p.returncode == 0, p.stderr
    return (t / o1).read_bytes(), (t / o2).read_bytes()


# per: about the pairs of a segment (slabs hold about equal shares)
WINDOWS = {
    "inside_a_segment": lambda per: (per // 2, 7),
    "across_a_border": lambda per: (per - 300, 600),
    "across_two_borders": lambda per: (per // 2, 2 * per),
    "the_last_pair": lambda per: (N - 1, 1),
    "clipped_at_the_end": lambda per: (N - 5, 1000),
    "all": lambda per: (0, N),
}


@gpu
@pytest.mark.parametrize("which", sorted(WINDOWS))
def test_windows_of_an_archive_of_several_segments(paired, which):
    t, ra, rb, nseg = paired
    p0, n = WINDOWS[which](N // nseg)
    got = window(t, "%d:%d" % (p0, n))
    assert got == (b"".join(ra[p0:p0 + n]), b"".join(rb[p0:p0 + n])), (p0, n)


@gpu
def test_a_window_behind_the_last_pair(paired):
    t = paired[0]
    p = _run(["-d", "-O", "-W", "%d:1" % N, "-f", t / "x.sfq", "-u", t / "n1.fq", "-p", t / "n2.fq"])
    assert p.returncode == 1 and b"-W" in p.stderr and str(N).encode() in p.stderr, p.stderr
    assert not (t / "n1.fq").exists() and not (t / "n2.fq").exists()


@gpu
def test_a_window_of_an_archive_written_without_p(tmp_path):
    (tmp_path / "r1.fq").write_bytes(capi.synth_fastq(100, 50, seed=3))
    assert _run(["-q", "-u", tmp_path / "r1.fq", "-f", tmp_path / "plain.sfq"]).returncode == 0
    p = _run(["-d", "-W", "0:1", "-f", tmp_path / "plain.sfq", "-u", tmp_path / "o1.fq", "-p", tmp_path / "o2.fq"])
    assert p.returncode == 1 and b"-p" in p.stderr, p.stderr


# ---- -M ------------------------------------------------------------------------------------------------------------------------------

@gpu
def test_files_out_of_step_in_the_second_slab(tmp_path):
    t = tmp_path
    a, b = mates(9000, 100, seed=8)                                   # about 2.6 MB each: with -S 1 (half a slab a file) several slabs
    ra, rb = records(a), records(b)
    at = 3000                                                         # R2 lost a record here: from then on its records are the next pair's
    (t / "r1.fq").write_bytes(b"".join(ra[:-1]))
    (t / "r2.fq").write_bytes(b"".join(rb[:at] + rb[at + 1:]))
    assert (1 << 19) + 4096 < len(b"".join(ra[:at])) < (1 << 20) - 4096 and (1 << 19) + 4096 < len(b"".join(rb[:at])) < (1 << 20) - 4096
    # (a slab takes half a MiB of each file: pair 3000 lies in the second)
    p = _run(["-q", "-M", "-S", 1, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / "x.sfq"])
    name_a, name_b = ra[at].split(b" ")[0][1:], rb[at + 1].split(b" ")[0][1:]
    assert p.returncode == 1, p.stderr
    assert b"-M" in p.stderr and (b"pair %d " % at) in p.stderr and name_a in p.stderr and name_b in p.stderr, p.stderr
    assert not (t / "x.sfq").exists() and sorted(os.listdir(t)) == ["r1.fq", "r2.fq"]
    # without -M the damage goes into the archive
    p = _run(["-q", "-S", 1, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0 and (t / "x.sfq").exists(), p.stderr


@gpu
def test_good_files_give_the_archive_they_give_without_the_check(tmp_path):
    t = tmp_path
    a, b = mates(9000, 100, seed=9)
    (t / "r1.fq").write_bytes(a)
    (t / "r2.fq").write_bytes(b)
    for name, extra in (("plain.sfq", []), ("checked.sfq", ["-M"])):
        p = _run(["-q", "-S", 1, "-u", t / "r1.fq", "-p", t / "r2.fq", "-f", t / name] + extra)
        assert p.returncode == 0, p.stderr
    assert (t / "plain.sfq").read_bytes() == (t / "checked.sfq").read_bytes()
    assert int(_info(t / "plain.sfq")["seg.count"]) > 2


# ---- the argument errors: no GPU -------------------------------------------------------------------------------------------------------

def refused(args, tmp_path, outputs, option, **kw):
    p = subprocess.run([_cli()] + [str(a) for a in args], capture_output=True, **kw)
    assert p.returncode == 1 and option in p.stderr, (p.returncode, p.stderr)
    for o in outputs:
        assert not (tmp_path / o).exists(), o


@pytest.fixture
def files(tmp_path):
    (tmp_path / "r1.fq").write_bytes(REC)
    (tmp_path / "r2.fq").write_bytes(REC)
    return tmp_path


def test_window_without_d(files):
    refused(["-W", "0:1", "-u", files / "r1.fq", "-p", files / "r2.fq", "-f", files / "x.sfq"], files, ["x.sfq"], b"-W")


def test_window_without_p(files):
    refused(["-d", "-W", "0:1", "-f", files / "nowhere.sfq", "-u", files / "o1.fq"], files, ["o1.fq"], b"-W")


def test_window_with_a_range(files):
    refused(["-d", "-W", "0:1", "-R", "0:2", "-f", files / "nowhere.sfq", "-u", files / "o1.fq", "-p", files / "o2.fq"], files, ["o1.fq", "o2.fq"], b"-W")


def test_window_with_batch(files):
    jobs = b"%s\t%s\n" % (str(files / "nowhere.sfq").encode(), str(files / "o1.fq").encode())
    refused(["-b", "-d", "-W", "0:1", "-p", files / "o2.fq"], files, ["o1.fq", "o2.fq"], b"-W", input=jobs)


@pytest.mark.parametrize("arg", ("", "5", "5:", ":5", "5:0", "a:b", "1:2:3", "-1:2", "1:2x", "99999999999999999999:1", "1:99999999999999999999"))
def test_window_with_a_malformed_range(files, arg):
    refused(["-d", "-W", arg, "-f", files / "nowhere.sfq", "-u", files / "o1.fq", "-p", files / "o2.fq"], files, ["o1.fq", "o2.fq"], b"-W")


def test_mate_check_without_p(files):
    refused(["-M", "-u", files / "r1.fq", "-f", files / "x.sfq"], files, ["x.sfq"], b"-M")


def test_mate_check_with_d(files):
    refused(["-d", "-M", "-f", files / "nowhere.sfq", "-u", files / "o1.fq", "-p", files / "o2.fq"], files, ["o1.fq", "o2.fq"], b"-M")

"""-X on the command line, where no GPU is needed: a bad list of terms, a sheet that is missing or malformed, a mode or an option that -X
does not go with, files that exist and more files than the process may open end the run with a message, before a device is opened or
anything is decoded."""
import os
import resource
import subprocess

import pytest

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=60, **kw)


@pytest.fixture
def sheet(tmp_path):
    (tmp_path / "s.tsv").write_bytes(b"# lane 1\nalpha\tATCACG\nbeta\tTTAGGC\n")
    return tmp_path / "s.tsv"


def refused(tmp_path, p, *says):
    assert p.returncode == 1 and b"-X" in p.stderr, p.stderr
    for s in says:
        assert s in p.stderr, p.stderr
    assert b"none.sfq" not in p.stderr                                 # refused before the archive is looked for
    assert not (tmp_path / "out").exists() and not list(tmp_path.glob("pre_*"))


@pytest.mark.parametrize("terms,says", [("mm=x", b"mm=x"), ("mm=33", b"mm=33"), ("nope", b"nope"), ("hdr,inline", b"hdr and inline"), ("hdr2", b"hdr2"),
                                        ("inline2", b"inline2"), ("inline,inline2,hdr2", b"inline2 and hdr2"), ("out=", b"out="), ("counts=", b"counts="),
                                        ("", b"no such term"), ("inline=-1", b"inline=-1"), ("mm=7", b"mm=7")])
def test_bad_terms(tmp_path, sheet, terms, says):
    p = _run(["-d", "-X", "%s,out=%s,%s" % (sheet, tmp_path / "pre_", terms), "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"])
    refused(tmp_path, p, says)


def test_out_is_required_and_inline2_needs_p(tmp_path, sheet):
    refused(tmp_path, _run(["-d", "-X", "%s,mm=1" % sheet, "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"]), b"out=PREFIX")
    refused(tmp_path, _run(["-d", "-X", "", "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"]))
    (tmp_path / "dual.tsv").write_bytes(b"a\tACG+TTA\nb\tGGC+CAT\n")
    refused(tmp_path, _run(["-d", "-X", "%s,out=%s,inline,inline2" % (tmp_path / "dual.tsv", tmp_path / "pre_"), "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"]),
            b"inline2", b"-p")


def test_sheets_that_cannot_be_used(tmp_path):
    for name, text, says in (("missing.tsv", None, b"missing.tsv"), ("empty.tsv", b"# nothing\n", b"no sample"), ("bad.tsv", b"a\tACGT\nb\tACG\n", b"line 2"),
                             ("dup.tsv", b"a\tACGT\na\tAAAA\n", b"line 2"), ("un.tsv", b"unassigned\tACGT\n", b"unassigned")):
        if text is not None:
            (tmp_path / name).write_bytes(text)
        p = _run(["-d", "-X", "%s,out=%s" % (tmp_path / name, tmp_path / "pre_"), "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"])
        refused(tmp_path, p, says, name.encode())


def test_where_it_does_not_go(tmp_path, sheet):
    spec = "%s,out=%s" % (sheet, tmp_path / "pre_")
    (tmp_path / "in.fq").write_bytes(b"@r 1:N:0:ATCACG\nACGT\n+\nIIII\n")
    p = _run(["-X", spec, "-u", tmp_path / "in.fq", "-f", tmp_path / "x.sfq"])                  # encode mode
    assert p.returncode == 1 and b"-X" in p.stderr and b"-d" in p.stderr and not (tmp_path / "x.sfq").exists()
    p = _run(["-s", "-X", spec, "-f", tmp_path / "x.sfq"])
    assert p.returncode == 1 and b"-X" in p.stderr
    refused(tmp_path, _run(["-d", "-X", spec, "-x", "fasta", "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"]), b"-x")
    refused(tmp_path, _run(["-d", "-X", spec, "-W", "0:10", "-p", tmp_path / "out2", "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"]), b"-W")
    refused(tmp_path, _run(["-d", "-X", spec, "-o", "merge=%s" % (tmp_path / "m.fq"), "-p", tmp_path / "out2", "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"]),
            b"merge=")
    assert not (tmp_path / "m.fq").exists() and not (tmp_path / "out2").exists()


def test_files_that_exist_and_too_many_files(tmp_path, sheet):
    spec = "%s,out=%s,counts=%s" % (sheet, tmp_path / "pre_", tmp_path / "counts.tsv")
    for name in ("pre_beta.fastq", "counts.tsv"):
        (tmp_path / name).write_bytes(b"mine\n")
        p = _run(["-d", "-X", spec, "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"])
        assert p.returncode == 1 and name.encode() in p.stderr and b"File exists" in p.stderr and b"none.sfq" not in p.stderr
        assert (tmp_path / name).read_bytes() == b"mine\n"
        p = _run(["-d", "-O", "-X", spec, "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"])  # with -O the run goes on, to the device and the archive that is not there
        assert p.returncode != 0 and b"File exists" not in p.stderr and b"-X" not in p.stderr
        (tmp_path / name).unlink()
    with open(tmp_path / "pre_alpha_R2.fastq", "wb") as f:
        f.write(b"mine\n")
    p = _run(["-d", "-X", spec, "-f", tmp_path / "none.sfq", "-u", tmp_path / "out", "-p", tmp_path / "out2"])
    assert p.returncode == 1 and b"pre_alpha_R2.fastq" in p.stderr and b"File exists" in p.stderr
    (tmp_path / "pre_alpha_R2.fastq").unlink()
    # 40 samples in pairs are 80 + 2 + 1 files: more than a limit of 64 less the 16 kept back; the message names both numbers
    (tmp_path / "many.tsv").write_bytes(b"".join(b"s%d\t%s\n" % (i, bytes(b"ACGT"[(i >> (2 * j)) & 3] for j in range(4))) for i in range(40)))
    spec = "%s,out=%s,counts=%s" % (tmp_path / "many.tsv", tmp_path / "pre_", tmp_path / "counts.tsv")
    hard = resource.getrlimit(resource.RLIMIT_NOFILE)[1]
    p = _run(["-d", "-X", spec, "-f", tmp_path / "none.sfq", "-u", tmp_path / "out", "-p", tmp_path / "out2"],
             preexec_fn=lambda: resource.setrlimit(resource.RLIMIT_NOFILE, (64, hard)))
    assert p.returncode == 1 and b"-X" in p.stderr and b"83 files" in p.stderr and b"(64," in p.stderr and b"none.sfq" not in p.stderr, p.stderr
    assert not list(tmp_path.glob("pre_*"))

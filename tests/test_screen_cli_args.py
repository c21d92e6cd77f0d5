"""-G on the command line, where no GPU is needed: a bad list of terms, a missing, empty or sequence-less reference and a mode that
-G does not go with end the run with a message, before a device is opened or anything is decoded."""
import os
import subprocess

import pytest

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")


def _run(args):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=60)


@pytest.fixture
def ref(tmp_path):
    (tmp_path / "ref.fa").write_bytes(b">r\nACGTACGTACGTAGCTAGCTAGCATCGATCGATCAGCTACGATCAGCTACGACT\n")
    return tmp_path / "ref.fa"


@pytest.mark.parametrize("spec", ["", "k=27", "ref=", "ref=%s,k=3", "ref=%s,k=32", "ref=%s,hits=0", "ref=%s,pct=101", "ref=%s,keep=1", "ref=%s,nope",
                                  "ref=%s,,keep", "%s"])
def test_bad_terms(tmp_path, ref, spec):
    spec = spec.replace("%s", str(ref))
    p = _run(["-d", "-G", spec, "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"])
    assert p.returncode == 1 and b"-G" in p.stderr and not (tmp_path / "out").exists()
    assert b"none.sfq" not in p.stderr                                 # the terms are refused before the archive is looked for


def test_references_that_cannot_be_used(tmp_path, ref):
    (tmp_path / "empty.fa").write_bytes(b"")
    (tmp_path / "names.fa").write_bytes(b">only\n>names\n")
    for bad in ("missing.fa", "empty.fa", "names.fa"):
        p = _run(["-d", "-G", "ref=%s,ref=%s" % (ref, tmp_path / bad), "-f", tmp_path / "none.sfq", "-u", tmp_path / "out"])
        assert p.returncode == 1 and bad.encode() in p.stderr and b"-G" in p.stderr and not (tmp_path / "out").exists()
        assert b"none.sfq" not in p.stderr


def test_where_it_does_not_go(tmp_path, ref):
    (tmp_path / "in.fq").write_bytes(b"@r\nACGT\n+\nIIII\n")
    p = _run(["-G", "ref=%s" % ref, "-u", tmp_path / "in.fq", "-f", tmp_path / "x.sfq"])
    assert p.returncode == 1 and b"-G" in p.stderr and b"-d" in p.stderr and not (tmp_path / "x.sfq").exists()
    p = _run(["-s", "-G", "ref=%s" % ref, "-f", tmp_path / "x.sfq"])
    assert p.returncode == 1 and b"-G" in p.stderr

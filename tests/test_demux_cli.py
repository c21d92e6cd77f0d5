"""-X on the command line (cli.cpp): a decode that sorts the reads of an archive of several segments into a file a
sample, by the barcode in the header's index field or inline with clip, single and with -p.  Every file is compared byte for byte with
the part that demux_rule.py's rule gives for the whole text; counts= and the line on stderr with the rule's counts; -O."""
import os
import subprocess

import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Demux, DemuxPart, DEMUX_HEADER as H, DEMUX_BASES as B
from demux_rule import demux
from test_demux import lane

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")
NAMES = ["alpha", "Beta.2", "gamma_-9", "d"]
ROWS = [b"ATCACGTT", b"TTAGGCAA", b"CGATGTCC", b"ACAGTGGG"]


CODED = b"ACGT"                 # what a spoiled INLINE base becomes: a '.' in a base line is no text an archive takes (test_demux.py has those bytes)


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


def line(c, what="reads"):
    return "demultiplexed %d %s: %d assigned (%d perfect), %d short, %d far, %d ambiguous" % (
        c["n_units"], what, c["n_assigned"], c["n_perfect"], c["n_short"], c["n_far"], c["n_ambiguous"])


def counts(units, dual=0):
    rows = ["%s\t%s\t%d\n" % (n, (r[:dual] + b"+" + r[dual:] if dual else r).decode(), u) for n, r, u in zip(NAMES, ROWS, units)]
    return "".join(rows) + "unassigned\t\t%d\n" % units[-1]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the sheets and four archives of several segments each: barcodes in the header or inline, single or paired"""
    t = tmp_path_factory.mktemp("demux_cli")
    (t / "one.tsv").write_bytes(b"# sample\tbarcode\n" + b"".join(b"%s\t%s\n" % (n.encode(), r.lower() if i & 1 else r) for i, (n, r) in enumerate(zip(NAMES, ROWS))))
    (t / "two.tsv").write_bytes(b"".join(b"%s\t%s+%s\n" % (n.encode(), r[:5], r[5:]) for n, r in zip(NAMES, ROWS)))
    rng = np.random.default_rng(77)
    texts = {"hdr": lane(rng, 18000, ROWS, 8, "hdr", lens=(30, 80)), "inline": lane(rng, 18000, ROWS, 8, "inline", lens=(30, 80), alphabet=CODED)}
    for k, fq in texts.items():
        (t / (k + ".fq")).write_bytes(fq)
        p = _run(["-q", "-S", "1", "-B", "500", "-u", t / (k + ".fq"), "-f", t / (k + ".sfq")])
        assert p.returncode == 0, p.stderr
    for k, where in (("phdr", "hdr"), ("pin2", "inline2")):
        inter = lane(rng, 9000, ROWS, 5, where, pairs=True, lens=(30, 80), alphabet=CODED)
        rs = inter.split(b"\n@r")
        recs = [rs[0] + b"\n"] + [b"@r" + r + b"\n" for r in rs[1:-1]] + [b"@r" + rs[-1]]
        assert b"".join(recs) == inter and len(recs) == 18000
        (t / (k + "_1.fq")).write_bytes(b"".join(recs[0::2]))
        (t / (k + "_2.fq")).write_bytes(b"".join(recs[1::2]))
        p = _run(["-q", "-S", "1", "-B", "500", "-u", t / (k + "_1.fq"), "-p", t / (k + "_2.fq"), "-f", t / (k + ".sfq")])
        assert p.returncode == 0, p.stderr
        texts[k] = inter
    return t, texts


def test_header_barcodes_single(tmp_path, world):
    t, texts = world
    fq = texts["hdr"]
    assert len(fq) > (2 << 20)                                          # more than one segment at -S 1
    rule = Demux([DemuxPart(H, 0, 0, 0, 8)], n_samples=4, max_mm=1)
    parts, units, c = demux(fq, rule, ROWS)
    pre = tmp_path / "s_"
    p = _run(["-d", "-X", "%s,out=%s,counts=%s" % (t / "one.tsv", pre, tmp_path / "c.tsv"), "-f", t / "hdr.sfq", "-u", tmp_path / "un.fq"])
    assert p.returncode == 0, p.stderr
    for n, want in zip(NAMES, parts):
        assert (tmp_path / ("s_%s.fastq" % n)).read_bytes() == want, n
    assert (tmp_path / "un.fq").read_bytes() == parts[4]
    assert (tmp_path / "c.tsv").read_text() == counts(units)
    assert p.stderr.decode().strip().splitlines()[-1] == line(c)
    assert 0 < c["n_perfect"] < c["n_assigned"] < c["n_units"]
    # files that exist: refused without -O, written over with it; -q: no line
    p = _run(["-d", "-X", "%s,out=%s,mm=0" % (t / "one.tsv", pre), "-f", t / "hdr.sfq", "-u", tmp_path / "un2.fq"])
    assert p.returncode == 1 and b"File exists" in p.stderr and not (tmp_path / "un2.fq").exists()
    parts0, _, _ = demux(fq, Demux([DemuxPart(H, 0, 0, 0, 8)], n_samples=4, max_mm=0), ROWS)
    p = _run(["-d", "-q", "-O", "-X", "%s,out=%s,mm=0" % (t / "one.tsv", pre), "-f", t / "hdr.sfq", "-u", tmp_path / "un.fq"])
    assert p.returncode == 0 and p.stderr == b"", p.stderr
    for n, want in zip(NAMES + ["un"], parts0):
        assert (tmp_path / ("s_%s.fastq" % n if n != "un" else "un.fq")).read_bytes() == want, n
    # a range of records, across a segment's end: the units outside are in no file
    ranged = Demux([DemuxPart(H, 0, 0, 0, 8)], n_samples=4, max_mm=1, first_record=6000, n_records=5000)
    partsr, _, cr = demux(fq, ranged, ROWS)
    p = _run(["-d", "-O", "-R", "6000:5000", "-X", "%s,out=%s" % (t / "one.tsv", pre), "-f", t / "hdr.sfq", "-u", tmp_path / "un.fq"])
    assert p.returncode == 0, p.stderr
    for n, want in zip(NAMES + ["un"], partsr):
        assert (tmp_path / ("s_%s.fastq" % n if n != "un" else "un.fq")).read_bytes() == want, n
    assert p.stderr.decode().strip().splitlines()[-1] == line(cr)


def test_inline_barcodes_with_clip(tmp_path, world):
    t, texts = world
    fq = texts["inline"]
    rule = Demux([DemuxPart(B, 0, 0, 0, 8)], n_samples=4, max_mm=2, clip=1)
    parts, units, c = demux(fq, rule, ROWS)
    p = _run(["-d", "-X", "%s,inline,clip,mm=2,out=%s" % (t / "one.tsv", tmp_path / "i_"), "-f", t / "inline.sfq", "-u", tmp_path / "un.fq"])
    assert p.returncode == 0, p.stderr
    for n, want in zip(NAMES, parts):
        assert (tmp_path / ("i_%s.fastq" % n)).read_bytes() == want, n
    assert (tmp_path / "un.fq").read_bytes() == parts[4] and sum(len(x) for x in parts) == len(fq) - 16 * c["n_assigned"]
    assert p.stderr.decode().strip().splitlines()[-1] == line(c)
    # the dual sheet on the same reads: part 1 follows part 0 in the bases
    rule = Demux([DemuxPart(B, 0, 0, 0, 5), DemuxPart(B, 0, 0, 5, 3)], n_samples=4, max_mm=1)
    parts, units, c = demux(fq, rule, ROWS)
    p = _run(["-d", "-X", "%s,inline,out=%s,counts=%s" % (t / "two.tsv", tmp_path / "j_", tmp_path / "c.tsv"), "-f", t / "inline.sfq", "-u", tmp_path / "un2.fq"])
    assert p.returncode == 0, p.stderr
    for n, want in zip(NAMES, parts):
        assert (tmp_path / ("j_%s.fastq" % n)).read_bytes() == want, n
    assert (tmp_path / "un2.fq").read_bytes() == parts[4] and (tmp_path / "c.tsv").read_text() == counts(units, dual=5)


def test_a_format_6_archive_is_refused(tmp_path, world):
    """an archive written with -B 0 is the reference's own format: refused once the archive is read, before any file is opened"""
    t, _ = world
    (tmp_path / "in.fq").write_bytes(capi.synth_fastq(2000, 100, seed=6))
    p = _run(["-q", "-B", "0", "-u", tmp_path / "in.fq", "-f", tmp_path / "v6.sfq"])
    assert p.returncode == 0, p.stderr
    p = _run(["-d", "-X", "%s,out=%s,counts=%s" % (t / "one.tsv", tmp_path / "v_", tmp_path / "c.tsv"), "-f", tmp_path / "v6.sfq", "-u", tmp_path / "un.fq"])
    assert p.returncode == 1 and b"-X" in p.stderr and b"format-6" in p.stderr and b"-B 0" in p.stderr, p.stderr
    assert not list(tmp_path.glob("v_*")) and not (tmp_path / "un.fq").exists() and not (tmp_path / "c.tsv").exists()
    p = _run(["-d", "-f", tmp_path / "v6.sfq", "-u", tmp_path / "un.fq"])                      # without -X the same archive decodes
    assert p.returncode == 0 and (tmp_path / "un.fq").read_bytes() == (tmp_path / "in.fq").read_bytes()


@pytest.mark.parametrize("k,terms,p1", [("phdr", "hdr", DemuxPart(H, 0, 1, 0, 3)), ("pin2", "inline,inline2,clip", DemuxPart(B, 1, 0, 0, 3))])
def test_pairs(tmp_path, world, k, terms, p1):
    t, texts = world
    inter = texts[k]
    p0 = DemuxPart(H, 0, 0, 0, 5) if k == "phdr" else DemuxPart(B, 0, 0, 0, 5)
    rule = Demux([p0, p1], n_samples=4, max_mm=1, pairs=1, split_mates=1, clip=int("clip" in terms))
    parts, units, c = demux(inter, rule, ROWS)
    p = _run(["-d", "-X", "%s,%s,out=%s,counts=%s" % (t / "two.tsv", terms, tmp_path / "p_", tmp_path / "c.tsv"), "-f", t / (k + ".sfq"),
              "-u", tmp_path / "un_1.fq", "-p", tmp_path / "un_2.fq"])
    assert p.returncode == 0, p.stderr
    for s, n in enumerate(NAMES):
        assert (tmp_path / ("p_%s_R1.fastq" % n)).read_bytes() == parts[2 * s], n
        assert (tmp_path / ("p_%s_R2.fastq" % n)).read_bytes() == parts[2 * s + 1], n
    assert (tmp_path / "un_1.fq").read_bytes() == parts[8] and (tmp_path / "un_2.fq").read_bytes() == parts[9]
    assert (tmp_path / "c.tsv").read_text() == counts(units, dual=5)
    assert p.stderr.decode().strip().splitlines()[-1] == line(c, "pairs")
    assert 0 < c["n_assigned"] < c["n_units"] == 9000

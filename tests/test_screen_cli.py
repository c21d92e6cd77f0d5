"""-G on the command line (cli.cpp): a decode that drops -- or with `keep` writes alone -- the reads that share
k-mers with two reference FASTA files, one of them wrapped at 60 columns with lower case, a run of N and two records: a k-mer across
a line wrap counts, one across two records does not.  Against screen_rule.py's rule and its own flattening of the files; with -p,
-x fasta, -D, -R and -q, and the line on stderr.  Every comparison is exact byte equality."""
import os
import subprocess

import numpy as np
import pytest

from slimfastq_amd import capi
from slimfastq_amd.capi import Dedup, Screen
from screen_rule import flat_fasta, kmer_set, screen, windows
from test_dedup_decode import dd, planted
from test_pairs import records
from test_select import picked

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")
K = 27
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


def wrap(seq, cols=60, eol=b"\n"):
    return b"".join(seq[i:i + cols] + eol for i in range(0, len(seq), cols))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the references, the reads, the archive: 3000 reads of 100 bases, of which every fifth is cut from a reference"""
    t = tmp_path_factory.mktemp("screen_cli")
    rng = np.random.default_rng(41)
    one, two, three = (ACGT[rng.integers(0, 4, n)].tobytes() for n in (1000, 700, 500))
    one = one[:400] + b"N" * 30 + one[430:600].lower() + one[600:]
    (t / "a.fa").write_bytes(b">one a record\n" + wrap(one) + b">two\n" + wrap(two))
    (t / "b.fa").write_bytes(b">three\r\n" + wrap(three, 70, b"\r\n"))
    kset = kmer_set(K, flat_fasta((t / "a.fa").read_bytes()), flat_fasta((t / "b.fa").read_bytes()))
    assert kset == kmer_set(K, one, two, three)
    rs = [r.split(b"\n") for r in records(capi.synth_fastq(3000, 100, seed=92))]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    for i in range(0, 3000, 5):
        src = (one.upper().replace(b"N", b"A"), two, three)[i % 3]
        at = int(rng.integers(0, len(src) - 100))
        b = src[at:at + 100]
        rs[i][1] = b if i % 2 else b.translate(comp)[::-1]
    rs[5][1] = one[30:90] + ACGT[rng.integers(0, 4, 40)].tobytes()     # bases 30..90 of `one` lie across its first line wrap
    rs[7][1] = one[-50:] + two[:50]                                    # the end of one record and the start of the next: not a sequence
    fq = b"".join(b"\n".join(r) for r in rs)
    (t / "in.fq").write_bytes(fq)
    p = _run(["-q", "-K", "-u", t / "in.fq", "-f", t / "x.sfq"])
    assert p.returncode == 0, p.stderr
    return t, fq, kset


def scr(fq, rule, kset):
    kept, units = screen(fq, rule, K, kset)[:2]
    rs = records(fq)
    return b"".join(rs[r] for r in kept), units, len(kept) // (2 if rule.pairs else 1)


def line(units, matched, kept, kset, what="reads", k=K):
    return "screened %d %s: %d matched (%.2f %%), %d kept (%d k-mers of %d bases in the set)" % (
        units, what, matched, 100.0 * matched / units if units else 0.0, kept, len(kset), k)


def spec(t, *more):
    return ",".join(["ref=%s" % (t / "a.fa"), "ref=%s" % (t / "b.fa")] + list(more))


def test_the_whole_archive_and_the_line_on_stderr(tmp_path, world):
    t, fq, kset = world
    rs = records(fq)
    assert len(windows(rs[5].split(b"\n")[1], K)) == 74 and sum(v in kset for v in windows(rs[5].split(b"\n")[1], K)) >= 34    # across the wrap
    assert sum(v in kset for v in windows(rs[7].split(b"\n")[1], K)) == 2 * (50 - K + 1)      # none of the windows across the two records
    want, units, kept = scr(fq, Screen(), kset)
    assert units == 3000 and 2390 <= kept <= 2399                      # the 600 reads cut from a reference and record 7, at least
    p = _run(["-d", "-G", spec(t), "-f", t / "x.sfq", "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out").read_bytes() == want
    assert p.stderr.decode().splitlines()[-1] == line(3000, 3000 - kept, kept, kset)
    # keep: the others; hits= and pct= as the rule says; rs[7] has 48 hits of 74 windows
    for terms, rule, seven in ((("keep",), Screen(keep_matched=True), True), (("hits=49",), Screen(min_hits=49), True),
                               (("pct=65", "keep"), Screen(min_pct=65, keep_matched=True), False), (("hits=48", "pct=64"), Screen(min_hits=48, min_pct=64), False)):
        want, units, kept = scr(fq, rule, kset)
        p = _run(["-d", "-G", spec(t, *terms), "-f", t / "x.sfq", "-u", tmp_path / "out", "-O"])
        assert p.returncode == 0, p.stderr
        assert (tmp_path / "out").read_bytes() == want, terms
        assert (rs[7] in records(want)) == seven, terms
        matched = kept if rule.keep_matched else units - kept
        assert p.stderr.decode().splitlines()[-1] == line(3000, matched, kept, kset)
    p = _run(["-q", "-d", "-G", spec(t), "-f", t / "x.sfq", "-u", tmp_path / "quiet"])
    assert p.returncode == 0 and b"screened" not in p.stderr and (tmp_path / "quiet").read_bytes() == scr(fq, Screen(), kset)[0]


def test_another_k(tmp_path, world):
    t, fq, _ = world
    kset = {v for f in ("a.fa", "b.fa") for v in windows(flat_fasta((t / f).read_bytes()), 12)}
    kept, units = screen(fq, Screen(min_hits=20), 12, kset)[:2]
    rs = records(fq)
    p = _run(["-d", "-G", spec(t, "k=12", "hits=20"), "-f", t / "x.sfq", "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out").read_bytes() == b"".join(rs[r] for r in kept)
    assert p.stderr.decode().splitlines()[-1] == line(3000, 3000 - len(kept), len(kept), kset, k=12)


def test_with_a_range_picked_lines_and_the_dedup(tmp_path, world):
    t, fq, kset = world
    want, units, kept = scr(fq, Screen(first_record=1001, n_records=1500), kset)
    p = _run(["-d", "-G", spec(t), "-R", "1001:1500", "-f", t / "x.sfq", "-u", tmp_path / "out"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out").read_bytes() == want and p.stderr.decode().splitlines()[-1] == line(1500, 1500 - kept, kept, kset)
    want, units, kept = scr(fq, Screen(), kset)
    p = _run(["-d", "-G", spec(t), "-x", "fasta", "-f", t / "x.sfq", "-u", tmp_path / "out.fa"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "out.fa").read_bytes() == picked(want, capi.PICK_FASTA)
    # -D behind: the reads cut from a reference never reach the dedup; its line closes stderr, the screen's stands in front
    matched, _, nm = scr(fq, Screen(keep_matched=True), kset)
    doubled = tmp_path / "twice.fq"
    doubled.write_bytes(fq + fq)
    p = _run(["-q", "-K", "-u", doubled, "-f", tmp_path / "twice.sfq"])
    assert p.returncode == 0, p.stderr
    p = _run(["-d", "-G", spec(t), "-D", "-f", tmp_path / "twice.sfq", "-u", tmp_path / "dd"])
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "dd").read_bytes() == dd(want)
    err = p.stderr.decode().splitlines()
    assert err[-2] == line(6000, 2 * nm, 2 * kept, kset)
    assert err[-1] == "kept %d of %d reads (%d duplicates, %.2f %%)" % (len(records(dd(want))), 2 * kept, 2 * kept - len(records(dd(want))),
                                                                       100.0 * (2 * kept - len(records(dd(want)))) / (2 * kept))


def test_with_paired_files(tmp_path, world):
    t, _, _ = world
    a, b, inter = planted()
    rs = records(inter)
    ref = b"".join(b">r%d\n" % i + wrap(r.split(b"\n")[1], 25) for i, r in enumerate(rs[::7]))
    (tmp_path / "p.fa").write_bytes(ref)
    kset = kmer_set(21, flat_fasta(ref))
    (tmp_path / "r1.fq").write_bytes(a)
    (tmp_path / "r2.fq").write_bytes(b)
    p = _run(["-q", "-B", 64, "-u", tmp_path / "r1.fq", "-p", tmp_path / "r2.fq", "-f", tmp_path / "x.sfq"])
    assert p.returncode == 0, p.stderr
    split = lambda fq: (b"".join(records(fq)[0::2]), b"".join(records(fq)[1::2]))
    for terms, rule in (((), Screen(pairs=1)), (("both",), Screen(pairs=2)), (("either", "keep"), Screen(pairs=1, keep_matched=True))):
        kept, units = screen(inter, rule, 21, kset)[:2]
        want = b"".join(rs[r] for r in kept)
        g = ",".join(("ref=%s" % (tmp_path / "p.fa"), "k=21") + terms)
        p = _run(["-d", "-O", "-G", g, "-f", tmp_path / "x.sfq", "-u", tmp_path / "o1", "-p", tmp_path / "o2"])
        assert p.returncode == 0, p.stderr
        assert ((tmp_path / "o1").read_bytes(), (tmp_path / "o2").read_bytes()) == split(want), terms
        n = len(kept) // 2
        assert p.stderr.decode().splitlines()[-1] == line(1200, n if rule.keep_matched else 1200 - n, n, kset, "pairs", 21)
    # without -p: the interleaved text, whole pairs all the same; -W: the window's pairs alone; -D behind, of pairs
    kept, units = screen(inter, Screen(pairs=1), 21, kset)[:2]
    want = b"".join(rs[r] for r in kept)
    g = "ref=%s,k=21" % (tmp_path / "p.fa")
    p = _run(["-d", "-O", "-G", g, "-f", tmp_path / "x.sfq", "-u", tmp_path / "both"])
    assert p.returncode == 0 and (tmp_path / "both").read_bytes() == want, p.stderr
    part = b"".join(rs[200:1800])
    win = b"".join(records(part)[r] for r in screen(part, Screen(pairs=1), 21, kset)[0])
    p = _run(["-d", "-O", "-G", g, "-W", "100:800", "-f", tmp_path / "x.sfq", "-u", tmp_path / "w1", "-p", tmp_path / "w2"])
    assert p.returncode == 0, p.stderr
    assert ((tmp_path / "w1").read_bytes(), (tmp_path / "w2").read_bytes()) == split(win)
    p = _run(["-q", "-d", "-O", "-G", g, "-D", "-f", tmp_path / "x.sfq", "-u", tmp_path / "d1", "-p", tmp_path / "d2"])
    assert p.returncode == 0, p.stderr
    assert ((tmp_path / "d1").read_bytes(), (tmp_path / "d2").read_bytes()) == split(dd(want, Dedup(pairs=1)))
    # both: pairs are wanted
    p = _run(["-d", "-O", "-G", spec(t, "both"), "-f", t / "x.sfq", "-u", tmp_path / "none"])
    assert p.returncode != 0 and b"-G both" in p.stderr

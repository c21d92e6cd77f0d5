"""Text statistics counted on the GPU at encode time (stats.hip): sfq_text_stats against ten lines of numpy
over fq.split(b"\\n"), their merge and their "txt.stat" stream, the switch on a context, and the CLI's -Y / -s.  Every comparison
of statistics is exact equality of the whole struct."""
import ctypes as C
import os
import subprocess
import zlib

import numpy as np
import pytest

import util
from slimfastq_amd import capi
from test_kernel_resources import kernel_metadata

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")
CYC = capi.STATS_CYCLES
# stats.hip: k_stats_records takes 64 records a wavefront and 256 a workgroup; k_stats_text takes SPAN bytes of text a
# wavefront, WG_TILE a workgroup, ROW with one load instruction
REC_WAVE, REC_TILE = 64, 256
ROW, SPAN, WG_TILE = 1024, 16 << 10, 64 << 10


def ref_stats(fq: bytes) -> capi.TextStats:
    """The reference: numpy over the lines of the text."""
    lines = fq.split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1
    t = capi.TextStats()
    t.n_records = len(lines) // 4
    t.hdr_bytes, t.seq_bytes, t.plus_bytes, t.qlt_bytes = (sum(len(l) for l in lines[k:-1:4]) for k in range(4))
    t.seq_len_min, t.seq_len_max = min(len(l) for l in lines[1:-1:4]), max(len(l) for l in lines[1:-1:4])
    t.seq_hist[:] = np.bincount(np.frombuffer(b"".join(lines[1:-1:4]), np.uint8), minlength=256).tolist()
    q = np.frombuffer(b"".join(lines[3:-1:4]), np.uint8)
    t.qlt_hist[:] = np.bincount(q, minlength=256).tolist()
    qlen = np.array([len(l) for l in lines[3:-1:4]], np.int64)
    cyc = np.minimum(np.arange(len(q)) - np.repeat(np.cumsum(qlen) - qlen, qlen), CYC)         # each byte's position in its line
    t.cyc_n[:] = np.bincount(cyc, minlength=CYC + 1).tolist()
    t.cyc_qsum[:] = np.bincount(cyc, weights=q, minlength=CYC + 1).astype(np.uint64).tolist()   # (sums far below 2^53: exact)
    return t


def diff(a: capi.TextStats, b: capi.TextStats):
    """Where two structs differ (for the assertion message)."""
    out = []
    for name, typ in capi.TextStats._fields_:
        x, y = getattr(a, name), getattr(b, name)
        if hasattr(x, "__len__"):
            out += ["%s[%d]: %d != %d" % (name, i, x[i], y[i]) for i in range(len(x)) if x[i] != y[i]][:4]
        elif x != y:
            out.append("%s: %d != %d" % (name, x, y))
    return out


def text_section(t: capi.TextStats):
    """The key = value lines -s prints under ':::: Text ::::' (cli.cpp print_text_stats, re-stated)."""
    def pct(part, total):
        return "%.2f" % (100.0 * part / total if total else 0.0)
    sh, qh = t.seq_hist, t.qlt_hist
    seen = [b for b in range(256) if qh[b]]
    cyc = ["%.1f" % (t.cyc_qsum[c] / t.cyc_n[c] - 33.0) for c in range(max([c for c in range(CYC) if t.cyc_n[c]], default=-1) + 1)]
    if t.cyc_n[CYC]:
        cyc.append("%.1f" % (t.cyc_qsum[CYC] / t.cyc_n[CYC] - 33.0))
    rows = [("records", str(t.n_records)), ("bases", str(t.seq_bytes)), ("seq_len_min", str(t.seq_len_min)), ("seq_len_max", str(t.seq_len_max)),
            ("seq_len_mean", "%.2f" % (t.seq_bytes / t.n_records)),
            ("gc_pct", pct(sh[ord("G")] + sh[ord("C")] + sh[ord("g")] + sh[ord("c")], t.seq_bytes)),
            ("n_pct", pct(sh[ord("N")] + sh[ord("n")] + sh[ord(".")], t.seq_bytes)),
            ("q20_pct", pct(sum(qh[b] for b in range(ord("5"), 256)), t.qlt_bytes)),
            ("q30_pct", pct(sum(qh[b] for b in range(ord("?"), 256)), t.qlt_bytes)),
            ("qlt_min", chr(seen[0])), ("qlt_max", chr(seen[-1])), ("cycle_mean_q", ",".join(cyc))]
    return ["%-16s = %s" % kv for kv in rows]


def random_stats(rng, top):
    t = capi.TextStats()
    for name, typ in capi.TextStats._fields_:
        if hasattr(getattr(t, name), "__len__"):
            getattr(t, name)[:] = [int(v) for v in rng.integers(1, top, len(getattr(t, name)), dtype=np.uint64)]
        else:
            setattr(t, name, int(rng.integers(1, min(top, 1 << 32) if "len" in name else top, dtype=np.uint64)))
    return t


# ---- CPU: merge, "txt.stat", resources, -s ----------------------------------------------------------------------------------

def test_merge_adds_sums_and_combines_the_length_range():
    rng = np.random.default_rng(1)
    a, b = random_stats(rng, 1 << 50), random_stats(rng, 1 << 50)
    a.seq_len_min, a.seq_len_max, b.seq_len_min, b.seq_len_max = 30, 150, 7, 90
    m = capi.stats_merge(a.copy(), b)
    assert (m.seq_len_min, m.seq_len_max) == (7, 150)
    assert capi.stats_merge(b.copy(), a) == m
    for name, typ in capi.TextStats._fields_:
        if name.startswith("seq_len"):
            continue
        x, y, z = getattr(a, name), getattr(b, name), getattr(m, name)
        if hasattr(x, "__len__"):
            assert list(z) == [p + q for p, q in zip(x, y)], name
        else:
            assert z == x + y, name
    # merging into zero copies; merging zero in changes nothing
    assert capi.stats_merge(capi.TextStats(), a) == a
    assert capi.stats_merge(a.copy(), capi.TextStats()) == a


def test_merge_of_two_halves_of_a_text_is_the_whole():
    fq = capi.synth_fastq(300, 100, seed=3) + capi.synth_fastq(5, 0, seed=4, kind=1) + capi.synth_fastq(200, 37, seed=5, kind=2)
    recs = util.split_records(fq, 1)
    for cut in (1, 300, 303, len(recs) - 1):
        a, b = ref_stats(b"".join(recs[:cut])), ref_stats(b"".join(recs[cut:]))
        got = capi.stats_merge(capi.stats_merge(capi.TextStats(), a), b)
        assert got == ref_stats(fq), (cut, diff(got, ref_stats(fq)))


def _pack_cases():
    rng = np.random.default_rng(2)
    dense = random_stats(rng, 1 << 62)
    assert min(dense.cyc_qsum) > 0 and max(dense.seq_hist) > 1 << 40
    early = ref_stats(capi.synth_fastq(50, 75, seed=6, kind=2))          # arrays that end early: 4 quality values, 75 cycles
    assert early.cyc_n[75] == 0 and early.cyc_n[74] == 50
    return {"zero": capi.TextStats(), "dense": dense, "early": early}


def test_pack_unpack_is_the_identity_and_damage_is_refused():
    for name, t in _pack_cases().items():
        blob = capi.pack_text_stats(t)
        assert capi.unpack_text_stats(blob) == t, name
        if name == "zero":
            assert len(blob) == 1 + 7 + 4
        if name == "early":
            assert len(blob) < 1024                                   # a few hundred bytes: the arrays end with their last non-zero entry
        cuts = range(len(blob)) if len(blob) < 600 else list(range(0, 40)) + list(range(40, len(blob), 97)) + [len(blob) - 1]
        for n in cuts:                                                # every truncation (the dense blob: a spread of them)
            with pytest.raises(capi.SfqError) as e:
                capi.unpack_text_stats(blob[:n])
            assert e.value.code == -6, (name, n)
        for bad in (blob + b"\0", bytes([blob[0] + 1]) + blob[1:], b"\0" + blob[1:]):
            with pytest.raises(capi.SfqError) as e:
                capi.unpack_text_stats(bad)
            assert e.value.code == -6, name


def test_pack_refuses_an_array_longer_than_the_struct():
    blob = bytearray(capi.pack_text_stats(capi.TextStats()))
    assert blob[8] == 0
    blob[8:9] = bytes([0x81, 0x02]) + b"\1" * 257                       # seq_hist with 257 entries
    with pytest.raises(capi.SfqError) as e:
        capi.unpack_text_stats(bytes(blob))
    assert e.value.code == -6


def test_stats_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata("stats.hip", tmp_path)
    assert len(meta) == 3, sorted(meta)
    for want in ("k_stats_records", "k_stats_text", "k_stats_finish"):
        assert [k for k in meta if want in k], want
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0 and vgprs <= 128, (name, vgprs, scratch)


KNOWN = b"@r1\nGGCCAATTNN\n+\nIIIIIIIIII\n@r2\nACGT\n+\n!5?~\n"
KNOWN_SECTION = ["records          = 2", "bases            = 14", "seq_len_min      = 4", "seq_len_max      = 10", "seq_len_mean     = 7.00",
                 "gc_pct           = 42.86", "n_pct            = 14.29", "q20_pct          = 92.86", "q30_pct          = 85.71",
                 "qlt_min          = !", "qlt_max          = ~", "cycle_mean_q     = 20.0,30.0,35.0,66.5,40.0,40.0,40.0,40.0,40.0,40.0"]
INFO = "whoami=slimfastq\nversion=10\nnum_records=2\ncomp.size=%d\n"


def _stat(path):
    p = subprocess.run([CLI, "-s", "-f", str(path)], capture_output=True, timeout=60)
    assert p.returncode == 0 and p.stdout == b"", p.stderr
    return p.stderr.decode()


def test_cli_stat_prints_the_text_section(tmp_path):
    assert text_section(ref_stats(KNOWN)) == KNOWN_SECTION            # the re-statement above against values worked out by hand
    plain = tmp_path / "plain.sfq"
    util.write_archive(str(plain), INFO % (3 * 8192), [("rec", b"abc")])
    today = (":::: Info ::::\nwhoami           = slimfastq\nversion          = 10\nnum_records      = 2\ncomp.size        = 24576\n"
             "\n:::: Files stream ::::\n i: name      : bytes\n 1: rec       : 3\n")
    assert _stat(plain) == today                                      # without the stream: what -s printed before
    blob = capi.pack_text_stats(ref_stats(KNOWN))
    with_stats = tmp_path / "stats.sfq"
    util.write_archive(str(with_stats), INFO % (4 * 8192), [("rec", b"abc"), ("txt.stat", blob)])
    out = _stat(with_stats)
    head, sep, tail = out.partition("\n:::: Text ::::\n")
    assert sep and head == today.replace("24576", "32768") + " 2: txt.stat  : %d\n" % len(blob)
    assert tail.splitlines() == KNOWN_SECTION
    # a read past cycle 511: the tail entry comes last
    long_fq = b"@r\n" + b"A" * 514 + b"\n+\n" + b"I" * 512 + b"5?\n"
    t = ref_stats(long_fq)
    assert (t.cyc_n[CYC], t.cyc_qsum[CYC]) == (2, ord("5") + ord("?"))
    util.write_archive(str(with_stats), INFO % (4 * 8192), [("rec", b"abc"), ("txt.stat", capi.pack_text_stats(t))])
    tail = _stat(with_stats).partition("\n:::: Text ::::\n")[2].splitlines()
    assert tail == text_section(t) and tail[-1] == "cycle_mean_q     = " + ",".join(["40.0"] * 512 + ["25.0"])
    # a damaged stream is reported, the rest still prints
    util.write_archive(str(with_stats), INFO % (4 * 8192), [("rec", b"abc"), ("txt.stat", blob[:-3])])
    out = _stat(with_stats)
    assert out.startswith(today.replace("24576", "32768")) and "txt.stat: damaged" in out and "records" not in out.partition(":::: Text ::::")[2]


def test_cli_usage_names_the_switch():
    p = subprocess.run([CLI, "-h"], capture_output=True, timeout=60)
    assert p.returncode == 0 and b"\n-Y " in p.stdout


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def sctx(ctx):
    """The session's context with the statistics on (off again afterwards)."""
    ctx.set_stats(True)
    try:
        yield ctx
    finally:
        ctx.set_stats(False)
        ctx.set_checksums(False)


LENGTHS = (1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1000)


def shaped_text(nrec, seed):
    """nrec records: base / quality lines of the LENGTHS (both lines of a record alike), header lines of '@' and 1..40 characters
    cycling, qualities over '!'..'~', bases from ACGTNacgtn. (the quality model alone codes such a text: sfq_encode_qlt_blocks)."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTNacgtn.", np.uint8)
    lens = rng.choice(LENGTHS, nrec)
    out = []
    for r in range(nrec):
        n = int(lens[r])
        out += [b"@", rng.integers(ord("a"), ord("z") + 1, 1 + r % 40, dtype=np.uint8).tobytes(), b"\n", alphabet[rng.integers(0, len(alphabet), n)].tobytes(),
                b"\n+\n", rng.integers(ord("!"), ord("~") + 1, n, dtype=np.uint8).tobytes(), b"\n"]
    return b"".join(out)


def _qlt_device(ctx, fq, off=0):
    """sfq_encode_qlt_blocks on a device copy of fq that starts off bytes behind a 16-byte boundary."""
    import torch
    t = torch.zeros(len(fq) + 64, dtype=torch.uint8, device="cuda")
    base = (-t.data_ptr()) % 16 + off
    t[base:base + len(fq)] = torch.frombuffer(bytearray(fq), dtype=torch.uint8).cuda()
    cap = capi.lib().sfq_encode_bound(len(fq))
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    ctx.encode_device(t.data_ptr() + base, len(fq), out.data_ptr(), cap, level=3, block_reads=256, qlt_only=True)
    return ctx.text_stats()


@pytest.mark.gpu
@pytest.mark.parametrize("nrec", [1, REC_WAVE - 1, REC_WAVE, REC_WAVE + 1, REC_TILE - 1, REC_TILE, REC_TILE + 1, 1100])
def test_shapes_records_and_lines_at_every_border(sctx, nrec):
    fq = shaped_text(nrec, seed=nrec)
    starts, lens = util.line_table(fq)
    if nrec >= REC_WAVE:
        assert set((starts % 16).tolist()) == set(range(16))           # lines start at every offset of a 16-byte unit
    if nrec >= REC_TILE:
        assert len(fq) > 2 * WG_TILE and set(lens[1::4].tolist()) == set(LENGTHS)
        # base and quality lines (the odd ones) straddle borders of spans and of tiles
        for step in (SPAN, WG_TILE):
            borders = np.arange(step, len(fq), step)
            k = np.searchsorted(starts, borders.astype(np.uint64), side="right") - 1
            assert np.any((k % 2 == 1) & (starts[k] < borders) & (borders < starts[k] + lens[k])), step
    want = ref_stats(fq)
    for off in ((0, 1, 15) if nrec in (1, REC_TILE + 1) else (0,)):    # the text's first byte anywhere in its 16-byte unit
        got = _qlt_device(sctx, fq, off)
        assert got is not None and got == want, (off, diff(got, want))


@pytest.mark.gpu
def test_shapes_a_text_that_ends_on_span_and_tile_borders(sctx):
    """Texts of exactly SPAN - 1, SPAN, SPAN + 1 and WG_TILE - 1, WG_TILE, WG_TILE + 1 bytes."""
    body = shaped_text(400, seed=77)
    recs = util.split_records(body, 1)
    for size in (SPAN - 1, SPAN, SPAN + 1, WG_TILE - 1, WG_TILE, WG_TILE + 1):
        fq, i = b"", 0
        while len(fq) + len(recs[i]) + 12 <= size:
            fq += recs[i]; i += 1
        hdr = b"@x" if (size - len(fq)) % 2 else b"@xy"                  # one last record of the bytes that are left, both lines alike
        n = (size - len(fq) - len(hdr) - 5) // 2
        fq += hdr + b"\n" + b"A" * n + b"\n+\n" + b"I" * n + b"\n"
        assert len(fq) == size
        got, want = _qlt_device(sctx, fq), ref_stats(fq)
        assert got == want, (size, diff(got, want))


@pytest.mark.gpu
def test_shapes_long_reads_fill_the_tail_entry(sctx):
    fq = capi.synth_fastq(6, 0, seed=8, kind=1)
    enc = sctx.encode_host(fq, level=3, block_reads=capi.BLOCK_AUTO, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN)
    want = ref_stats(fq)
    assert want.seq_len_min >= 10000 and list(want.cyc_n[:CYC]) == [6] * CYC and want.cyc_n[CYC] == want.qlt_bytes - 6 * CYC
    assert enc.stats == want, diff(enc.stats, want)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["constant", "binned"])
def test_skew_every_lane_on_one_counter(sctx, case):
    if case == "constant":                                            # every quality byte the same, every base 'A'
        fq = b"".join(b"@r%d\n" % i + b"A" * 150 + b"\n+\n" + b"F" * 150 + b"\n" for i in range(50000))
        got = _qlt_device(sctx, fq)
    else:
        fq = capi.synth_fastq(50000, 150, seed=9, kind=2)
        got = sctx.encode_host(fq, level=3, block_reads=capi.BLOCK_AUTO, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN).stats
    want = ref_stats(fq)
    assert sum(1 for v in want.qlt_hist if v) == (1 if case == "constant" else 4)
    assert got == want, diff(got, want)


def _blocks_of(fq):
    return max(1, (fq.count(b"\n") // 4) // 3)


# test_checksums.py's CASES, re-stated, and the small goldens
CASES = {
    "frozen": lambda: (capi.synth_fastq(20000, 150, seed=2), dict(level=3, block_reads=capi.BLOCK_AUTO, prior_step=capi.PRIOR_AUTO,
                                                                   tables=capi.TABLES_FROZEN)),
    "adaptive": lambda: (capi.synth_fastq(3000, 120, seed=21), dict(level=3, block_reads=256, tables=capi.TABLES_ADAPTIVE)),
    "segments": lambda: (capi.synth_fastq(60, 150, seed=5, kind=1), dict(level=3, block_reads=capi.BLOCK_AUTO, prior_step=capi.PRIOR_AUTO,
                                                                         tables=capi.TABLES_FROZEN)),
    "genome": lambda: (capi.synth_fastq(20000, 150, seed=4, kind=3), dict(level=3, block_reads=1000, prior_step=capi.PRIOR_AUTO,
                                                                          tables=capi.TABLES_FROZEN)),
    "format6_oversize": lambda: (util.golden_fastq("edge_oversize"), dict(level=3, block_reads=0)),
}
for _name in ("solid", "edge_lower", "edge_n", "edge_len", "edge_one"):
    CASES[_name] = (lambda n: lambda: (util.golden_fastq(n), dict(level=3, block_reads=_blocks_of(util.golden_fastq(n)))))(_name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_encode_counts_the_whole_input_and_changes_nothing(ctx, case):
    fq, kw = CASES[case]()
    off = ctx.encode_host(fq, **kw)
    assert off.stats is None and ctx.text_stats() is None
    ctx.set_stats(True)
    try:
        on = ctx.encode_host(fq, **kw)
    finally:
        ctx.set_stats(False)
    if case == "format6_oversize":                                    # the oversize records are counted too
        assert len(on.blocks) == 1 and on.blocks[0].size[capi.STREAM_NAMES.index("usr.lrec")] > 0
    want = ref_stats(fq)
    assert on.stats == want, diff(on.stats, want)
    assert on.clone().stats == want and on.clone().stats is not on.stats
    # the archive is the same with and without
    assert bytes(on.data) == bytes(off.data)
    assert bytes(on.blocks) == bytes(off.blocks)
    assert (on.first_hdrs, on.prior, on.chains, on.rec_prior) == (off.first_hdrs, off.prior, off.chains, off.rec_prior)


@pytest.mark.gpu
def test_switch_and_reuse_on_one_context(ctx):
    kw = dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN, chain_reads=32)
    a, b = capi.synth_fastq(3000, 120, seed=21), capi.synth_fastq(700, 90, seed=22, kind=2)
    assert ctx.encode_host(a, **kw).stats is None and ctx.text_stats() is None          # off
    ctx.set_stats(True)
    try:
        assert ctx.encode_host(a, **kw).stats == ref_stats(a)
        got = ctx.encode_host(b, **kw).stats                            # the accumulator is cleared per call
        assert got == ref_stats(b), diff(got, ref_stats(b))
        # a call that fails leaves none
        with pytest.raises(capi.SfqError) as e:
            ctx.encode_host(b"@r\nACGT\n+\nIIII\n@r2\n", **kw)
        assert e.value.code == -4 and ctx.text_stats() is None
        # the calls that only build priors compute none
        import torch
        t = torch.frombuffer(bytearray(a), dtype=torch.uint8).cuda()
        assert ctx.encode_host(a, **kw).stats is not None
        ctx.build_priors(t.data_ptr(), len(a), block_reads=256)
        assert ctx.text_stats() is None
        # with the checksums on as well: both right
        ctx.set_checksums(True)
        both = ctx.encode_host(a, **kw)
        ctx.set_checksums(False)
        assert both.stats == ref_stats(a) and both.text_crc == zlib.crc32(a) and len(both.crcs) == len(both.blocks)
        assert ctx.decode_host(both, level=3, out_cap=len(a) + 4096) == a
        assert ctx.text_stats() == ref_stats(a)                         # a decode is not an encode: the last encode's stand
    finally:
        ctx.set_stats(False)
        ctx.set_checksums(False)
    assert ctx.encode_host(a, **kw).stats is None and ctx.text_stats() is None          # off again


def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


@pytest.mark.gpu
def test_cli_stats_over_segments(tmp_path):
    """-Y -S 1: a segment per MiB of text; the archive's statistics are the merge of the calls'."""
    rng = np.random.default_rng(13)

    def reads(n, length, tag):
        out = []
        for i in range(n):
            out += [b"@%s.%d\n" % (tag, i), np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)].tobytes(), b"\n+\n",
                    rng.integers(ord("#"), ord("J"), length, dtype=np.uint8).tobytes(), b"\n"]
        return b"".join(out)
    # the shortest read lies in the first MiB, the longest in the middle: neither is the last slab's
    fq = reads(100, 120, b"a") + reads(1, 50, b"short") + reads(5000, 120, b"b") + reads(1, 200, b"long") + reads(3500, 150, b"c") + reads(4000, 130, b"d")
    assert 3.2e6 < len(fq) < 3.9e6
    src = tmp_path / "a.fq"; src.write_bytes(fq)
    arc, plain = tmp_path / "a.sfq", tmp_path / "plain.sfq"
    p = _run(["-Y", "-S", 1, "-q", "-u", src, "-f", arc])
    assert p.returncode == 0, p.stderr
    want = ref_stats(fq)
    assert (want.seq_len_min, want.seq_len_max) == (50, 200)
    out = _run(["-s", "-f", arc]).stderr.decode()
    info = dict(l.split("=", 1) for l in out.partition("\n:::: Files")[0].replace(" ", "").splitlines() if "=" in l)
    assert int(info["seg.count"]) >= 3
    assert out.partition("\n:::: Text ::::\n")[2].splitlines() == text_section(want)
    back = tmp_path / "back.fq"
    p = _run(["-d", "-f", arc, "-u", back])
    assert p.returncode == 0 and back.read_bytes() == fq, p.stderr
    # without -Y: no stream, no section
    p = _run(["-S", 1, "-q", "-u", src, "-f", plain])
    assert p.returncode == 0, p.stderr
    out = _run(["-s", "-f", plain]).stderr.decode()
    assert "txt.stat" not in out and ":::: Text" not in out
    # format 6 takes the switch too (the stream is beside the reference's own)
    f6, back6 = tmp_path / "f6.sfq", tmp_path / "back6.fq"
    small = reads(300, 100, b"e")
    src.write_bytes(small)
    p = _run(["-Y", "-B", 0, "-q", "-u", src, "-f", f6])
    assert p.returncode == 0, p.stderr
    out = _run(["-s", "-f", f6]).stderr.decode()
    assert "version          = 6" in out and out.partition("\n:::: Text ::::\n")[2].splitlines() == text_section(ref_stats(small))
    p = _run(["-d", "-f", f6, "-u", back6])
    assert p.returncode == 0 and back6.read_bytes() == small, p.stderr
    # -b: per process
    jobs = "%s\t%s\n" % (src, tmp_path / "b.sfq")
    p = _run(["-b", "-Y", "-O"], input=jobs.encode())
    assert p.stdout.decode().startswith("ok\t"), (p.stdout, p.stderr)
    assert _run(["-s", "-f", tmp_path / "b.sfq"]).stderr.decode().partition("\n:::: Text ::::\n")[2].splitlines() == text_section(ref_stats(small))

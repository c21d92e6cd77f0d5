"""Quality binning on the GPU (qmap.hip): sfq_map_qualities against ten lines of numpy over
fq.split(b"\\n"), on texts whose line ends fall on every border of the kernels; the switch on a context, which makes the host
encode entry code the mapped text and nothing else; the refusals; the CLI's -Q.  Every comparison is exact byte equality."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import util
from oracle import oracle as O
from slimfastq_amd import capi
from test_text_stats import ref_stats, diff

pytestmark = pytest.mark.gpu
CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")
# qmap.hip: a lane takes one aligned UNIT, a load instruction of a wavefront covers a ROW, a wavefront takes a SPAN of contiguous
# text and a workgroup four of them (WG_TILE); spans are laid from the aligned unit that holds the text's first byte
UNIT, ROW, SPAN, WG_TILE = 16, 1024, 16 << 10, 64 << 10
GUARD = 64
IDENTITY = bytes(range(256))
ILLUMINA8 = capi.quality_map_preset("illumina8")
NOVASEQ4 = capi.quality_map_preset("novaseq4")
E_ARG, E_UNSUPPORTED = -1, -7


def numpy_mapped(fq: bytes, lut: bytes) -> bytes:
    """The reference: every 4th line through the table."""
    t = np.frombuffer(lut, np.uint8)
    lines = fq.split(b"\n")
    lines[3::4] = [t[np.frombuffer(l, np.uint8)].tobytes() for l in lines[3::4]]
    return b"\n".join(lines)


def n_diff(a: bytes, b: bytes) -> int:
    assert len(a) == len(b)
    return int(np.count_nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8)))


def map_on_device(ctx, fq: bytes, lut: bytes, off=0):
    """sfq_map_qualities on a device copy of fq that starts off bytes behind a 16-byte boundary, GUARD bytes of 'I' (a byte the
    presets change) on either side: (the text afterwards, the count returned).  The guards must come back untouched."""
    import torch
    t = torch.full((len(fq) + 2 * GUARD + 32,), ord("I"), dtype=torch.uint8, device="cuda")
    base = (-t.data_ptr()) % 16 + GUARD + off
    assert (t.data_ptr() + base) % 16 == off
    t[base:base + len(fq)] = torch.frombuffer(bytearray(fq), dtype=torch.uint8).cuda()
    try:
        changed = ctx.map_qualities(t.data_ptr() + base, len(fq), lut)
    finally:
        back = t.cpu().numpy().tobytes()
        assert back[:base] == b"I" * base and back[base + len(fq):] == b"I" * (len(back) - base - len(fq)), "a guard byte was written"
    return back[base:base + len(fq)], changed


def check(ctx, fq, lut=ILLUMINA8, off=0, what=""):
    want = numpy_mapped(fq, lut)
    got, changed = map_on_device(ctx, fq, lut, off)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        bad = np.flatnonzero(a != b)
        raise AssertionError("%s off %d: %d bytes differ, the first at %d of %d" % (what, off, len(bad), bad[0], len(fq)))
    assert changed == n_diff(fq, want), (what, off)
    return want


def record(rng, length, hdr=None):
    return b"".join([hdr if hdr is not None else b"@r%d" % int(rng.integers(0, 10 ** int(rng.integers(1, 9)))), b"\n",
                     np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, length)].tobytes(), b"\n+\n",
                     rng.integers(ord("!"), ord("~") + 1, length, dtype=np.uint8).tobytes(), b"\n"])


def reads(nbytes, length, seed):
    """records of `length` bases until the text has at least nbytes bytes"""
    rng = np.random.default_rng(seed)
    out, n = [], 0
    while n < nbytes:
        out.append(record(rng, length))
        n += len(out[-1])
    return b"".join(out)


def sized_text(total, seed):
    """a text of exactly `total` bytes (>= 16): reads of 100 bases, and a last record that fills what is left"""
    rng = np.random.default_rng(seed)
    out, n = [], 0
    while total - n > 300:
        out.append(record(rng, 100))
        n += len(out[-1])
    left = total - n                                                   # = len(hdr) + 2 * length + 5
    hl = 2 if (left - 5) % 2 == 0 else 3
    out.append(record(rng, (left - 5 - hl) // 2, hdr=b"@" + b"h" * (hl - 1)))
    fq = b"".join(out)
    assert len(fq) == total
    return fq


def newline_at(pos, seed):
    """a text whose '\\n' in front of a quality line (the end of a '+' line) is byte `pos`; more records follow"""
    rng = np.random.default_rng(seed)
    fq = reads(pos - 400, 100, seed)
    hl = pos - len(fq) - 50 - 3                                        # hdr '\n' 50 bases '\n' '+' '\n'
    assert hl >= 2
    fq += record(rng, 50, hdr=b"@" + b"h" * (hl - 1)) + reads(3000, 100, seed + 1)
    lines_before = fq[:pos].count(b"\n")
    assert fq[pos] == 10 and lines_before % 4 == 2 and fq[pos - 1] == ord("+")
    return fq


@pytest.fixture
def qctx(ctx):
    """The session's context; no map installed afterwards, checksums and statistics off."""
    try:
        yield ctx
    finally:
        ctx.set_quality_map(None)
        ctx.set_checksums(False)
        ctx.set_stats(False)


# ---- sfq_map_qualities against numpy -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("length", (1, 15, 16, 17, 100, 150))
def test_reads_of_every_length_over_more_than_a_tile(ctx, length):
    fq = reads(WG_TILE + SPAN + 100, length, seed=length)
    starts, lens = util.line_table(fq)
    assert set((starts[3::4] % UNIT).tolist()) == set(range(UNIT))    # quality lines start at every offset of a unit
    check(ctx, fq, what="reads of %d" % length)


def test_long_reads_a_line_over_several_spans_and_a_tile(ctx):
    rng = np.random.default_rng(7)
    fq = b"".join(record(rng, n) for n in (40000, 150000, 70000, 3))
    assert 150000 > 2 * WG_TILE and 40000 > 2 * SPAN
    check(ctx, fq, what="long reads")
    check(ctx, capi.synth_fastq(6, 0, seed=8, kind=1), what="kind 1")


def test_empty_base_and_quality_lines(ctx):
    rng = np.random.default_rng(9)
    parts = []
    for i in range(3000):
        parts.append(b"@h\n\n+\n\n" if i % 3 else record(rng, int(rng.integers(0, 40))))
    fq = b"".join(parts)
    assert len(fq) > SPAN
    check(ctx, fq, what="empty lines")
    check(ctx, b"@h\n\n+\n\n" * 5000, what="empty lines alone")       # 16 line ends a unit: the kinds inside a unit go round


@pytest.mark.parametrize("size", (ROW, SPAN, WG_TILE))
def test_texts_that_end_on_and_around_every_border(ctx, size):
    for d in (-17, -1, 0, 1, 17):
        check(ctx, sized_text(size + d, seed=size + d), what="size %d%+d" % (size, d))


@pytest.mark.parametrize("border", (UNIT, ROW, SPAN))
def test_the_line_end_in_front_of_a_quality_line_on_either_side_of_a_border(ctx, border):
    at = 2 * SPAN + (3 * border if border != SPAN else 0)             # a border of that kind ...
    assert at % border == 0 and (border == SPAN or at % (border * 16) != 0)      # ... and of no larger kind
    for pos in (at - 1, at):                                           # the last byte in front of it, the first behind it
        check(ctx, newline_at(pos, seed=pos), what="line end at %d" % pos)


def test_small_texts(ctx):
    rng = np.random.default_rng(11)
    check(ctx, record(rng, 100), what="one record")
    check(ctx, b"@r\nA\n+\nI\n", what="9 bytes")
    assert len(b"@r\nACG\n+\nIJK\n") < UNIT
    check(ctx, b"@r\nACG\n+\nIJK\n", what="13 bytes")
    check(ctx, b"\n\n\nJ", what="4 bytes")


def test_a_text_without_a_final_line_end(ctx):
    fq = reads(SPAN + 500, 100, seed=12)[:-1]
    assert fq[-1] != 10
    want = check(ctx, fq, what="no final line end")
    assert want[-1] == ILLUMINA8[fq[-1]]                              # its last line is a line
    check(ctx, b"@r\nACGT\n+\nIIII", what="one record, no final line end")
    cut = reads(2000, 100, seed=13)[:-40]                              # the text stops inside a quality line
    check(ctx, cut, what="cut quality line")


@pytest.mark.parametrize("off", (0, 1, 7, 15))
def test_unaligned_buffers_and_guards(ctx, off):
    for what, fq in (("13 bytes", b"@r\nACG\n+\nIJK\n"), ("a row", sized_text(ROW - off, seed=20 + off)), ("reads of 150", reads(WG_TILE + 3000, 150, seed=21)),
                     ("a span less the offset", sized_text(SPAN - off, seed=22)), ("no final line end", reads(SPAN + 77, 100, seed=23)[:-1]),
                     ("empty lines", b"@h\n\n+\n\n" * 700)):
        check(ctx, fq, off=off, what=what)


# ---- counts and fixed points ---------------------------------------------------------------------------------------------------

def test_changed_counts_and_fixed_points(ctx):
    fq = reads(3 * SPAN, 100, seed=30)
    got, changed = map_on_device(ctx, fq, IDENTITY)
    assert got == fq and changed == 0
    binned = capi.synth_fastq(400, 100, seed=31, kind=2)
    got, changed = map_on_device(ctx, binned, NOVASEQ4, off=7)
    assert got == binned and changed == 0                             # such a text is a fixed point of the map
    for lut in (ILLUMINA8, NOVASEQ4):
        once = check(ctx, fq, lut, what="first application")
        assert once != fq
        twice, changed = map_on_device(ctx, once, lut)
        assert twice == once and changed == 0                         # idempotent


def test_a_refused_table_changes_nothing(qctx):
    ctx = qctx
    fq = reads(5000, 100, seed=32)
    for b, v in ((10, ord("I")), (13, ord("I")), (127, ord("I")), (ord("I"), 32)):
        bad = bytearray(IDENTITY); bad[b] = v
        with pytest.raises(capi.SfqError) as e:
            map_on_device(ctx, fq, bytes(bad))                         # (its finally clause checks the guards)
        assert e.value.code == E_ARG
        import torch
        t = torch.frombuffer(bytearray(fq), dtype=torch.uint8).cuda()
        with pytest.raises(capi.SfqError):
            ctx.map_qualities(t.data_ptr(), len(fq), bytes(bad))
        assert t.cpu().numpy().tobytes() == fq
        with pytest.raises(capi.SfqError) as e:
            ctx.set_quality_map(bytes(bad))
        assert e.value.code == E_ARG
    # ... and a refused table installs nothing: the encode is the plain text's
    plain = ctx.encode_host(fq, level=3, block_reads=64)
    assert same_archive(ctx.encode_host(fq, level=3, block_reads=64), plain) and ctx.quality_map_changed() == 0


# ---- the switch on a context -----------------------------------------------------------------------------------------------------

def same_archive(a, b):
    return (bytes(a.data) == bytes(b.data) and bytes(a.blocks) == bytes(b.blocks) and
            (a.first_hdrs, a.prior, a.chains, a.rec_prior) == (b.first_hdrs, b.prior, b.chains, b.rec_prior) and
            list(a.res.stream_bytes) == list(b.res.stream_bytes) and list(a.res.stream_offset) == list(b.res.stream_offset))


SWITCH = {
    "adaptive": lambda: (capi.synth_fastq(2000, 100, seed=40), dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO)),
    "frozen": lambda: (capi.synth_fastq(20000, 100, seed=41), dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN)),
    "one_block": lambda: (capi.synth_fastq(2000, 100, seed=42), dict(level=3, block_reads=0)),
}


@pytest.mark.parametrize("case", sorted(SWITCH))
def test_the_host_entry_codes_the_mapped_text(qctx, case):
    ctx = qctx
    fq, kw = SWITCH[case]()
    mapped = numpy_mapped(fq, ILLUMINA8)
    assert mapped != fq
    plain, want = ctx.encode_host(fq, **kw), ctx.encode_host(mapped, **kw)
    assert ctx.quality_map_changed() == 0 and not same_archive(plain, want)
    if case == "frozen":
        assert len(want.chains) > 0 and len(want.rec_prior) > 0
    ctx.set_quality_map(ILLUMINA8)
    got = ctx.encode_host(fq, **kw)
    assert same_archive(got, want)                                    # streams, block index, priors, chain index
    assert ctx.quality_map_changed() == n_diff(fq, mapped)
    assert ctx.decode_host(got, level=3, out_cap=len(fq) + 4096) == mapped
    assert ctx.quality_map_changed() == n_diff(fq, mapped)             # a decode is not an encode: the last encode's stands
    assert same_archive(ctx.encode_host(mapped, **kw), want) and ctx.quality_map_changed() == 0     # a fixed point
    ctx.set_quality_map(None)
    assert same_archive(ctx.encode_host(fq, **kw), plain) and ctx.quality_map_changed() == 0


def test_const_text_entries_refuse_while_a_map_is_installed(qctx):
    import torch
    ctx = qctx
    fq = capi.synth_fastq(600, 100, seed=43)
    t = torch.frombuffer(bytearray(fq), dtype=torch.uint8).cuda()
    cap = capi.lib().sfq_encode_bound(len(fq))
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    calls = {
        "sfq_encode_blocks": lambda: ctx.encode_device(t.data_ptr(), len(fq), out.data_ptr(), cap, level=3, block_reads=256),
        "sfq_encode_qlt_blocks": lambda: ctx.encode_device(t.data_ptr(), len(fq), out.data_ptr(), cap, level=3, block_reads=256, qlt_only=True),
        "sfq_build_priors": lambda: ctx.build_priors(t.data_ptr(), len(fq), block_reads=256),
        "sfq_count_priors": lambda: ctx.count_priors(t.data_ptr(), len(fq), block_reads=256),
    }
    before = {name: f() for name, f in calls.items()}                  # without a map they work
    ctx.set_quality_map(NOVASEQ4)
    for name, f in calls.items():
        with pytest.raises(capi.SfqError) as e:
            f()
        assert e.value.code == E_UNSUPPORTED and name in str(e.value) and "sfq_map_qualities" in str(e.value), name
    assert t.cpu().numpy().tobytes() == fq
    ctx.set_quality_map(None)
    assert calls["sfq_encode_blocks"]().total_bytes == before["sfq_encode_blocks"].total_bytes
    assert calls["sfq_build_priors"]() == before["sfq_build_priors"]
    calls["sfq_count_priors"]()
    # what the message advises: map the buffer, then the const entry codes the mapped text
    changed = ctx.map_qualities(t.data_ptr(), len(fq), NOVASEQ4)
    mapped = numpy_mapped(fq, NOVASEQ4)
    assert changed == n_diff(fq, mapped) and t.cpu().numpy().tobytes() == mapped
    res = calls["sfq_encode_blocks"]()
    want = ctx.encode_host(mapped, level=3, block_reads=256)
    assert out[:res.total_bytes].cpu().numpy().tobytes() == bytes(want.data)


def test_checksums_and_statistics_are_the_mapped_texts(qctx):
    ctx = qctx
    kw = dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN, chain_reads=32)
    fq = capi.synth_fastq(3000, 120, seed=44)
    mapped = numpy_mapped(fq, ILLUMINA8)
    ctx.set_checksums(True); ctx.set_stats(True); ctx.set_quality_map(ILLUMINA8)
    enc = ctx.encode_host(fq, **kw)
    assert enc.text_crc == zlib.crc32(mapped) != zlib.crc32(fq)
    bounds = [int(b.first_record) for b in enc.blocks]
    recs = util.split_records(mapped, 1)
    assert enc.crcs == [zlib.crc32(b"".join(recs[a:b])) for a, b in zip(bounds, bounds[1:] + [len(recs)])]
    want = ref_stats(mapped)
    assert enc.stats == want, diff(enc.stats, want)
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == mapped         # (the decode checks the block CRCs)


def test_it_pays(qctx):
    """stream_bytes[SFQ_S_QLT] of 20 000 kind-0 reads of 100 bases, frozen tables, with ILLUMINA8 against without: strictly smaller
    (the two sizes: DESIGN.md 4.13)."""
    ctx = qctx
    kw = dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN)
    fq = capi.synth_fastq(20000, 100, seed=45)
    qlt = capi.STREAM_NAMES.index("qlt")
    plain = int(ctx.encode_host(fq, **kw).res.stream_bytes[qlt])
    ctx.set_quality_map(ILLUMINA8)
    binned = int(ctx.encode_host(fq, **kw).res.stream_bytes[qlt])
    print("qlt stream: %d bytes plain, %d bytes with illumina8" % (plain, binned))
    assert binned < plain


# ---- the CLI -------------------------------------------------------------------------------------------------------------------

def _run(args, **kw):
    return subprocess.run([CLI] + [str(a) for a in args], capture_output=True, timeout=300, **kw)


def _info(path):
    out = _run(["-s", "-f", path]).stderr.decode()
    return dict(l.split("=", 1) for l in out.partition("\n:::: Files")[0].replace(" ", "").splitlines() if "=" in l)


def test_cli_quality_map(tmp_path):
    fq = capi.synth_fastq(2000, 100, seed=46)
    src = tmp_path / "a.fq"; src.write_bytes(fq)
    for name, lut, extra in (("illumina8", ILLUMINA8, []), ("illumina8", ILLUMINA8, ["-K", "-Y"]), ("novaseq4", NOVASEQ4, ["-B", 0])):
        mapped = numpy_mapped(fq, lut)
        arc, back = tmp_path / "a.sfq", tmp_path / "back.fq"
        p = _run(["-Q", name, "-q", "-O", "-u", src, "-f", arc] + extra)
        assert p.returncode == 0, p.stderr
        p = _run(["-d", "-O", "-f", arc, "-u", back])
        assert p.returncode == 0 and back.read_bytes() == mapped, (name, extra, p.stderr)
        info = _info(arc)
        assert info["qlt.map"] == name and int(info["qlt.map.changed"]) == n_diff(fq, mapped), info
        if "-K" in extra:
            assert int(info["crc32"], 16) == zlib.crc32(mapped)
        if 0 in extra:
            img = arc.read_bytes()
            assert info["version"] == "6" and O.decompress(img) == mapped
    assert src.read_bytes() == fq                                     # the input file is read, never written
    # without -Q: neither key
    plain = tmp_path / "plain.sfq"
    assert _run(["-q", "-u", src, "-f", plain]).returncode == 0
    assert "qlt.map" not in _info(plain) and "qlt.map.changed" not in _info(plain)
    # -b: the map is the process's, set for every job
    jobs = "%s\t%s\n" % (src, tmp_path / "b.sfq")
    p = _run(["-b", "-Q", "illumina8", "-O"], input=jobs.encode())
    assert p.returncode == 0 and p.stdout.startswith(b"ok\t"), (p.stdout, p.stderr)
    assert _info(tmp_path / "b.sfq")["qlt.map"] == "illumina8"
    p = _run(["-d", "-O", "-f", tmp_path / "b.sfq", "-u", tmp_path / "b.fq"])
    assert p.returncode == 0 and (tmp_path / "b.fq").read_bytes() == numpy_mapped(fq, ILLUMINA8)


def test_the_reference_decodes_a_one_block_archive_with_the_new_keys(tmp_path):
    if not O.ref_binary():
        pytest.skip("the compiled reference is not here")
    fq = capi.synth_fastq(1500, 100, seed=47)
    src = tmp_path / "a.fq"; src.write_bytes(fq)
    arc = tmp_path / "a.sfq"
    p = _run(["-Q", "illumina8", "-B", 0, "-q", "-u", src, "-f", arc])
    assert p.returncode == 0, p.stderr
    assert O.ref_decompress(arc.read_bytes()) == numpy_mapped(fq, ILLUMINA8)

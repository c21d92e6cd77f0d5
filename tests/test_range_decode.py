"""A window of a call's blocks without the rest (sfq_decode_block_range[_host], the CLI's -R): the bytes, the counts, and -- through
sfq_result.n_chains -- that the quality chains outside the window were not decoded."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import util
from slimfastq_amd import capi
from test_gpu_parity import _cli, _quirk_fastq

pytestmark = pytest.mark.gpu

NB = 64                         # blocks per archive: seven generations of the base model (1, 1, 2, 4, 8, 16, 32 blocks)
GUARD = 4096


def _genome_reads(n, read_len, genome_len, seed):
    """n reads of read_len bases from either strand of a random genome, 0.5 % substitutions: bases the match model takes."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_len, dtype=np.uint8)
    pos = rng.integers(0, genome_len - read_len, n)
    rev = rng.random(n) < 0.5
    idx = pos[:, None] + np.arange(read_len)[None, :]
    b = genome[idx]
    b = np.where(rev[:, None], 3 - b[:, ::-1], b)
    sub = rng.random(b.shape) < 0.005
    b = np.where(sub, (b + rng.integers(1, 4, b.shape)) & 3, b)
    seqs = np.frombuffer(b"ACGT", np.uint8)[b]
    quals = (33 + rng.integers(2, 41, b.shape)).astype(np.uint8)
    out = []
    for i in range(n):
        out += [b"@g%d:%d:%d" % (i, 1000 + i % 7, i * 3), seqs[i].tobytes(), b"+", quals[i].tobytes()]
    return b"\n".join(out) + b"\n"


FROZEN = dict(level=3, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN)
_texts = {}


def _text(key, make):
    if key not in _texts:
        _texts[key] = make()
    return _texts[key]


def _case(name):
    """(text, encode arguments, (chn.idx flag bits that must be set, bits that must be clear) or None for adaptive tables)"""
    if name == "adaptive":
        return capi.synth_fastq(4096, 150, seed=31), dict(level=3, block_reads=64, tables=capi.TABLES_ADAPTIVE), None
    if name == "frozen_flat":
        return capi.synth_fastq(4096, 150, seed=31), dict(block_reads=64, **FROZEN), (0x80, 0x01)
    if name == "frozen_match":
        return _text("genome", lambda: _genome_reads(4096, 150, 2000, 7)), dict(block_reads=64, **FROZEN), (0x21, 0)
    if name == "frozen_kernel2":
        return _text("genome", lambda: _genome_reads(4096, 150, 2000, 7)), dict(block_reads=64, kernel=2, **FROZEN), (0x01, 0x20)
    if name == "segments":
        return capi.synth_fastq(128, 150, seed=5, kind=1), dict(block_reads=2, **FROZEN), (0x08, 0)
    if name == "hostile_frozen":
        return _text("hostile", lambda: _quirk_fastq(4090, 9)), dict(block_reads=64, chain_reads=16, **FROZEN), (0, 0)
    if name == "hostile_adaptive":
        return _text("hostile", lambda: _quirk_fastq(4090, 9)), dict(level=3, block_reads=64, tables=capi.TABLES_ADAPTIVE), None
    raise KeyError(name)


CASES = ("adaptive", "frozen_flat", "frozen_match", "frozen_kernel2", "segments", "hostile_frozen", "hostile_adaptive")
_archives = {}


@pytest.fixture(scope="module")
def archive(ctx):
    """name -> (text, the text's blocks, Encoded with per-block CRCs, chains per block or None): encoded once per module, checksums on."""
    def get(name):
        if name not in _archives:
            fq, kw, flags = _case(name)
            ctx.set_checksums(True)
            try:
                enc = ctx.encode_host(fq, **kw)
            finally:
                ctx.set_checksums(False)
            assert len(enc.blocks) == NB and enc.crcs is not None and len(enc.crcs) == NB
            chunks = util.split_records(fq, kw["block_reads"])
            assert len(chunks) == NB
            qchains = None
            if flags is not None:
                ci = util.unpack_chains(enc.chains, nblocks=NB)
                assert ci["flags"] & flags[0] == flags[0] and ci["flags"] & flags[1] == 0, "chn.idx flags %#x" % ci["flags"]
                if ci["flags"] & 8:
                    qchains = list(ci["seg_blocks"])
                else:
                    cr = ci["chain_reads"]
                    qchains = [(enc.blocks[b].n_records + cr - 1) // cr for b in range(NB)]
                assert sum(qchains) == len(ci["qlt"])
            else:
                assert enc.chains == b""
            _archives[name] = (fq, chunks, enc, qchains)
        return _archives[name]
    yield get
    _archives.clear()
    _texts.clear()


WINDOWS = ((0, 1), (1, 1), (2, 2), (31, 2), (NB - 1, 1), (5, 20), (0, NB))


def _device_parts(enc):
    import torch
    d = torch.from_numpy(np.frombuffer(enc.data, np.uint8).copy()).cuda()
    return d, dict(prior=enc.prior, chains=enc.chains, rec_prior=enc.rec_prior, level=3)


def _range_device(ctx, enc, d, kw, b0, n, nbytes, crcs=None):
    """The device entry into a guarded buffer of exactly nbytes: (text, Result); the guards must come back untouched."""
    import torch
    buf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    got, res = ctx.decode_range_device(enc.blocks, enc.first_hdrs, d.data_ptr(), list(enc.res.stream_offset), b0, n,
                                       buf.data_ptr() + GUARD, nbytes, crcs=crcs, **kw)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all()), "guard region written"
    return buf[GUARD:GUARD + got].cpu().numpy().tobytes(), res


@pytest.mark.parametrize("name", CASES)
def test_windows_give_their_blocks_and_decode_no_other_quality_chain(ctx, archive, name):
    fq, chunks, enc, qchains = archive(name)
    d, kw = _device_parts(enc)
    whole = ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096)
    assert whole == fq
    for b0, n in WINDOWS:
        want = b"".join(chunks[b0:b0 + n])
        nrec = sum(enc.blocks[b].n_records for b in range(b0, b0 + n))
        # exact capacity, guards on either side, the window's checksums installed
        got, res = _range_device(ctx, enc, d, kw, b0, n, len(want), crcs=enc.crcs[b0:b0 + n])
        assert got == want, (name, b0, n)
        assert res.n_records == nrec and res.n_blocks == n and res.total_bytes == len(want), (name, b0, n)
        assert res.n_chains == (sum(qchains[b0:b0 + n]) if qchains is not None else 0), (name, b0, n)
        crcs, _ = ctx.checksums()
        assert crcs == enc.crcs[b0:b0 + n], (name, b0, n)
        # the host entry: the same bytes
        got_h, res_h = ctx.decode_range_host(enc, b0, n, out_cap=len(want))
        assert got_h == want and res_h.n_records == nrec and res_h.n_chains == res.n_chains, (name, b0, n)
        if (b0, n) == (0, NB):
            assert got == whole
    # the short last block
    if enc.blocks[NB - 1].n_records != enc.blocks[0].n_records:
        assert len(chunks[-1]) < len(chunks[0])


@pytest.mark.parametrize("name", ("adaptive", "frozen_match", "segments"))
def test_one_byte_too_little_reports_the_size_needed(ctx, archive, name):
    fq, chunks, enc, _ = archive(name)
    d, kw = _device_parts(enc)
    import torch
    for b0, n in ((2, 2), (NB - 1, 1)):
        want = b"".join(chunks[b0:b0 + n])
        buf = torch.full((GUARD + len(want) + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.set_priors(enc.prior, enc.rec_prior)
        L = capi.lib()
        assert L.sfq_set_chain_index(ctx.handle, enc.chains if enc.chains else None, len(enc.chains)) == 0
        p = capi.Params(3, 0, 0, 0, 0, 0, 0, 0, 0, 0)
        nout = C.c_uint64()
        fb = np.frombuffer(enc.first_hdrs, np.uint8)
        soff = (C.c_uint64 * capi.NSTREAMS)(*list(enc.res.stream_offset))
        rc = L.sfq_decode_block_range(ctx.handle, C.byref(p), enc.blocks, NB, fb.ctypes.data_as(C.c_void_p), len(enc.first_hdrs),
                                      C.c_void_p(d.data_ptr()), soff, b0, n, C.c_void_p(buf.data_ptr() + GUARD), len(want) - 1, C.byref(nout), None)
        torch.cuda.synchronize()
        assert rc == -5 and nout.value == len(want), (name, b0, n, rc, nout.value)
        assert bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + len(want) - 1:] == 0xA5).all())
        got, _ = _range_device(ctx, enc, d, kw, b0, n, len(want))
        assert got == want


def test_argument_errors_leave_the_context_usable(ctx, archive):
    fq, chunks, enc, _ = archive("frozen_flat")
    d, kw = _device_parts(enc)
    for b0, n in ((0, 0), (5, 0), (NB, 1), (NB - 1, 2), (0, NB + 1), (0xFFFFFFFF, 2)):
        with pytest.raises(capi.SfqError) as e:
            _range_device(ctx, enc, d, kw, b0, n, 1 << 16)
        assert e.value.code == -1, (b0, n)
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_range_host(enc, b0, n, out_cap=1 << 16, crcs=[])
        assert e.value.code == -1, (b0, n)
    # checksums that are not the window's count
    with pytest.raises(capi.SfqError) as e:
        _range_device(ctx, enc, d, kw, 3, 2, 1 << 20, crcs=enc.crcs[3:6])
    assert e.value.code == -1
    with pytest.raises(capi.SfqError) as e:
        _range_device(ctx, enc, d, kw, 3, 2, 1 << 20, crcs=enc.crcs)
    assert e.value.code == -1
    want = b"".join(chunks[3:5])
    got, _ = _range_device(ctx, enc, d, kw, 3, 2, len(want), crcs=enc.crcs[3:5])
    assert got == want
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq


def test_a_one_block_archive_with_oversize_records_is_refused(ctx):
    fq = util.golden_fastq("edge_oversize")
    enc = ctx.encode_host(fq, level=3, block_reads=0)
    assert enc.res.stream_bytes[capi.STREAM_NAMES.index("usr.lrec")] > 0
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_range_host(enc, 0, 1, out_cap=2 * len(fq) + 4096)
    assert e.value.code == -7
    # a one-block archive without them: the window is the archive
    fq = capi.synth_fastq(500, 100, seed=3)
    enc = ctx.encode_host(fq, level=3, block_reads=0)
    got, res = ctx.decode_range_host(enc, 0, 1, out_cap=len(fq))
    assert got == fq and res.n_records == 500 and res.n_chains == 0


@pytest.mark.parametrize("name", ("frozen_flat", "frozen_match"))
def test_a_flipped_byte_is_caught_by_the_window_that_holds_it_and_by_no_other(ctx, archive, name):
    fq, chunks, enc, qchains = archive(name)
    ci = util.unpack_chains(enc.chains, nblocks=NB)
    bad_block = 33
    c = sum(qchains[:bad_block]) + qchains[bad_block] // 2             # a quality chain of the block, a byte in its middle
    at = enc.res.stream_offset[capi.STREAM_NAMES.index("qlt")] + int(ci["qlt"][:c].sum()) + int(ci["qlt"][c]) // 2
    bad = enc.clone()
    bad.data = np.array(bad.data, copy=True)
    bad.data[at] ^= 0x5A
    for b0, n in ((33, 1), (31, 4), (20, 20)):
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_range_host(bad, b0, n, out_cap=len(fq))
        msg = str(e.value)
        assert e.value.code == -6 and ("block %d " % bad_block in msg or "block %d:" % bad_block in msg), msg
    for b0, n in ((0, 33), (34, 30), (32, 1), (5, 20)):
        got, _ = ctx.decode_range_host(bad, b0, n, out_cap=len(fq))
        assert got == b"".join(chunks[b0:b0 + n]), (b0, n)


def test_cli_ranges(tmp_path):
    cli = _cli()
    fq = capi.synth_fastq(4096, 150, seed=12)
    recs = util.split_records(fq, 1)
    src = tmp_path / "in.fq"; src.write_bytes(fq)
    for extra, tag in ((["-K"], "k"), ([], "plain")):
        sfq = tmp_path / (tag + ".sfq")
        subprocess.check_call([cli, "-u", str(src), "-f", str(sfq), "-O", "-F", "-B", "64", "-S", "1"] + extra)
        p = subprocess.run([cli, "-s", "-f", str(sfq)], capture_output=True)
        info = dict(l.split("=", 1) for l in p.stderr.decode("latin1").replace(" ", "").splitlines() if "=" in l)
        assert int(info["seg.count"]) >= 2

        def run(first, count):
            """-d -R first:count -> how many segments the run decoded (a -z line per library call)"""
            out = tmp_path / "out.fq"
            p = subprocess.run([cli, "-d", "-z", "-R", "%d:%d" % (first, count), "-f", str(sfq), "-u", str(out), "-O"], capture_output=True, check=True)
            assert out.read_bytes() == b"".join(recs[first:first + count]), (tag, first, count)
            return p.stderr.count(b"sfq_decode_blocks_host")
        assert run(100, 300) == 1                                      # (a slab of 1 MiB holds some 3000 of these records)
        # ranges of 300 records that overlap by 50 and cover the file: whatever record a segment starts at lies inside one of them
        touched = [run(first, 300) for first in range(100, 4096, 250)]
        assert max(touched) == 2 and min(touched) == 1, touched
        for first, count in ((0, 1), (4095, 1), (63, 2), (0, 4096)):
            run(first, count)
        p = subprocess.run([cli, "-d", "-R", "4000:1000", "-f", str(sfq)], capture_output=True, check=True)
        assert p.stdout == b"".join(recs[4000:])
        out = tmp_path / "none.fq"
        p = subprocess.run([cli, "-d", "-R", "5000:1", "-f", str(sfq), "-u", str(out), "-O"], capture_output=True)
        assert p.returncode == 1 and b"4096 records" in p.stderr and not out.exists()
        p = subprocess.run([cli, "-d", "-R", "4096:1", "-f", str(sfq)], capture_output=True)
        assert p.returncode == 1
    # a format-6 archive: decoded whole and trimmed
    leg = tmp_path / "v6.sfq"
    subprocess.check_call([cli, "-u", str(src), "-f", str(leg), "-O", "-B", "0", "-q"])
    p = subprocess.run([cli, "-d", "-R", "1000:10", "-f", str(leg)], capture_output=True, check=True)
    assert p.stdout == b"".join(recs[1000:1010])
    # ... unless it holds oversize records
    over = tmp_path / "over.fq"; over.write_bytes(util.golden_fastq("edge_oversize"))
    osfq = tmp_path / "over.sfq"
    subprocess.check_call([cli, "-u", str(over), "-f", str(osfq), "-O", "-B", "0", "-q"])
    p = subprocess.run([cli, "-d", "-R", "0:1", "-f", str(osfq)], capture_output=True)
    assert p.returncode == 1 and b"oversize" in p.stderr
    # batch mode: the range applies to every job
    jobs = "%s\t%s\n%s\t%s\n" % (tmp_path / "k.sfq", tmp_path / "b1.out", tmp_path / "plain.sfq", tmp_path / "b2.out")
    p = subprocess.run([cli, "-b", "-d", "-O", "-R", "1500:700"], input=jobs.encode(), capture_output=True)
    assert p.returncode == 0, p.stdout
    assert (tmp_path / "b1.out").read_bytes() == (tmp_path / "b2.out").read_bytes() == b"".join(recs[1500:2200])

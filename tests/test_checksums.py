"""CRC-32 checksums of the text (crc.hip): the device pass against zlib.crc32, the per-block values of an
encode, the check of a decode, and what they catch of a damaged archive."""
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import util
from slimfastq_amd import capi
from test_kernel_resources import kernel_metadata


# ---- CPU -------------------------------------------------------------------------------------------------------------------

def test_crc32_combine_matches_zlib():
    rnd = random.Random(7)
    for n in (0, 1, 2, 15, 16, 17, 1000, 70000):
        buf = bytes(rnd.getrandbits(8) for _ in range(n))
        for cut in sorted({0, n, n // 2, rnd.randint(0, n)}):
            a, b = buf[:cut], buf[cut:]
            assert capi.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(buf), (n, cut)
    assert capi.crc32_combine(0x12345678, 0, 0) == 0x12345678


def test_crc_kernels_use_no_scratch(tmp_path):
    meta = kernel_metadata("crc.hip", tmp_path)
    for want in ("k_crc_tiles", "k_crc_groups", "k_crc_ranges", "k_crc_block_bounds"):
        hits = [(k, v) for k, v in meta.items() if want in k]
        assert hits, want
        for name, (vgprs, scratch) in hits:
            assert scratch == 0 and vgprs <= 128, (name, vgprs, scratch)


# ---- GPU: the pass itself ----------------------------------------------------------------------------------------------------

def _device(buf: bytes):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


@pytest.mark.gpu
def test_crc32_small_ranges_and_tile_borders(ctx):
    rnd = random.Random(3)
    buf = bytes(rnd.getrandbits(8) for _ in range(3 * 4096 * 64 + 5000))
    t = _device(buf)
    p = t.data_ptr()
    # empty and one-byte ranges
    bounds = [0, 0, 1, 1, 2, 3, 3, 100, 101]
    assert ctx.crc32(p, bounds) == [zlib.crc32(buf[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    # every start and end offset mod 64 around tile borders (4 KiB) and group borders (256 KiB)
    for border in (4096, 8192, 4096 * 64, 4096 * 65):
        for s in range(border - 64, border + 1):
            bounds = [s - 40, s, s + 1, s + 4096 + (s % 64), s + 3 * 4096 + 64 + (s % 16)]
            assert ctx.crc32(p, bounds) == [zlib.crc32(buf[a:b]) for a, b in zip(bounds[:-1], bounds[1:])], (border, s)
    # ranges that start off the buffer's own 16-byte grid
    for off in (1, 7, 15, 17):
        bounds = [off, off + 5, off + 4096 * 3 + 9, off + 4096 * 70 + 1, len(buf)]
        assert ctx.crc32(p, bounds) == [zlib.crc32(buf[a:b]) for a, b in zip(bounds[:-1], bounds[1:])], off
    with pytest.raises(capi.SfqError):
        ctx.crc32(p, [10, 5])


@pytest.mark.gpu
def test_crc32_ten_thousand_ragged_ranges(ctx):
    rnd = random.Random(5)
    sizes = [rnd.choice((0, 1, 17, 4095, 4096, 4097, 65536, 376 << 10)) + rnd.randrange(3000) for _ in range(10000)]
    n = sum(sizes)
    buf = np.random.default_rng(1).integers(0, 256, n + 100, dtype=np.uint8).tobytes()
    t = _device(buf)
    bounds = [37]
    for s in sizes:
        bounds.append(bounds[-1] + s)
    got = ctx.crc32(t.data_ptr(), bounds)
    want = [zlib.crc32(buf[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
    assert got == want


@pytest.mark.gpu
def test_crc32_one_300mb_range(ctx):
    import torch
    g = torch.Generator(device="cuda").manual_seed(9)
    t = torch.randint(0, 256, (300_000_003,), dtype=torch.uint8, device="cuda", generator=g)
    buf = t.cpu().numpy().tobytes()
    assert ctx.crc32(t.data_ptr(), [0, len(buf)]) == [zlib.crc32(buf)]
    assert ctx.crc32(t.data_ptr(), [3, len(buf) - 5]) == [zlib.crc32(buf[3:-5])]


# ---- GPU: encode and decode ---------------------------------------------------------------------------------------------------

def _block_ranges(fq: bytes, enc):
    """Byte ranges of the blocks: from each block's first record to the next block's."""
    starts = [0]
    nl = np.flatnonzero(np.frombuffer(fq, np.uint8) == 10)
    rec_start = np.concatenate(([0], nl[3::4][:-1] + 1))
    for b in range(1, len(enc.blocks)):
        starts.append(int(rec_start[enc.blocks[b].first_record]))
    return list(zip(starts, starts[1:] + [len(fq)]))


def _encode_both(ctx, fq, **kw):
    off = ctx.encode_host(fq, **kw)
    assert off.crcs is None
    ctx.set_checksums(True)
    try:
        on = ctx.encode_host(fq, **kw)
    finally:
        ctx.set_checksums(False)
    return off, on


def _without_crcs(enc):
    c = enc.clone()
    c.crcs = None
    return c


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


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_encode_checksums_cover_the_blocks_and_change_nothing(ctx, case):
    fq, kw = CASES[case]()
    off, on = _encode_both(ctx, fq, **kw)
    assert on.crcs is not None and len(on.crcs) == len(on.blocks)
    if case == "format6_oversize":
        assert len(on.blocks) == 1 and on.blocks[0].size[capi.STREAM_NAMES.index("usr.lrec")] > 0
    assert on.crcs == [zlib.crc32(fq[a:b]) for a, b in _block_ranges(fq, on)]
    assert on.text_crc == zlib.crc32(fq)
    # the archive is the same with and without
    assert bytes(on.data) == bytes(off.data)
    assert bytes(on.blocks) == bytes(off.blocks)
    assert (on.first_hdrs, on.prior, on.chains, on.rec_prior) == (off.first_hdrs, off.prior, off.chains, off.rec_prior)
    # a decode with the encoder's values installed gives the text back, and reports the same values
    assert ctx.decode_host(on, level=3, out_cap=len(fq) + 4096) == fq
    assert ctx.checksums() == (on.crcs, on.text_crc)


@pytest.mark.gpu
def test_decode_checks_the_installed_checksums(ctx):
    fq = capi.synth_fastq(3000, 120, seed=21)
    _, enc = _encode_both(ctx, fq, level=3, block_reads=256, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN, chain_reads=32)
    assert len(enc.crcs) > 3
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq
    bad = enc.clone()
    bad.crcs[2] ^= 0x10
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(bad, level=3, out_cap=len(fq) + 4096)
    assert e.value.code == -6 and "block 2 " in str(e.value) and "%08x" % bad.crcs[2] in str(e.value)
    got, _ = ctx.checksums()
    assert got == enc.crcs                                          # what was computed, every block
    # the values were the failed call's: the next decode checks nothing, and the intact archive decodes
    assert ctx.decode_host(_without_crcs(enc), level=3, out_cap=len(fq) + 4096) == fq
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq
    # a count that is not the call's
    ctx.set_block_checksums(enc.crcs[:-1])
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(_without_crcs(enc), level=3, out_cap=len(fq) + 4096)
    assert e.value.code == -1


@pytest.mark.gpu
def test_installed_checksums_do_not_outlive_a_call_that_fails_early(ctx):
    """Installed values belong to the next decode call even where it returns before decoding (the host entry's check of the
    stream bounds, a null argument): the call after it must not check its text against them."""
    import ctypes as C
    fq = capi.synth_fastq(3000, 120, seed=21)
    kw = dict(level=3, block_reads=256, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN, chain_reads=32)
    _, enc = _encode_both(ctx, fq, **kw)
    fq2 = capi.synth_fastq(3000, 120, seed=22)
    other = ctx.encode_host(fq2, **kw)                            # as many blocks, other text, no checksums
    assert len(other.blocks) == len(enc.blocks) and other.crcs is None
    bad = enc.clone()
    bad.data = bad.data[:len(bad.data) // 2]
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_host(bad, level=3, out_cap=len(fq) + 4096)
    assert e.value.code == -6 and "block index" in str(e.value)     # refused before the decode proper
    assert ctx.decode_host(other, level=3, out_cap=len(fq2) + 4096) == fq2
    # a null argument
    ctx.set_block_checksums(enc.crcs)
    p = capi.Params(3, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    n = C.c_uint64()
    rc = capi.lib().sfq_decode_blocks_host(ctx.handle, C.byref(p), enc.blocks, len(enc.blocks), None, 0, None, 0,
                                          (C.c_uint64 * capi.NSTREAMS)(), None, 0, C.byref(n), None)
    assert rc == -1
    assert ctx.decode_host(other, level=3, out_cap=len(fq2) + 4096) == fq2
    ctx.set_block_checksums(enc.crcs)
    rc = capi.lib().sfq_decode_blocks(ctx.handle, None, enc.blocks, len(enc.blocks), None, 0, None,
                                      (C.c_uint64 * capi.NSTREAMS)(), None, 0, C.byref(n), None)
    assert rc == -1
    assert ctx.decode_host(other, level=3, out_cap=len(fq2) + 4096) == fq2


@pytest.mark.gpu
def test_damaged_archives_with_checksums_fail_or_decode_exactly(ctx):
    """test_gpu_parity.py::test_corrupt_archives_fail_cleanly_or_decode_to_something's damage, on its input and seeds: with the
    encoder's checksums installed, every decode either fails or gives back exactly the original text."""
    rnd = random.Random(11)
    fq = capi.synth_fastq(3000, 120, seed=21)
    for tables in (capi.TABLES_FROZEN, capi.TABLES_ADAPTIVE):
        _, enc = _encode_both(ctx, fq, level=3, block_reads=256, prior_step=capi.PRIOR_AUTO, tables=tables, chain_reads=32)
        assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq
        outcomes = {"error": 0, "same": 0}
        for trial in range(60):
            bad = enc.clone()
            kind = trial % 6
            if kind == 0:
                data = bytearray(bad.data)
                for _ in range(rnd.randint(1, 8)):
                    data[rnd.randrange(len(data))] ^= 1 << rnd.randrange(8)
                bad.data = bytes(data)
            elif kind == 1:
                b = bad.blocks[rnd.randrange(len(bad.blocks))]
                what = rnd.randrange(5)
                if what == 0: b.llen = rnd.choice((0, 1, 119, 121, 5000))
                elif what == 1: b.hdr_bytes = rnd.choice((0, 1, 7, 1 << 20))
                elif what == 2: b.two_id ^= 1
                elif what == 3: b.solid ^= 1
                else: b.n_byte = rnd.randrange(256)
            elif kind == 2 and bad.chains:
                ch = bytearray(bad.chains)
                i = rnd.randrange(4, max(5, len(ch) - 2))
                if 1 < ch[i] < 0x7f and 1 < ch[i + 1] < 0x7f: ch[i] -= 1; ch[i + 1] += 1
                bad.chains = bytes(ch)
            elif kind == 3 and bad.prior:
                pr = bytearray(bad.prior); pr[rnd.randrange(len(pr))] ^= 0x55; bad.prior = bytes(pr)
            elif kind == 4 and bad.rec_prior:
                pr = bytearray(bad.rec_prior); pr[rnd.randrange(len(pr))] ^= 0x33; bad.rec_prior = bytes(pr)
            else:
                bad.data = bad.data[:rnd.randrange(len(bad.data) // 2, len(bad.data))]
            try:
                out = ctx.decode_host(bad, level=3, out_cap=2 * len(fq) + 4096)
            except capi.SfqError:
                outcomes["error"] += 1
                continue
            assert out == fq, "trial %d (kind %d) decoded to other text without an error" % (trial, kind)
            outcomes["same"] += 1
        assert outcomes["error"] > 0
        assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq


# ---- the CLI -------------------------------------------------------------------------------------------------------------

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slimfastq_amd", "bin", "slimfastq-amd")


def test_cli_refuses_checksums_for_format_6_before_touching_a_gpu(tmp_path):
    src = tmp_path / "a.fq"; src.write_bytes(b"@r\nACGT\n+\nIIII\n")
    p = subprocess.run([CLI, "-K", "-B", "0", "-u", str(src), "-f", str(tmp_path / "a.sfq")], capture_output=True)
    assert p.returncode == 1 and b"-K" in p.stderr and b"block format" in p.stderr
    assert b"HIP device" not in p.stderr and not (tmp_path / "a.sfq").exists()
    p = subprocess.run([CLI, "-h"], capture_output=True)
    assert p.returncode == 0 and b"\n-K " in p.stdout


@pytest.mark.gpu
def test_cli_checksum_round_trip_segments_and_forgery(tmp_path):
    from oracle import oracle as O
    fq = capi.synth_fastq(25000, 150, seed=12)                 # ~8 MB: eight 1 MiB segments
    src = tmp_path / "a.fq"; src.write_bytes(fq)
    plain, ck = tmp_path / "plain.sfq", tmp_path / "ck.sfq"
    subprocess.run([CLI, "-u", str(src), "-f", str(plain), "-S", "1", "-q"], check=True)
    subprocess.run([CLI, "-K", "-u", str(src), "-f", str(ck), "-S", "1", "-q"], check=True)
    a, b = O.parse(plain.read_bytes()), O.parse(ck.read_bytes())
    assert int(b.info["seg.count"]) > 4
    extra = {k: v for k, v in b.streams.items() if k not in a.streams}
    assert set(extra) == {"blk.crc"} and all(b.streams[k] == v for k, v in a.streams.items() if k != "<info>")
    assert len(extra["blk.crc"]) == 4 * int(b.info["blk.count"])
    assert {k: v for k, v in b.info.items() if k not in ("crc32", "comp.size")} == {k: v for k, v in a.info.items() if k != "comp.size"}
    assert "crc32" not in a.info and int(b.info["crc32"], 16) == zlib.crc32(fq) and len(b.info["crc32"]) == 8
    p = subprocess.run([CLI, "-s", "-f", str(ck)], capture_output=True, check=True)
    assert ("%08x" % zlib.crc32(fq)).encode() in p.stderr
    for arc in (ck, plain):                                    # an archive without blk.crc decodes as before
        out = tmp_path / (arc.name + ".fq")
        subprocess.run([CLI, "-d", "-f", str(arc), "-u", str(out)], check=True)
        assert out.read_bytes() == fq
    # one block's checksum changed: -d exits 1 naming the block, -b answers fail and goes on
    img = bytearray(ck.read_bytes())
    at = bytes(img).find(extra["blk.crc"])
    assert at > 0 and bytes(img).find(extra["blk.crc"], at + 1) < 0
    img[at + 4 * (int(b.info["blk.count"]) // 2)] ^= 0x01
    forged = tmp_path / "forged.sfq"; forged.write_bytes(bytes(img))
    p = subprocess.run([CLI, "-d", "-f", str(forged), "-u", str(tmp_path / "f.fq")], capture_output=True)
    assert p.returncode == 1 and b"checksum: block" in p.stderr and b"segment " in p.stderr and b"archive blocks" in p.stderr, p.stderr
    jobs = "%s\t%s\n%s\t%s\n" % (forged, tmp_path / "b1.fq", ck, tmp_path / "b2.fq")
    p = subprocess.run([CLI, "-b", "-d"], input=jobs.encode(), capture_output=True)
    lines = p.stdout.decode().splitlines()
    assert lines[0].startswith("fail\t") and "checksum" in lines[0] and lines[1].startswith("ok\t"), lines
    assert (tmp_path / "b2.fq").read_bytes() == fq

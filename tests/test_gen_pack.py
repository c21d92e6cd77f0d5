"""Bases without a model (block format 10, "chn.idx" flag bit 7) are packed by k_gen_pack_raw (chains.hip): a wavefront per chain, a lane per
output dword of sixteen bases.  The bytes are the pack's -- two bits a base, four a byte, the first in the low bits, across the records' ends,
the last byte padded with zeros -- stated here in numpy, and the oracle's (check_against_oracle) where the input allows it; the edges the lane's
dword meets: lines that end inside a dword, records shorter than a dword (an empty base line is refused by the framing), chains of one record or of more than 64 (two chunks of the
wave's prefix), unusual characters at every position of a dword, the last line of the text, colour space and segments of long reads."""
import os
import re
import subprocess

import numpy as np
import pytest

from slimfastq_amd import capi
import util
from test_frozen_tables import SEG, base_chains_oracle, check_against_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SFQ_E_GENCHAR = -8            # include/slimfastq_amd.h

CODE = np.zeros(256, np.uint8)
for _ch, _v in zip("ACGTacgt0123", [0, 1, 2, 3] * 3):
    CODE[ord(_ch)] = _v


def fastq(seqs, rng, solid=False):
    out = []
    for i, s in enumerate(seqs):
        q = "".join(chr(int(v)) for v in rng.integers(35, 74, len(s) + (1 if solid else 0)))
        out.append("@g%d\n%s%s\n+\n%s\n" % (i, "T" if solid else "", s, q))
    return "".join(out).encode()


def random_bases(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


def packed(fq, br, cr, solid=0):
    """The base stream and the chains' sizes, in numpy"""
    starts, lens = util.line_table(fq)
    goff, glen = starts[1::4] + solid, lens[1::4] - solid
    a = np.frombuffer(fq, np.uint8)
    want = bytearray(); sizes = []
    nrec = len(goff)
    for b0 in range(0, nrec, br):
        for r0 in range(b0, min(b0 + br, nrec), cr):
            r1 = min(r0 + cr, b0 + br, nrec)
            c = np.concatenate([CODE[a[int(goff[r]): int(goff[r]) + int(glen[r])]] for r in range(r0, r1)] + [np.zeros(0, np.uint8)])
            c = np.concatenate([c, np.zeros(-len(c) % 4, np.uint8)]).reshape(-1, 4)
            by = (c[:, 0] | c[:, 1] << 2 | c[:, 2] << 4 | c[:, 3] << 6).astype(np.uint8)
            want += by.tobytes(); sizes.append(len(by))
    return bytes(want), sizes


def check_pack(ctx, fq, br, cr, oracle=True, solid=0):
    if oracle:
        enc = check_against_oracle(ctx, fq, 3, br=br, cr=cr, step=1, what="packed bases, %d / %d" % (br, cr))
    else:
        enc = ctx.encode_host(fq, level=3, block_reads=br, prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=cr)
    ci = util.unpack_chains(enc.chains)
    assert ci["flags"] & 128 and not ci["flags"] & (1 | 32 | 64)
    want, sizes = packed(fq, br, min(cr, br), solid)
    assert list(ci["gen"]) == sizes
    assert enc.stream("gen") == want
    assert ctx.decode_host(enc, level=3, out_cap=2 * len(fq) + 4096) == fq
    return enc


@pytest.mark.gpu
@pytest.mark.parametrize("br,cr", ((600, 1), (600, 7), (600, 64), (600, 65), (1000, 200)))
def test_short_lines_and_lines_around_dword_multiples(ctx, br, cr):
    rng = np.random.default_rng(br + cr)
    lens = list(range(1, 41)) + [63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 16, 15, 17, 31, 32, 33]
    seqs = [random_bases(rng, lens[i % len(lens)]) for i in range(1200)]
    check_pack(ctx, fastq(seqs, rng), br, cr)


@pytest.mark.gpu
@pytest.mark.parametrize("cr", (1, 5, 64, 100))
def test_n_and_lowercase_at_every_position_of_a_dword(ctx, cr):
    rng = np.random.default_rng(cr)
    seqs = []
    for i in range(2000):
        ln = 20 + (i * 7) % 150
        s = list(random_bases(rng, ln))
        p = (i % 16) + 16 * ((i // 16) % max(1, ln // 16))
        if p < ln:
            s[p] = "Nnacgt"[(i // 5) % 6]
        if i % 23 == 0:
            s[: ln // 3] = [ch.lower() for ch in s[: ln // 3]]
        seqs.append("".join(s))
    check_pack(ctx, fastq(seqs, rng), 500, cr)


@pytest.mark.gpu
def test_dots_as_the_n_byte(ctx):
    rng = np.random.default_rng(3)
    seqs = []
    for i in range(800):
        s = list(random_bases(rng, 60 + i % 50))
        s[i % 16] = "."
        seqs.append("".join(s))
    check_pack(ctx, fastq(seqs, rng), 400, 9)


@pytest.mark.gpu
def test_colour_space(ctx):
    rng = np.random.default_rng(5)
    seqs = ["".join(np.array(list("0123"))[rng.integers(0, 4, 40 + i % 90)]) for i in range(1500)]
    for i in range(0, len(seqs), 13):
        s = list(seqs[i]); s[i % len(s)] = "."; seqs[i] = "".join(s)
    fq = fastq(seqs, rng, solid=True)
    enc = check_pack(ctx, fq, 300, 11, oracle=False, solid=1)
    assert enc.blocks[0].solid == 1
    # the oracle's bases as well
    starts, lens = util.line_table(fq)
    ci = util.unpack_chains(enc.chains)
    want, sizes, on = base_chains_oracle(fq, starts[1::4] + 1, lens[1::4] - 1, ci, 300, 11)
    assert not on and enc.stream("gen") == want


@pytest.mark.gpu
@pytest.mark.parametrize("ln", (1, 13, 16, 150))
def test_last_line_of_the_text(ctx, ln):
    """The base line of the last record lies a few bytes before the text's end: a lane's sixteen-byte loads there must stay inside the text"""
    rng = np.random.default_rng(ln)
    seqs = [random_bases(rng, 100 + i % 17) for i in range(299)] + [random_bases(rng, ln)]
    fq = fastq(seqs, rng)
    check_pack(ctx, fq, 128, 10)


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(16))
def test_illegal_character_fails_the_block(ctx, j):
    rng = np.random.default_rng(j)
    seqs = [random_bases(rng, 150) for _ in range(200)]
    s = list(seqs[77]); s[32 + j] = "X"; seqs[77] = "".join(s)
    with pytest.raises(capi.SfqError) as e:
        ctx.encode_host(fastq(seqs, rng), level=3, block_reads=100, prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=1)
    assert e.value.code == SFQ_E_GENCHAR


@pytest.mark.gpu
@pytest.mark.parametrize("seg", (700, 1000))
def test_segments_of_long_reads(ctx, seg):
    rng = np.random.default_rng(seg)
    seqs = []
    for i in range(24):
        s = list(random_bases(rng, int(rng.integers(2500, 6000))))
        if i % 5 == 1:
            s[seg - 3: seg + 5] = "NNNNnnnn"
        if i % 7 == 2:
            s[100:140] = [ch.lower() for ch in s[100:140]]
        seqs.append("".join(s))
    fq = fastq(seqs, rng)
    br = 4
    enc = ctx.encode_host(fq, level=3, block_reads=br, prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=SEG | seg)
    starts, lens = util.line_table(fq)
    ci = util.unpack_chains(enc.chains, -(-len(seqs) // br))
    assert ci["flags"] & 8 and ci["flags"] & 128 and ci["seg_len"] == seg
    want, sizes, on = base_chains_oracle(fq, starts[1::4], lens[1::4], ci, br, 1, seg, lens[3::4])
    assert not on and list(ci["gen"]) == list(sizes) and enc.stream("gen") == want
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq


def test_pack_kernel_resources(tmp_path):
    """k_gen_pack_raw compiles for gfx950 without scratch, and within its register budget"""
    out = tmp_path / "chains.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-o", str(out), os.path.join(ROOT, "slimfastq_amd", "csrc", "chains.hip")], check=True, capture_output=True, timeout=900)
    found = False
    for blk in out.read_text().split("  - ."):
        name = re.search(r"\.name:\s+(\S+)", blk)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
        sc = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
        if name and vg and sc and "k_gen_pack_raw" in name.group(1):
            found = True
            assert int(sc.group(1)) == 0, "k_gen_pack_raw keeps scratch"
            assert int(vg.group(1)) <= 80, "k_gen_pack_raw needs %s VGPRs: fewer than 6 waves per SIMD" % vg.group(1)
    assert found

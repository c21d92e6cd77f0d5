"""k_gen_pack_raw (chains.hip) gives a record to a GROUP of lanes -- as many as the longest line among 64 records has pieces of sixteen bases:
4, 8, 16 for lines of up to 64, 128, 256 bases, the whole wavefront from 1009 on, a turn per 1024 bases above that -- and ORs each lane's
sixteen codes into a ring of 128 dwords in LDS (gen_pack_place.h).  test_gen_pack.py mixes all lengths in one text, which always picks the
widest group; the texts here keep to one class of widths at a time, put dozens of records into one dword, go round the ring many times, and
put the unusual characters where a group's first and last lanes meet them.  The expected bytes are test_gen_pack's numpy pack and the
oracle's (check_pack), with the way back."""
import numpy as np
import pytest

from slimfastq_amd import capi
import util
from test_frozen_tables import SEG, base_chains_oracle, check_against_oracle
from test_gen_pack import SFQ_E_GENCHAR, check_pack, fastq, packed, random_bases

WIDTHS = ((1, 64), (65, 128), (129, 256), (257, 1100))          # lines of up to 4, 8, 16 and 64 lanes a record (and, past 1024 bases, a second turn)


def class_lengths(rng, lo, hi, n):
    """n lengths of [lo, hi]: both edges, their neighbours, every residue mod 16, and random ones"""
    fixed = [lo, hi, lo + 1, hi - 1, hi, lo] + [lo + r for r in range(16)] + [hi - r for r in range(16)]
    return [fixed[i] if i < len(fixed) else int(rng.integers(lo, hi + 1)) for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("cr", (1, 7, 64, 65, 130))
@pytest.mark.parametrize("lo,hi", WIDTHS)
def test_one_group_width_at_a_time(ctx, lo, hi, cr):
    """chain_reads 1 .. 130: a chain of one step, of a partial last step, of exactly one chunk of 64 records, of a chunk and one record, of three chunks"""
    rng = np.random.default_rng(1000 * hi + cr)
    n = 1300 if hi <= 256 else 400
    seqs = [random_bases(rng, ln) for ln in class_lengths(rng, lo, hi, n)]
    check_pack(ctx, fastq(seqs, rng), 390, cr)


@pytest.mark.gpu
@pytest.mark.parametrize("cr", (7, 100))
@pytest.mark.parametrize("tiny", (1, 2, 3))
def test_many_records_in_one_dword(ctx, tiny, cr):
    """Runs of 40 and more lines of 1, 2 or 3 bases between normal lines: up to sixteen records OR into one dword and into the one behind it"""
    rng = np.random.default_rng(10 * tiny + cr)
    seqs = []
    for g in range(40):
        seqs.append(random_bases(rng, (150, 37, 64, 255, 16, 300)[g % 6] + g % 3))
        seqs += [random_bases(rng, tiny) for _ in range(40 + g % 9)]
    check_pack(ctx, fastq(seqs, rng), 500, cr)


@pytest.mark.gpu
@pytest.mark.parametrize("ln", (257, 150))
def test_chains_that_go_round_the_ring(ctx, ln):
    """200 records a chain: 51 400 (30 000) bases, 25 (14) times the ring's 2048"""
    rng = np.random.default_rng(ln)
    seqs = [random_bases(rng, ln) for _ in range(1000)]
    check_pack(ctx, fastq(seqs, rng), 400, 200)


@pytest.mark.gpu
@pytest.mark.parametrize("seg", (700, 1000))
def test_segments_that_start_anywhere(ctx, seg):
    """Segments of long reads: a chain is bases [sub_lo, sub_lo + sub_len) of one line, sub_lo no multiple of 16, 1024 bases a turn of the wavefront"""
    rng = np.random.default_rng(seg + 1)
    seqs = []
    for i in range(20):
        s = list(random_bases(rng, int(rng.integers(2500, 6000))))
        if i % 4 == 1:
            s[seg - 2: seg + 3] = "NNnNN"
            s[-1] = "N"
        if i % 5 == 2:
            s[1020:1030] = [ch.lower() for ch in s[1020:1030]]
        seqs.append("".join(s))
    fq = fastq(seqs, rng)
    br = 4
    enc = ctx.encode_host(fq, level=3, block_reads=br, prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=SEG | seg)
    starts, lens = util.line_table(fq)
    ci = util.unpack_chains(enc.chains, -(-len(seqs) // br))
    assert ci["flags"] & 8 and ci["flags"] & 128 and ci["seg_len"] == seg
    segs = [-(-int(m) // seg) for m in lens[1::4]]
    assert any((-(-int(m) // k)) % 16 for m, k in zip(lens[1::4], segs))          # (segment lengths that are no multiple of 16)
    want, sizes, on = base_chains_oracle(fq, starts[1::4], lens[1::4], ci, br, 1, seg, lens[3::4])
    assert not on and list(ci["gen"]) == list(sizes) and enc.stream("gen") == want
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq


@pytest.mark.gpu
@pytest.mark.parametrize("cr", (1, 40))
@pytest.mark.parametrize("ch", ("N", "g", "."))
def test_marks_in_the_first_and_the_last_piece(ctx, ch, cr):
    """An N, a lowercase base or a '.': at the first and the last base of a record, in the first and the last piece, in a record of one base, and
    in a record of five bases that shares its dwords with both neighbours.  The oracle's exception streams and the way back hold the marks
    (a record the pack did not mark would lose them)."""
    rng = np.random.default_rng(ord(ch) + cr)
    seqs = []
    for i in range(1200):
        ln = (150, 1, 5, 64, 65, 256, 257, 300, 17, 1030)[i % 10]
        s = list(random_bases(rng, ln))
        kind = (i // 10) % 6
        if kind == 0:
            s[0] = ch
        elif kind == 1:
            s[-1] = ch
        elif kind == 2:
            s[min(15, ln - 1)] = ch                       # the last base of the first piece
        elif kind == 3:
            s[(ln - 1) & ~15] = ch                        # the first base of the last piece
        elif kind == 4 and ln > 2:
            s[ln // 2] = ch
        seqs.append("".join(s))                           # (kind 5: clean records between the marked ones)
    check_pack(ctx, fastq(seqs, rng), 400, cr)


@pytest.mark.gpu
@pytest.mark.parametrize("j", range(16))
def test_illegal_character_in_a_last_partial_piece(ctx, j):
    """Byte j of a line's last piece, which ends there: the validity mask must keep it"""
    rng = np.random.default_rng(j)
    seqs = [random_bases(rng, 150) for _ in range(200)]
    seqs[77] = random_bases(rng, 144 + j) + "X"
    for cr in (1, 40):
        with pytest.raises(capi.SfqError) as e:
            ctx.encode_host(fastq(seqs, rng), level=3, block_reads=100, prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=cr)
        assert e.value.code == SFQ_E_GENCHAR


@pytest.mark.gpu
def test_bytes_behind_a_line_end_are_not_bases(ctx):
    """A lane's sixteen bytes reach past its line's end into '\\n', '+' and the quality line -- here all 'X', no base: none of it is an illegal
    base, whatever the line's length mod 16, and none of it is packed"""
    rng = np.random.default_rng(16)
    seqs = [random_bases(rng, 1 + i % 48) for i in range(960)] + [random_bases(rng, 130 + i % 16) for i in range(320)]
    fq = "".join("@g%d\n%s\n+\n%s\n" % (i, s, "X" * len(s)) for i, s in enumerate(seqs)).encode()
    for cr in (1, 40):
        check_pack(ctx, fq, 320, cr)


@pytest.mark.gpu
@pytest.mark.parametrize("ln", (1, 13, 16))
def test_text_at_an_odd_device_offset(ctx, ln):
    """The text placed 13 bytes behind a 16-byte boundary between guards of FASTQ-like bytes, its last base line ln bases long: the loads
    of the last record's lanes end with the text"""
    rng = np.random.default_rng(40 + ln)
    seqs = [random_bases(rng, 100 + i % 60) for i in range(599)] + [random_bases(rng, ln)]
    fq = fastq(seqs, rng)
    src = util.Placed(len(fq), 13, "fastq", fq)
    cap = capi.lib().sfq_encode_bound(len(fq))
    dst = util.Placed(cap, 8, "fastq")
    res = ctx.encode_device(src.ptr, len(fq), dst.ptr, cap, level=3, block_reads=128, prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=10)
    assert dst.guards_intact() and src.back("the input") == fq
    enc = ctx._encoded(res, np.frombuffer(dst.head(res.total_bytes), np.uint8))
    check_against_oracle(ctx, fq, 3, br=128, cr=10, step=1, what="placed text", enc=enc)
    want, sizes = packed(fq, 128, 10)
    assert list(util.unpack_chains(enc.chains)["gen"]) == sizes and enc.stream("gen") == want
    assert ctx.decode_host(enc, level=3, out_cap=2 * len(fq) + 4096) == fq

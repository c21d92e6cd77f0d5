"""A window of pairs from an archive of paired files (sfq_decode_pair_range_host): the blocks that hold the pairs
are decoded, cut to the records and split on the device; every window against the slices of the two original files.  Blocks of
seven records begin at second mates.  sfq_pair_window_blocks alone needs no GPU."""
import numpy as np
import pytest

from test_pairs import E_ARG, E_CORRUPT, E_FORMAT, interleaved, reads, records
from slimfastq_amd import capi

gpu = pytest.mark.gpu
PAIRS, BLOCK = 3000, 7
CASES = {
    "adaptive": dict(level=3, block_reads=BLOCK, tables=capi.TABLES_ADAPTIVE),
    "frozen": dict(level=3, block_reads=BLOCK, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN, chain_reads=16),
}
# (first pair, pairs): the first, all, records 8 and 9 = the second and third of block 1, records 6 and 7 = the last of block 0 and the
# first of block 1, a hundred pairs over 29 blocks, the last
WINDOWS = ((0, 1), (0, PAIRS), (4, 1), (3, 1), (1000, 100), (PAIRS - 1, 1))
_files = None


def files():
    global _files
    if _files is None:
        a, b = reads(PAIRS, 30, 60, seed=21), reads(PAIRS, 30, 60, seed=22)
        _files = (a, b, records(a), records(b))
    return _files


@pytest.fixture(scope="module", params=sorted(CASES))
def archive(request, ctx):
    """(the archive with its blocks' CRCs, the case's name)"""
    a, b, _, _ = files()
    ctx.set_checksums(True)
    try:
        enc = ctx.encode_pairs_host(a, b, **CASES[request.param])
    finally:
        ctx.set_checksums(False)
    assert len(enc.blocks) == (2 * PAIRS + BLOCK - 1) // BLOCK and len(enc.crcs) == len(enc.blocks)
    if request.param == "frozen":
        assert len(enc.chains) > 0
    return enc


def blocks_of(first_pair, n):
    return 2 * first_pair // BLOCK, (2 * (first_pair + n) - 1) // BLOCK - 2 * first_pair // BLOCK + 1


@gpu
@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "%d_%d" % w)
def test_windows(ctx, archive, window):
    _, _, ra, rb = files()
    p0, n = window
    assert capi.pair_window_blocks(archive.blocks, p0, n) == blocks_of(p0, n)
    cap = len(interleaved(b"".join(ra[p0:p0 + n]), b"".join(rb[p0:p0 + n]))) + 4096 + 2 * BLOCK * 200
    for split_switch in (False, True):                                # it works whatever the switch says
        ctx.set_pair_split(split_switch)
        try:
            first, second, res = ctx.decode_pair_range_host(archive, p0, n, out_cap=cap)      # (installs the window's blocks' CRCs)
        finally:
            ctx.set_pair_split(False)
        assert first == b"".join(ra[p0:p0 + n]) and second == b"".join(rb[p0:p0 + n])
        assert ctx.pair_split() == (len(first), n)
        assert res.n_blocks == blocks_of(p0, n)[1]
    first, second, _ = ctx.decode_pair_range_host(archive, p0, n, out_cap=cap, crcs=())       # and without checksums: () installs none
    assert first == b"".join(ra[p0:p0 + n]) and second == b"".join(rb[p0:p0 + n])


@gpu
def test_a_flipped_checksum_is_corrupt(ctx, archive):
    b0, nb = blocks_of(1000, 100)
    crcs = list(archive.crcs[b0:b0 + nb])
    crcs[nb // 2] ^= 1
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_pair_range_host(archive, 1000, 100, crcs=crcs)
    assert e.value.code == E_CORRUPT and ctx.pair_split() is None
    with pytest.raises(capi.SfqError) as e:                           # the CRCs of other blocks than the window's
        ctx.decode_pair_range_host(archive, 1000, 100, crcs=archive.crcs[b0 + 1:b0 + 1 + nb])
    assert e.value.code == E_CORRUPT


@gpu
def test_argument_errors(ctx, archive):
    for p0, n in ((0, 0), (5, 0), (PAIRS, 1), (PAIRS - 1, 2), (0, PAIRS + 1), (1 << 62, 1), (1 << 63, 1 << 63)):
        with pytest.raises(capi.SfqError) as e:
            ctx.decode_pair_range_host(archive, p0, n)
        assert e.value.code == E_ARG, (p0, n)
    _, _, ra, rb = files()
    first, second, _ = ctx.decode_pair_range_host(archive, 10, 2)
    assert (first, second) == (b"".join(ra[10:12]), b"".join(rb[10:12]))


@gpu
def test_an_archive_of_an_odd_record_count(ctx):
    enc = ctx.encode_host(reads(2001, 30, 60, seed=23), **CASES["adaptive"])
    with pytest.raises(capi.SfqError) as e:
        ctx.decode_pair_range_host(enc, 0, 1)
    assert e.value.code == E_FORMAT


def test_pair_window_blocks_against_a_search():
    """a hand-made index, blocks of unequal n_records: the blocks of a window are those that hold one of its records"""
    counts = (7, 7, 3, 10, 1, 4, 2)
    assert sum(counts) % 2 == 0
    blocks = (capi.BlockInfo * len(counts))()
    owner = []
    for i, c in enumerate(counts):
        blocks[i].first_record, blocks[i].n_records = len(owner), c
        owner += [i] * c
    pairs = len(owner) // 2
    for p0 in range(pairs + 2):
        for n in range(pairs + 3):
            got = capi.pair_window_blocks(blocks, p0, n)
            if n == 0 or p0 + n > pairs:
                assert got is None, (p0, n)
            else:
                held = sorted(set(owner[2 * p0:2 * (p0 + n)]))
                assert held == list(range(held[0], held[-1] + 1))
                assert got == (held[0], len(held)), (p0, n)
    assert capi.pair_window_blocks(blocks, 1 << 63, 1 << 63) is None and capi.pair_window_blocks(blocks, (1 << 64) - 1, 1) is None

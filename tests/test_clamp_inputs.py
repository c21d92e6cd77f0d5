"""The texts of clamp_mint.py (inputs for GPU cases that push every copy of the range coder through its interval clamp), qualified on the CPU:
each is legal FASTQ, the oracle codes it and reads it back, and the stream a GPU case is to compare takes the clamp (coder.hpp:76-77) at
least MIN_CLAMPS times on the way out and as often on the way back -- a condition, so that no GPU case passes without having run the line -- while the ordinary text it was made from takes it never.
Also what the corpus itself gives: edge_hdr's header stream clamps at every level, the only clamp any fixture reaches."""
import numpy as np
import pytest

import clamp_mint as M
import util
from oracle import oracle as O
from slimfastq_amd import capi


def test_the_counter_counts_every_coder_of_the_oracle_and_resets():
    O.rc_clamps(True)
    fq = capi.synth_fastq(300, 150, seed=3)
    O.compress(fq, 3)
    assert O.rc_clamps(False) == 0 and O.rc_clamps(True) == 0
    t = M.adaptive(*M.FORMAT6[1])
    a = O.compress(t["fq"], 1)
    n = O.rc_clamps(False)
    assert n >= 2 * M.MIN_CLAMPS and O.rc_clamps(True) == n and O.rc_clamps(True) == 0
    assert O.decompress(a.image) == t["fq"] and 2 * M.MIN_CLAMPS <= O.rc_clamps(True) <= n          # RCoder's decoder
    t = M.frozen_qlt(*M.FROZEN_QLT["all-lanes-level1"])
    (s, sizes, _), ne = M.clamps_of(M.frozen_qlt_streams, t)                              # the chains' encoder and decoder
    _, nd = M.clamps_of(M.frozen_qlt_back, t, s, sizes)
    assert ne >= M.MIN_CLAMPS and nd == ne


def test_quality_chains_decode_back_on_ordinary_text():
    """O.qlt_decode_chains / _segs are O.qlt_encode_chains / _segs' mirrors (escapes included)."""
    fq = util.golden_fastq("edge_hiq") + capi.synth_fastq(500, 150, seed=12)
    starts, lens = util.line_table(fq)
    qoff, qlen, glen = starts[3::4], lens[3::4], lens[1::4]
    for level in (1, 2, 3):
        frozen = O.qlt_frozen_rows(O.qlt_prior_rows(O.qlt_histogram(fq, qoff, qlen, level, 0, 3)))
        s, sizes, extra = O.qlt_encode_chains(fq, qoff, qlen, level, 100, 7, frozen)
        assert M.with_lines(fq, 3, O.qlt_decode_chains(s, sizes, qoff, qlen, level, 100, 7, frozen)) == fq
        s, sizes, _ = O.qlt_encode_segs(fq, qoff, qlen, glen, level, 64, frozen)
        assert M.with_lines(fq, 3, O.qlt_decode_segs(s, sizes, qoff, qlen, glen, level, 64, frozen)) == fq
    assert extra > 0


def test_generation_table_chains_decode_back():
    fq = M.folded_genome_reads(6000, 61)
    starts, lens = util.line_table(fq)
    s, sizes, on = O.gen_encode_chains(fq, starts[1::4], lens[1::4], 16, 32, 8, M.GEN_STEP)
    assert on == 1
    assert M.with_lines(fq, 1, O.gen_decode_chains(s, sizes, starts[1::4], lens[1::4], 16, 32, 8, M.GEN_STEP, 1)) == fq


def test_a_text_is_a_function_of_its_arguments():
    """Every minting function once more, uncached: the same text."""
    for fn, args in ((M.frozen_qlt, M.FROZEN_QLT["lane31"]), (M.frozen_qlt, M.FROZEN_QLT["segments"]), (M.adaptive, M.FORMAT6[1]),
                     (M.adaptive, M.BLOCKS["cold-level1"][0]), (M.frozen_bases, M.FROZEN_BASES["tables"]), (M.frozen_bases, M.FROZEN_BASES["gm"])):
        assert fn(*args) is fn(*args) and fn.__wrapped__(*args)["fq"] == fn(*args)["fq"]


@pytest.mark.parametrize("name", sorted(M.FROZEN_QLT))
def test_frozen_quality_texts(name):
    t = M.frozen_qlt(*M.FROZEN_QLT[name])
    assert M.is_legal(t["fq"]) and util.line_table(t["fq"])[1].tolist() == util.line_table(t["plain"])[1].tolist()
    assert np.array_equal(util.unpack_prior(t["prior"], M.q_rows(t["level"])), t["rows66"])
    (s, sizes, extra), ne = M.clamps_of(M.frozen_qlt_streams, t)
    back, nd = M.clamps_of(M.frozen_qlt_back, t, s, sizes)
    print(name, "clamps", ne)
    assert back == t["fq"] and extra == 0
    assert ne >= M.MIN_CLAMPS and nd == ne
    assert M.clamps_of(M.frozen_qlt_streams, t, t["plain"])[1] == 0
    assert np.array_equal(util.unpack_rec_prior(t["rec_prior"]), t["rec_f"])          # (the header prior the encoder is given beside it)


def _adaptive_checks(t, qlt=True):
    fq = t["fq"]
    assert M.is_legal(fq)
    starts, lens = util.line_table(fq)
    counts = {}
    if qlt:
        (s, sizes), ne = M.clamps_of(M.adaptive_qlt_streams, t)
        # back: the steered decoder on streams an encoder wrote never has to steer (chain framing: without the four leading zero bytes)
        parts, at = [], 0
        for n in sizes:
            assert s[at:at + 4] == b"\0\0\0\0"
            parts.append(s[at + 4:at + int(n)]); at += int(n)
        back, nd = M.clamps_of(O.qlt_steer_blocks, b"".join(parts), [len(p) for p in parts], starts[3::4], lens[3::4], t["level"], t["per"],
                               tuple(range(63)), t["rows66"])
        assert M.with_lines(fq, 3, back) == fq
        assert ne >= M.MIN_CLAMPS and nd == ne
        assert M.clamps_of(M.adaptive_qlt_streams, t, t["plain"])[1] == 0
        counts["qlt"] = ne
    g, ne = M.clamps_of(M.adaptive_gen_streams, t)
    assert all(p[:4] == b"\0\0\0\0" for p in g)
    back, nd = M.clamps_of(O.gen_steer_blocks, b"".join(p[4:] for p in g), [len(p) - 4 for p in g], starts[1::4], lens[1::4], t["gen_bits"], t["per"])
    assert M.with_lines(fq, 1, back) == fq
    assert ne >= M.MIN_CLAMPS and nd == ne
    assert M.clamps_of(M.adaptive_gen_streams, t, t["plain"])[1] == 0
    counts["gen"] = ne
    print(counts)


@pytest.mark.parametrize("level", sorted(M.FORMAT6))
def test_format_6_texts(level):
    t = M.adaptive(*M.FORMAT6[level])
    _adaptive_checks(t)
    a = O.compress(t["fq"], level)                                              # the whole file through the reference's own path, and back
    assert a.streams["qlt"] == M.adaptive_qlt_streams(t)[0] and a.streams["gen"] == M.adaptive_gen_streams(t)[0]
    assert O.decompress(a.image) == t["fq"]


@pytest.mark.parametrize("name", sorted(M.BLOCKS))
def test_adaptive_block_texts(name):
    args, step = M.BLOCKS[name]
    t = M.adaptive(*args)
    _adaptive_checks(t, qlt=name != "counted-prior")
    if t["rows66"] is not None:
        assert np.array_equal(util.unpack_prior(t["prior"], M.q_rows(t["level"])), t["rows66"])


@pytest.mark.parametrize("name", sorted(M.FROZEN_BASES))
def test_frozen_base_texts(name):
    t = M.frozen_bases(*M.FROZEN_BASES[name])
    fq = t["fq"]
    assert M.is_legal(fq)
    starts, lens = util.line_table(fq)
    (s, sizes, on), ne = M.clamps_of(M.frozen_bases_streams, t)
    assert on == 1
    if name == "gm":
        codes, nd = M.clamps_of(O.gm_decode_chains, s, sizes, lens[1::4], t["tb"], t["br"], t["cr"])
        back = np.frombuffer(b"ACGT", np.uint8)[codes].tobytes()
        assert back == b"".join(r[1] for r in M.records(fq))
    else:
        back, nd = M.clamps_of(O.gen_decode_chains, s, sizes, starts[1::4], lens[1::4], t["gen_bits"], t["br"], t["cr"], M.GEN_STEP, 1)
        assert M.with_lines(fq, 1, back) == fq
    print(name, "clamps", ne)
    assert ne >= M.MIN_CLAMPS and nd == ne
    # every clamp lies in the minted chains; the ordinary text takes none
    (s0, sizes0, on0), n0 = M.clamps_of(M.frozen_bases_streams, t, t["plain"])
    assert on0 == 1 and n0 == 0
    at = int(np.asarray(sizes[:t["first"]]).sum())
    assert s[:at] == s0[:at]


def test_the_corpus_reaches_the_clamp_only_in_edge_hdrs_headers():
    """What the fixtures give without minting: edge_hdr's "rec" stream takes the clamp at every level (the format-6 header coder's only
    coverage); its quality and base streams take it never."""
    fq = util.golden_fastq("edge_hdr")
    starts, lens = util.line_table(fq)
    for level in (1, 2, 3, 4):
        assert M.clamps_of(O.compress, fq, level)[1] >= 1
    assert M.clamps_of(O.rec_encode, fq, starts[0::4] + 1, lens[0::4] - 1)[1] >= 1
    assert M.clamps_of(O.qlt_encode, fq, starts[3::4], lens[3::4], 3)[1] == 0
    assert M.clamps_of(O.gen_encode, fq, starts[1::4], lens[1::4], starts[3::4], lens[3::4], 24)[1] == 0

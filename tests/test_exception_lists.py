"""The base-exception lists of every block against a Python statement of the code (exc_mint.py: positions, rice_encode), on texts minted for
the edges of dev_rice.h, k_gen_exc_q (models_w.hip) and k_gen_exc_decode_r (exc.hip).  Frozen tables, level 3, through encode_host / decode_host.

Cases (19; the module takes 2.4 s on one MI355X, its slowest case -- far-25, 71 MB of text -- 0.3 s):
  8  edges, queue, queue-dot, queue-colour at two geometries each (the second: blocks of no multiple of 64, chains that do not divide them): every
     block's gen.Ns / gen.Nn / gen.lc equal rice_encode(gaps of positions(block)), the block's N byte is the rule's, chn.idx flag bit 4, decode == text
  2  ragged-flat, ragged-match: the same, the stage asserted from chn.idx, decoded into the packed and the padded capacity
  2  far-20, far-25: the lists and the round trip only
  2  check_against_oracle on edges and queue: the new texts tied to everything else a call writes
  2  kernel = 2 on edges and queue: the reference's own coding of the same gaps, every block against the reference run on it
  1  a window of queue's blocks that does not start at block 0
  2  damaged lists (ones instead of a list; no end mark): what the Python decoder says first, then SfqError

Mutation checks (scratch builds, one change each, values and comparisons only; the new module and test_frozen_tables.py run against each; "older":
test_frozen_tables.py, before AND after its comparison was widened to every block -- the two noticed the same mutants):
  dev_rice.h  q <= RICE_ESC, encoder only           edges (both geometries), its oracle case, both damaged-list cases      older: the exception-scan cases
              q <= RICE_ESC, encoder and decoder    15 cases: every text's lists, both far cases                           older: 15 cases (the round trip breaks)
              upper field & 0xFFFF                  NOT caught, and cannot be: it loses bits of gaps of 2^36 and more, and a block has fewer bases
              upper field & 0x1F (instead)          far-25 gen.Ns, one byte                                                older: passes
              N > 32, both                          edges, all queue texts, both oracle cases, the missing end             older: 16 cases (against the oracle's C)
              RICE_KMAX 23, both                    far-25 alone                                                           older: passes
  k_gen_exc_q ninth event dropped                   13 cases: edges (a record of nine), all queue texts, the window        older: 10 cases
              llen >= EXQ_MAXLEN                    nothing, as it should: 1024 bases through the wave's walk give the same lists
              fl without the bases' mask            all queue texts, queue's oracle case, the window                       older: passes
              quality behind a short line '!'       all queue texts, queue's oracle case, the window                       older: 7 cases
  k_gen_exc_decode_r
              rec_of only steps down                all queue texts, both ragged texts, the window                         older: 9 cases
              no `k >= nr` clamp                    nothing: (at - 1) * nr / nb is below nr for every at <= nb, and `at > nb` is refused before the look-up
Only the Python rule notices a fault that coder and decoder share and the oracle's C shares too; of the faults above the oracle's C shares none, so
what the new texts add is reach: the clamp, the escape's upper field and the '!' behind the bases are met by no older text.
"""
import time

import numpy as np
import pytest

import exc_mint as M
import util
from slimfastq_amd import capi
from test_frozen_tables import check_against_oracle

pytestmark = pytest.mark.gpu
_ENC = {}


def _encode(ctx, name, br, cr, kernel=0):
    key = (name, br, cr, kernel)
    if key not in _ENC:
        _ENC[key] = ctx.encode_host(M.text(name)["fq"], level=3, block_reads=br, prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=cr, kernel=kernel)
    return _ENC[key]


def _lists_are_the_rules(enc, name, br):
    """every block's three streams bit for bit, and its N byte"""
    want = M.lists(name, br)
    assert len(enc.blocks) == len(want)
    assert util.unpack_chains(enc.chains)["flags"] & 16
    for b, (lists, n_byte, _) in enumerate(want):
        for ln in M.NAMES:
            util.first_difference(enc.stream(ln, b), lists[ln][0], "%s, blocks of %d: block %d %s" % (name, br, b, ln))
        assert enc.blocks[b].n_byte == n_byte, (name, br, b)
        assert enc.blocks[b].solid == M.text(name)["solid"]


def _geos(names):
    return [(n, br, cr) for n in names for br, cr in M.text(n)["geos"]]


@pytest.mark.parametrize("name,br,cr", _geos(("edges",) + M.QUEUES))
def test_lists_of_every_block_at_the_codes_and_the_queues_edges(ctx, name, br, cr):
    fq = M.text(name)["fq"]
    enc = _encode(ctx, name, br, cr)
    _lists_are_the_rules(enc, name, br)
    assert br % 64 != 0 and br % cr != 0 or (br, cr) == M.text(name)["geos"][0]
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq


@pytest.mark.parametrize("name", ("ragged-flat", "ragged-match"))
def test_lists_of_ragged_blocks_in_either_stage(ctx, name):
    """k_gen_exc_decode_r's rec_of looks a position's record up wherever the staged lines are not back to back: the match model's stage (a sentinel
    behind every line) and the flat bases' stage of lines on 32-byte sectors, which a call takes where the output has 128 bytes a record or more.
    The flat text is decoded into both capacities: the packed stage (no look-up) and the padded one."""
    t = M.text(name)
    fq, (br, cr) = t["fq"], t["geos"][0]
    enc = _encode(ctx, name, br, cr)
    _lists_are_the_rules(enc, name, br)
    flags = util.unpack_chains(enc.chains)["flags"]
    assert not flags & 8                                      # whole records, no segments
    if t["claims"]["match"]:
        assert flags & 32
    else:
        assert flags & 192 == 128 and not flags & (1 | 32)
    assert (len(fq) + 4096) // t["nrec"] < 128
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 128 * t["nrec"]) == fq


@pytest.mark.parametrize("name", ("far-20", "far-25"))
def test_lists_with_gaps_of_two_to_the_twenty_and_more(ctx, name):
    """far-20: the escape's upper field 0, 1 and 2.  far-25: gaps behind an event 2^25 bases in, coded with the clamped k = 24.
    Measured on one MI355X: far-20 (8.6 MB) encode_host 0.01 s, decode_host 0.02 s; far-25 (71 MB) encode_host 0.04 s, the comparison 0.10 s,
    decode_host 0.03 s; minting far-25 and stating its lists in numpy, 0.7 s on the host, is done once and shared with test_exception_inputs.py."""
    t = M.text(name)
    fq, (br, cr) = t["fq"], t["geos"][0]
    t0 = time.perf_counter()
    enc = ctx.encode_host(fq, level=3, block_reads=br, prior_step=1, tables=capi.TABLES_FROZEN, chain_reads=cr)
    t1 = time.perf_counter()
    _lists_are_the_rules(enc, name, br)
    t2 = time.perf_counter()
    back = ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096)
    t3 = time.perf_counter()
    print("%s: encode_host %.2f s, lists %.2f s, decode_host %.2f s" % (name, t1 - t0, t2 - t1, t3 - t2))
    assert back == fq


@pytest.mark.parametrize("name", ("edges", "queue"))
def test_the_whole_call_against_the_oracle(ctx, name):
    t = M.text(name)
    br, cr = t["geos"][0]
    check_against_oracle(ctx, t["fq"], 3, br=br, cr=cr, step=1, what=name, enc=_encode(ctx, name, br, cr))


@pytest.mark.parametrize("name", ("edges", "queue"))
def test_the_references_own_coding_of_the_same_gaps(ctx, name):
    """kernel = 2: the gaps through the reference's XFile coding (k_gen_exc_w<false>, k_gen_exc_decode_w), gaps of two and more bytes among them:
    every block's three streams are the reference's on a file holding the block, and the archive decodes."""
    t = M.text(name)
    fq, (br, cr) = t["fq"], t["geos"][0]
    old = _encode(ctx, name, br, cr, kernel=2)
    assert not util.unpack_chains(old.chains)["flags"] & 16
    big = 0
    for b, chunk in enumerate(M.block_chunks(t, br)):
        ref = util.block_reference(chunk, 3, gen_bits=old.blocks[b].gen_bits).streams
        for ln in M.NAMES:
            util.first_difference(old.stream(ln, b), ref.get(ln, b""), "%s block %d %s" % (name, b, ln))
        big += any(v >= 256 for ln in M.NAMES for v, _, _ in M.lists(name, br)[b][0][ln][1]["steps"])
    assert big >= 3
    assert ctx.decode_host(old, level=3, out_cap=len(fq) + 4096) == fq


def test_a_window_of_queue_blocks(ctx):
    """launch_gen_exc_decode_r takes the blocks [b0, b1): a window that does not start with block 0"""
    t = M.text("queue")
    br, cr = t["geos"][0]
    enc = _encode(ctx, "queue", br, cr)
    chunks = M.block_chunks(t, br)
    for b0, n in ((3, 5), (9, 2), (10, 1)):
        got, _ = ctx.decode_range_host(enc, b0, n, level=3, out_cap=len(t["fq"]) + 4096)
        assert got == b"".join(chunks[b0:b0 + n]), (b0, n)


def _place(enc, ln, b):
    s = capi.STREAM_NAMES.index(ln)
    return int(enc.res.stream_offset[s]) + sum(int(enc.blocks[i].size[s]) for i in range(b))


def test_a_list_overwritten_with_ones_is_refused(ctx):
    """A block's gen.Ns as 0xFF bytes: an escape to a position of 2^40 - 1, far behind the block's bases (exc.hip: at > nb)."""
    t = M.text("edges")
    fq, (br, cr) = t["fq"], t["geos"][0]
    enc = _encode(ctx, "edges", br, cr)
    b = t["claims"]["same list as Ns"][0]
    n = len(enc.stream("gen.Ns", b))
    assert n >= 9 and M.verdict(b"\xff" * n, M.lists("edges", br)[b][2]) == "position beyond the block"
    bad = enc.clone()
    at = _place(bad, "gen.Ns", b)
    bad.data[at:at + n] = 0xFF
    assert bad.stream("gen.Ns", b) == b"\xff" * n and len(bad.data) == len(enc.data)
    with pytest.raises(capi.SfqError):
        ctx.decode_host(bad, level=3, out_cap=len(fq) + 4096)
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq


def test_a_list_without_its_end_is_refused(ctx):
    """The end mark's zero bits and the padding of the list's last byte set to ones: the list has no end inside its stream (RiceR reads zeros
    behind the stream, and says so)."""
    t = M.text("edges")
    fq, (br, cr) = t["fq"], t["geos"][0]
    enc = _encode(ctx, "edges", br, cr)
    L = M.lists("edges", br)
    found = None
    for b, (lists, _, nb) in enumerate(L):
        for ln in M.NAMES:
            blob, rep = lists[ln]
            if blob and found is None:
                v = int.from_bytes(blob, "little") | (((1 << (8 * len(blob) - rep["bits"])) - 1) << rep["bits"])
                v = v.to_bytes(len(blob), "little")
                if M.verdict(v, nb) == "end outside the stream":
                    found = (b, ln, v)
    assert found is not None
    b, ln, v = found
    assert enc.stream(ln, b) == L[b][0][ln][0]
    bad = enc.clone()
    at = _place(bad, ln, b)
    bad.data[at:at + len(v)] = np.frombuffer(v, np.uint8)
    assert bad.stream(ln, b) == v
    with pytest.raises(capi.SfqError):
        ctx.decode_host(bad, level=3, out_cap=len(fq) + 4096)
    assert ctx.decode_host(enc, level=3, out_cap=len(fq) + 4096) == fq

"""The decoder's last step -- launch_assemble (csrc/decode_l.hip) lays headers, bases and qualities out as FASTQ text in the caller's buffer --
at the record counts that pick each of its kernels, on hostile records, and at the edges of the caller's buffer.

launch_assemble takes rpw = clamp(nrec / 32768, 1, 64) records a wave (rpw_of below is this module's own statement of the rule) and runs k_assemble
for rpw < 4, k_assemble4 (sixteen lanes a record, sixteen bytes a lane) from 131 072 records up.  Which kernel a test reaches follows from its record
count through rpw_of, asserted in the test; which staging the decode took is read from the chain index ("chn.idx" flags, util.unpack_chains): bit 5 =
the match model (gm.hip: base lines staged with a sentinel behind each), bits 7 and 4 = flat two-bit bases with Rice-coded exception lists (the
staging `spad` belongs to, api.cpp).  Both are asserted where they are claimed.

hostile_fastq(nrec, seed, ...) is a vectorised generator (numpy, chunks of 65 536 records): header, base and quality lines of 1..15 bytes in every
value and of every residue mod 16 above that, a few headers over 256 bytes and base lines of 300..1100, quality lines as long as, shorter than (by
1..40) and longer than (by 1..20: the oracle takes it) their base lines, N under '!' and under other qualities, '!' over real bases, lowercase bases
single, in runs and under '!', 'n' -- at every offset of a sixteen-byte piece, inside the overlapping end piece, in lines under sixteen bytes and
behind the quality line's end; per text: a second id on every '+' line, colour space (primer, 0123, '.'), '.' as the N byte in base space, bases
drawn from a small pool (the match model switches on) or iid (flat two-bit bases).

  test_hostile_text_covers_every_class_and_the_oracle_takes_it   CPU.  The classes above occur in the texts the GPU tests use (5 003 records, every
      switch set; 200 000 records), at least a stated number of times each; records average under 128 bytes; every switch set passes the oracle both
      ways at 3 000 records (block format: util.block_reference, a block a time; format 6: O.compress / O.decompress -- it refuses 'n' beside 'N', so
      format 6 runs with n_byte = '.').  No switch set had to be dropped.
  test_assembly_at_every_records_per_wave   rpw = 1 (5 003 records), 3 (131 071: the last count of k_assemble), 4 (131 073, nrec % 4 = 1), 6
      (196 613: cnt % 4 = 2, two groups of lanes sit out a wave's last round), 7 (229 379), 64 (2 097 189, nrec % 64 = 37): k_assemble for the first
      two, k_assemble4 for the rest (asserted through rpw_of).  Frozen and adaptive tables.  All twelve switch sets at rpw = 1 and rpw = 4, the four of
      THIN (every switch on once and off once, both kinds of bases) at rpw = 3, 6, 7, two at rpw = 64 (frozen: second id, 'N', iid bases; adaptive: colour
      space, '.', pooled bases).  decode == input with the exact capacity and -- frozen tables up to rpw = 7 -- again with 128 bytes a record (the padded
      stages).  Staging: frozen + pooled bases -> flags & 32; frozen + iid bases -> flags & 192 == 128 and flags & 16 (asserted).
      The encoder's bytes: adaptive -> all streams of the first, the last and 16 seeded blocks equal util.block_reference; frozen -> check_against_oracle
      (everything) at rpw = 1 for every switch set and at rpw = 3 and 4 for the first two of THIN (flat and match model); above that, where the bases are
      iid and the text in base space, sampled chains as test_gpu_parity._check_sampled_chains_against_oracle; else the round trip and the smaller counts.
  test_format_6_at_four_records_a_wave   format 6 (one block) at 131 073 records, and the same text with two records over 65 534 bases spliced in
      (n_over = 2: k_assemble4 writes through oroff_k beside launch_over_place; 131 073 kept records, so still rpw = 4): streams == O.compress(..).streams,
      text == the oracle's decode, decoder kernels 0 and 1.
  test_exact_capacity_and_guards   sfq_decode_blocks into the middle of one 0xA5-filled tensor, 64 KiB of guard on either side, out_cap == the text's
      size: 5 003 records (k_assemble; frozen, adaptive, format 6) and 131 073 (k_assemble4; frozen, adaptive); then out_cap of size - 1, size / 2 and 1:
      SFQ_E_OVERFLOW with the size needed, or SFQ_E_CORRUPT, and not one byte of the tensor touched (assembly is not launched when the text does not
      fit); then the exact decode again.
  test_output_at_any_alignment   the same at 1 and 13 bytes past a sixteen-byte boundary, with and without checksums (CRCs == zlib.crc32 of the blocks).
  test_slack_does_not_show_in_the_text   out_cap of size, 128 * nrec - 1, 128 * nrec, 4 * size: qpad / spad off, off, on, on (api.cpp); flat (spad and
      qpad), match model (qpad), adaptive (neither), 131 073 records each: same text, same out_bytes, nothing behind the text touched.

Wall time on one MI355X, same machine: the GPU suite without this module 227 s (234 tests), this module alone 91 s (96 tests) -- over the tenth it was
given.  55 s of it are the two format-6 cases (one wave codes and reads 10.5 MB three times over; the generator's records average 80 bytes, and 131 072 of
them are what rpw = 4 needs), 11 s the first adaptive case at rpw = 4, 5 s the two rpw = 64 cases, which were kept: they are the only test of rpw = 64 on
anything but uniform reads.  The cross product is already thinned at rpw = 3, 6, 7 and 64; the classes of records are not.

Checked on scratch copies of k_assemble4: merge_n without `low` fails every case with 'n' in its text (k_assemble's too: the function is shared);
without the sl > ql tail loop every case from rpw = 4 up fails and the rpw = 1 cases pass.  `sub <= h` in the short-header branch changes no byte of the
output and cannot be caught: the one byte too many lands where the same wave stores the line's '\n' afterwards."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from slimfastq_amd import capi
from oracle import oracle as O
import util
from test_frozen_tables import check_against_oracle
from test_gpu_parity import KERNELS, _check_sampled_chains_against_oracle, assert_streams_equal

SFQ_E_OVERFLOW, SFQ_E_CORRUPT = -5, -6            # include/slimfastq_amd.h
GUARD = 64 << 10
CHUNK = 65536
_ALPHA = np.frombuffer(b"ACGTNacgtn0123456789:_/#.-=xyzXYZ", np.uint8)
_WORD = np.frombuffer(b"ACGTNacgtn0123456789xyzXYZ", np.uint8)
_POOL_READS, _POOL_LEN, _POOL_SHIFTS = 32, 1200, 8


def rpw_of(nrec):
    """Records a wave of the assembly kernel takes (decode_l.hip launch_assemble), restated"""
    return max(1, min(64, nrec // 32768))


def _hostile_chunk(first, n, seed, two_id, solid, n_byte, repeat_bases):
    rng = np.random.default_rng([seed, first // CHUNK])
    idx = first + np.arange(n, dtype=np.int64)
    # line lengths: 1..15, every residue mod 16 above, every thousandth record a header over 256 bytes / a base line of 300..1100
    u = rng.random(n)
    h = np.where(u < 0.55, rng.integers(1, 16, n), np.where(u < 0.95, rng.integers(16, 48, n), rng.integers(48, 101, n)))
    h = np.where(idx % 1000 == 7, 257 + (idx // 1000) % 140, h)
    u = rng.random(n)
    sl = np.where(u < 0.45, rng.integers(1, 16, n), np.where(u < 0.95, rng.integers(16, 64, n), rng.integers(64, 151, n)))
    sl = np.where(idx % 1000 == 500, 300 + (idx // 1000 * 37) % 801, sl)
    u = rng.random(n)                                     # (a quality line longer than its bases: the oracle takes it, both ways)
    ql = np.where(u < 0.5, sl, np.where(u < 0.95, np.maximum(1, sl - rng.integers(1, 41, n)), sl + rng.integers(1, 21, n)))
    # bases and qualities, drawn over the longer of a record's two lines
    ml = np.maximum(sl, ql)
    tot = int(ml.sum())
    rec = np.repeat(np.arange(n), ml)
    pos = np.arange(tot) - (np.cumsum(ml) - ml)[rec]
    letters = np.frombuffer(b"0123" if solid else b"ACGT", np.uint8)
    if repeat_bases:
        pool = np.random.default_rng([seed, 1 << 30]).integers(0, 4, _POOL_READS * _POOL_LEN)
        start = rng.integers(0, _POOL_READS, n) * _POOL_LEN + rng.integers(0, _POOL_SHIFTS, n)
        code = pool[start[rec] + pos]
    else:
        code = rng.integers(0, 4, tot)
    b = letters[code]
    q = rng.integers(35, 75, tot).astype(np.uint8)
    e = rng.random(tot)
    if solid:
        e = np.where(pos == 0, 1.0, e)                    # (a block is in colour space by its first record's first colour that is not a '.': frame.hip)
    nb = ord(".") if solid else ord(n_byte)
    is_n = e < 0.02                                       # N under '!' (e < 0.01), N under another quality
    bang = (e < 0.01) | ((e >= 0.02) & (e < 0.03)) | ((e >= 0.04) & (e < 0.05)) | ((e >= 0.06) & (e < 0.065))       # ... '!' over a real base ...
    lower = (e >= 0.03) & (e < 0.05)                      # a single lowercase base, and one under '!'
    low_n = (e >= 0.06) & (e < 0.07)                      # 'n' under '!', under another quality
    run = rng.random(n) < 0.04                            # a soft-masked stretch
    ra = (rng.random(n) * sl).astype(np.int64)
    rb = ra + 1 + (rng.random(n) * (sl - ra)).astype(np.int64)
    lower |= run[rec] & (pos >= ra[rec]) & (pos < rb[rec])
    b = np.where(is_n, nb, b)
    if not solid:
        b = np.where(lower & ~is_n, b | 0x20, b)
    b = np.where(low_n, ord("n") if (n_byte == "N" and not solid) else nb, b).astype(np.uint8)
    q = np.where(bang, 33, q).astype(np.uint8)
    qf = q[pos < ql[rec]]
    b = b[pos < sl[rec]]
    hrec = np.repeat(np.arange(n), h)                     # (a header has 64 fields at the most, recs.cpp:153-154: no separators behind its 60th byte)
    hpos = np.arange(int(h.sum())) - (np.cumsum(h) - h)[hrec]
    hf = np.where(hpos < 60, _ALPHA[rng.integers(0, len(_ALPHA), len(hpos))], _WORD[rng.integers(0, len(_WORD), len(hpos))])
    pf = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
    pq = rng.integers(35, 75, n).astype(np.uint8)
    # the lines' places: twelve pieces a record, their offsets a cumulative sum, all copied from one source array by one gather
    src = np.concatenate([np.frombuffer(b"@\n+", np.uint8), hf, b, qf, pf, pq])
    o_h = 3; o_b = o_h + len(hf); o_q = o_b + len(b); o_pf = o_q + len(qf); o_pq = o_pf + n
    h0, s0, q0 = np.cumsum(h) - h, np.cumsum(sl) - sl, np.cumsum(ql) - ql
    one = np.ones(n, np.int64); s = one * int(solid); ar = np.arange(n)
    at = np.stack([0 * one, o_h + h0, one, o_pf + ar, o_b + s0, one, 2 * one, o_h + h0, one, o_pq + ar, o_q + q0, one], 1).ravel()
    ln = np.stack([one, h, one, s, sl, one, one, h * int(two_id), one, s, ql, one], 1).ravel()
    return src[np.repeat(at - (np.cumsum(ln) - ln), ln) + np.arange(int(ln.sum()))].tobytes()


def hostile_fastq(nrec, seed, *, two_id, solid, n_byte, repeat_bases):
    """Hostile records at scale (the module's docstring lists what they hold); the same text for the same arguments."""
    assert n_byte in ("N", ".") and (n_byte == "." or not solid)
    return b"".join(_hostile_chunk(c, min(CHUNK, nrec - c), seed, two_id, solid, n_byte, repeat_bases) for c in range(0, nrec, CHUNK))


def coverage(fq, solid, n_byte):
    """How often every class of record and base that the assembly kernels treat differently occurs, read back from the text alone"""
    s = int(solid)
    a = np.frombuffer(fq, np.uint8)
    starts, lens = util.line_table(fq)
    starts = starts.astype(np.int64); lens = lens.astype(np.int64)
    h, sl, ql = lens[0::4] - 1, lens[1::4] - s, lens[3::4] - s
    n = len(h)
    md = np.minimum(sl, ql)
    out = {"nrec": n, "bytes_per_record": len(fq) // n}
    for name, v in (("h", h), ("sl", sl), ("ql_cut", ql[ql < sl]), ("md", md)):
        out[name + "_1_15"] = int(np.bincount(v[v < 16], minlength=16)[1:].min())                     # the rarest of the lengths 1..15
        out[name + "_residues"] = int(np.bincount(v[v >= 16] & 15, minlength=16).min())               # the rarest residue mod 16 above
    out["ql_over"] = int((ql > sl).sum())
    out["h_over_256"] = int((h > 256).sum())
    out["sl_300_1100"] = int(((sl >= 300) & (sl <= 1100)).sum())
    out["ql_equal"] = int((ql == sl).sum())
    out["ql_cut_by"] = int(np.bincount((sl - ql)[ql < sl], minlength=41)[1:41].min())                 # the rarest of the differences 1..40
    out["two_id"] = int((lens[2::4] == 1 + h).sum())
    out["plain_plus"] = int((lens[2::4] == 1).sum())
    rec = np.repeat(np.arange(n), sl)
    pos = np.arange(int(sl.sum())) - (np.cumsum(sl) - sl)[rec]
    c = a[(starts[1::4] + s)[rec] + pos]
    inq = pos < ql[rec]
    q = np.where(inq, a[np.minimum((starts[3::4] + s)[rec] + pos, len(a) - 1)], 0)
    full = (md & ~15)[rec]
    # where a base lies: in a whole sixteen-byte piece (counted per offset 0..15: the rarest), in the end piece that overlaps the one before, in a line
    # of under sixteen bytes (moved singly), behind the quality line's end (the sl > ql tail)
    where = {"piece": inq & (pos < full), "end_piece": inq & (md[rec] >= 16) & (pos >= full), "short": inq & (md[rec] < 16), "behind_ql": ~inq}
    nb = ord(".") if solid else ord(n_byte)
    low = (c >= ord("a")) & (c <= ord("z")) & (c != ord("n"))
    real = ~low & (c != nb) & (c != ord("n"))
    kind = {"N_bang": (c == nb) & (q == 33), "N_other": (c == nb) & (q != 33), "bang_real": real & (q == 33), "lower": low & (q != 33),
            "lower_bang": low & (q == 33), "n_bang": (c == ord("n")) & (q == 33), "n_other": (c == ord("n")) & (q != 33)}
    for k, km in kind.items():
        for w, wm in where.items():
            m = km & wm
            out[k + "/" + w] = int(np.bincount(pos[m] & 15, minlength=16).min()) if w == "piece" else int(m.sum())
    out["lower_runs"] = int((low[:-2] & low[1:-1] & low[2:] & (rec[:-2] == rec[2:])).sum())            # three lowercase bases in a row
    if solid:
        out["primers"] = int(np.isin(a[starts[1::4]], np.frombuffer(b"ACGT", np.uint8)).sum())
        out["colours"] = int(np.isin(c, np.frombuffer(b"0123.", np.uint8)).sum())
    return out


# What a text of 5 003 records must hold at least (conditions, not measurements: the generator as written gives two to four times as many); a text of
# 200 000 records thirty times that.  '/piece' counts are per offset 0..15 of a sixteen-byte piece.
MINIMA = {"h_1_15": 50, "h_residues": 40, "sl_1_15": 50, "sl_residues": 50, "ql_cut_1_15": 5, "ql_cut_residues": 10, "md_1_15": 30, "md_residues": 40,
          "ql_over": 100, "h_over_256": 3, "sl_300_1100": 3, "ql_equal": 1500, "ql_cut_by": 2,
          "N_bang/piece": 10, "N_bang/end_piece": 40, "N_bang/short": 40, "N_other/piece": 10, "N_other/end_piece": 40, "N_other/short": 40,
          "N_other/behind_ql": 100, "bang_real/piece": 10, "bang_real/end_piece": 40, "bang_real/short": 40}
MINIMA_CASE = {"lower/piece": 10, "lower/end_piece": 40, "lower/short": 40, "lower/behind_ql": 100, "lower_bang/piece": 10, "lower_bang/end_piece": 40,
               "lower_bang/short": 40, "lower_runs": 300}                                             # base space only
MINIMA_N = {"n_bang/piece": 5, "n_bang/end_piece": 25, "n_bang/short": 25, "n_other/piece": 5, "n_other/end_piece": 25, "n_other/short": 25,
            "n_other/behind_ql": 80}                                                                   # base space with 'N' only

# (two_id, solid, n_byte, repeat_bases): every switch set the format has -- colour space has '.' for its N byte; none was refused by the oracle
SWITCHES = [(t, s, nb, r) for t, s, nb in ((0, 0, "N"), (0, 0, "."), (0, 1, "."), (1, 0, "N"), (1, 0, "."), (1, 1, ".")) for r in (0, 1)]
THIN = [(0, 0, "N", 0), (1, 0, ".", 1), (1, 1, ".", 0), (0, 1, ".", 1)]       # every switch on once and off once; iid and pooled bases
SEED = 5003
N_RPW = {1: 5003, 3: 4 * 32768 - 1, 4: 4 * 32768 + 1, 6: 6 * 32768 + 5, 7: 7 * 32768 + 3, 64: 64 * 32768 + 37}


@functools.lru_cache(maxsize=2)
def text(nrec, sw):
    return hostile_fastq(nrec, SEED, two_id=bool(sw[0]), solid=bool(sw[1]), n_byte=sw[2], repeat_bases=bool(sw[3]))


def _check_minima(cov, sw, scale):
    need = dict(MINIMA)
    if not sw[1]:
        need.update(MINIMA_CASE)
        if sw[2] == "N":
            need.update(MINIMA_N)
    for k, v in need.items():
        assert cov[k] >= v * scale, (sw, k, cov[k], v * scale)
    n = cov["nrec"]
    assert (cov["two_id"], cov["plain_plus"]) == ((n, 0) if sw[0] else (0, n))
    if sw[1]:
        assert cov["primers"] == n and cov["colours"] > 0 and cov["lower/piece"] == 0
    assert cov["bytes_per_record"] < 128                  # (the caller's slack chooses the staging at 128 bytes a record: api.cpp qpad / spad)


def test_hostile_text_covers_every_class_and_the_oracle_takes_it():
    for sw in SWITCHES:
        fq = text(N_RPW[1], sw)
        assert fq == hostile_fastq(N_RPW[1], SEED, two_id=bool(sw[0]), solid=bool(sw[1]), n_byte=sw[2], repeat_bases=bool(sw[3]))
        _check_minima(coverage(fq, sw[1], sw[2]), sw, 1)
    for sw in THIN:
        _check_minima(coverage(text(200_000, sw), sw[1], sw[2]), sw, 30)
    # the oracle takes every switch set: the block format a block a time (lossless), format 6 where 'n' does not meet 'N'
    for sw in SWITCHES:
        fq = hostile_fastq(3000, 7, two_id=bool(sw[0]), solid=bool(sw[1]), n_byte=sw[2], repeat_bases=bool(sw[3]))
        for chunk in util.split_records(fq, 1024):
            ref = util.block_reference(chunk, 3)
            assert O.decompress(ref.image) == chunk, sw
        if sw[2] == ".":
            back = O.decompress(O.compress(fq, 3).image)       # (lossy where the reference is: lowercase bases, some header fields -- SURVEY H7)
            assert back.count(b"\n") == fq.count(b"\n"), sw
        else:
            with pytest.raises(O.OracleError):            # "switched N_byte" (gens.cpp:107-108): format 6 runs with '.' below
                O.compress(fq, 3)


# ---- 2. assembly at every rpw ---------------------------------------------------------------------------------------------------------------------
def _matrix():
    for rpw, n in N_RPW.items():
        if rpw == 64:
            yield rpw, (1, 0, "N", 0), capi.TABLES_FROZEN
            yield rpw, (0, 1, ".", 1), capi.TABLES_ADAPTIVE
            continue
        for sw in (SWITCHES if rpw in (1, 4) else THIN):
            for tables in (capi.TABLES_FROZEN, capi.TABLES_ADAPTIVE):
                yield rpw, sw, tables


def _record_starts(fq):
    starts, _ = util.line_table(fq)
    return np.concatenate((starts[0::4].astype(np.int64), [len(fq)]))


@pytest.mark.gpu
@pytest.mark.parametrize("rpw,sw,tables", list(_matrix()), ids=lambda v: "".join(str(x) for x in v) if isinstance(v, tuple) else str(v))
def test_assembly_at_every_records_per_wave(ctx, rpw, sw, tables):
    nrec = N_RPW[rpw]
    assert rpw_of(nrec) == rpw and (rpw < 4 or nrec % rpw) and (rpw != 64 or nrec >= 2_097_152)
    fq = text(nrec, sw)
    br, cr = 1024, 64
    if tables == capi.TABLES_FROZEN:
        full = rpw == 1 or (rpw in (3, 4) and sw in THIN[:2])
        if full:
            enc = check_against_oracle(ctx, fq, 3, br=br, cr=cr, step=1 if rpw == 1 else 4, what=str((rpw, sw)))
        else:
            enc = ctx.encode_host(fq, level=3, block_reads=br, prior_step=capi.PRIOR_AUTO, tables=tables, chain_reads=cr)
        ci = util.unpack_chains(enc.chains)
        if sw[3]:
            assert ci["flags"] & 32                                            # pooled bases: the match model, its stage
        else:
            assert ci["flags"] & 192 == 128 and ci["flags"] & 16 and not ci["flags"] & (1 | 32)      # iid bases: flat, two bits each, Rice-coded lists
            if not full and not sw[1]:
                import torch
                _check_sampled_chains_against_oracle(fq, torch.from_numpy(np.frombuffer(enc.data, np.uint8).copy()), list(enc.res.stream_offset), ci,
                                                     enc.prior, enc.rec_prior, enc.blocks, 3, per_stream=16)
    else:
        enc = ctx.encode_host(fq, level=3, block_reads=br, tables=tables)
        assert not enc.chains
        rs = _record_starts(fq)
        nb = len(enc.blocks)
        assert nb == -(-nrec // br)
        rng = np.random.default_rng(nrec)
        for b in sorted({0, nb - 1} | set(rng.integers(0, nb, 16).tolist())):
            chunk = fq[int(rs[b * br]): int(rs[min((b + 1) * br, nrec)])]
            assert_streams_equal(enc, util.block_reference(chunk, 3, gen_bits=enc.blocks[b].gen_bits).streams, block=b, ctxmsg="%s block %d" % ((rpw, sw), b))
    assert all(b.solid == sw[1] and b.two_id == sw[0] for b in enc.blocks)
    got = ctx.decode_host(enc, level=3, out_cap=len(fq))                       # the exact capacity, as the CLI gives it
    assert got == fq
    if tables == capi.TABLES_FROZEN and rpw != 64:                             # room for the padded stages (128 bytes a record or more)
        assert len(fq) // nrec < 128
        assert ctx.decode_host(enc, level=3, out_cap=128 * nrec) == fq


def _short_enough_for_format_6(fq, keep):
    """The first `keep` records (format 6 is one block, a few MB/s by design)"""
    return fq[: int(_record_starts(fq)[keep])]


@pytest.mark.gpu
@pytest.mark.parametrize("oversize", (False, True))
def test_format_6_at_four_records_a_wave(ctx, oversize):
    nrec = N_RPW[4]
    fq = text(nrec, (0, 0, ".", 0))
    if oversize:                                                               # two records whose base and quality lines pass 65 534 bytes
        rs = _record_starts(fq)
        rng = np.random.default_rng(9)
        big = []
        for i, n in enumerate((70_000, 65_535)):
            seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy(); seq[500:507] = ord(".")
            qual = rng.integers(35, 75, n).astype(np.uint8); qual[500:507] = 33
            big.append(b"@over.%d len=%d\n" % (i, n) + seq.tobytes() + b"\n+\n" + qual.tobytes() + b"\n")
        cut = [int(rs[1000]), int(rs[nrec - 3])]
        fq = fq[:cut[0]] + big[0] + fq[cut[0]:cut[1]] + big[1] + fq[cut[1]:]
    assert rpw_of(nrec) == 4 and nrec % 4                                       # (the oversize records are laid out by launch_over_place, not by the wave)
    ref = O.compress(fq, 3)
    want = O.decompress(ref.image)
    enc = ctx.encode_host(fq, level=3, block_reads=0)
    assert_streams_equal(enc, ref.streams, ctxmsg="format 6, oversize %s" % oversize)
    assert enc.res.n_records == nrec + 2 * oversize
    assert bool(enc.blocks[0].size[capi.STREAM_NAMES.index("usr.lrec")]) == oversize
    for kernel in KERNELS:
        assert ctx.decode_host(enc, level=3, out_cap=len(want), kernel=kernel) == want, kernel


# ---- 3. the caller's buffer -----------------------------------------------------------------------------------------------------------------------
class _OnDevice:
    """An archive whose streams lie in device memory (sfq_encode_blocks), and the raw sfq_decode_blocks call: status and *out_bytes, no exception"""

    def __init__(self, ctx, fq, **kw):
        import torch
        self.ctx = ctx
        d_in = torch.from_numpy(np.frombuffer(fq, np.uint8).copy()).cuda()
        cap = capi.lib().sfq_encode_bound(len(fq))
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        res = ctx.encode_device(d_in.data_ptr(), len(fq), d_out.data_ptr(), cap, **kw)
        torch.cuda.synchronize()
        self.blocks, self.first = ctx.index(res.n_blocks), ctx.first_headers(res.first_hdr_bytes)
        self.d = d_out[:res.total_bytes].clone()
        self.soff = list(res.stream_offset)
        self.prior, self.chains, self.rec_prior = ctx.prior(), ctx.chains(), ctx.rec_prior()
        self.nrec = int(res.n_records)

    def decode(self, d_out, cap, kernel=0):
        import torch
        L, ctx = capi.lib(), self.ctx
        ctx._check(L.sfq_set_qlt_prior(ctx.handle, self.prior if self.prior else None, len(self.prior)))
        ctx._check(L.sfq_set_chain_index(ctx.handle, self.chains if self.chains else None, len(self.chains)))
        ctx._check(L.sfq_set_rec_prior(ctx.handle, self.rec_prior if self.rec_prior else None, len(self.rec_prior)))
        p = capi.Params(3, 0, 0, 0, kernel, 0, 0, 0, 0, 0)
        res, n = capi.Result(), C.c_uint64(0)
        fb = np.frombuffer(self.first if len(self.first) else b"\0", np.uint8)
        soff = (C.c_uint64 * capi.NSTREAMS)(*self.soff)
        torch.cuda.synchronize()                                               # (the fills of the test's tensor are through)
        rc = L.sfq_decode_blocks(ctx.handle, C.byref(p), self.blocks, len(self.blocks), fb.ctypes.data_as(C.c_void_p), len(self.first),
                                 C.c_void_p(self.d.data_ptr()), soff, C.c_void_p(d_out), cap, C.byref(n), C.byref(res))
        torch.cuda.synchronize()
        return rc, n.value


def _guarded(nbytes, off=0):
    import torch
    buf = torch.full((GUARD + off + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and GUARD % 16 == 0
    return buf, GUARD + off


def _all_a5(t):
    return bool((t == 0xA5).all())


KW = {"frozen": dict(level=3, block_reads=1024, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN, chain_reads=64),
      "adaptive": dict(level=3, block_reads=1024, tables=capi.TABLES_ADAPTIVE),
      "format6": dict(level=3, block_reads=0)}


@pytest.mark.gpu
@pytest.mark.parametrize("rpw,mode", ((1, "frozen"), (1, "adaptive"), (1, "format6"), (4, "frozen"), (4, "adaptive")))
def test_exact_capacity_and_guards(ctx, rpw, mode):
    import torch
    nrec = N_RPW[rpw]
    assert rpw_of(nrec) == rpw
    fq = text(nrec, (1, 0, ".", 0))
    want = O.decompress(O.compress(fq, 3).image) if mode == "format6" else fq      # (format 6 gives back what the reference gives back)
    nbytes = len(want)
    arch = _OnDevice(ctx, fq, **KW[mode])
    d_want = torch.from_numpy(np.frombuffer(want, np.uint8).copy()).cuda()
    buf, at = _guarded(nbytes)
    rc, n = arch.decode(buf.data_ptr() + at, nbytes)
    assert rc == 0 and n == nbytes
    assert torch.equal(buf[at:at + nbytes], d_want)
    assert _all_a5(buf[:at]) and _all_a5(buf[at + nbytes:])
    for cap in (nbytes - 1, nbytes // 2, 1):
        buf.fill_(0xA5)
        rc, n = arch.decode(buf.data_ptr() + at, cap)
        assert rc in (SFQ_E_OVERFLOW, SFQ_E_CORRUPT), (cap, rc)
        if rc == SFQ_E_OVERFLOW:
            assert n == nbytes, cap                                            # the size a second try needs (the CLI's retry)
        assert _all_a5(buf[at + cap:]), cap                                    # nothing behind the caller's capacity
        assert _all_a5(buf[:at + cap]), cap                                    # and nothing inside it: the records are not laid out unless all of them fit
    buf.fill_(0xA5)
    rc, n = arch.decode(buf.data_ptr() + at, nbytes)
    assert rc == 0 and n == nbytes and torch.equal(buf[at:at + nbytes], d_want)
    assert _all_a5(buf[:at]) and _all_a5(buf[at + nbytes:])


@pytest.mark.gpu
@pytest.mark.parametrize("checksums", (False, True))
@pytest.mark.parametrize("off", (1, 13))
@pytest.mark.parametrize("rpw,mode", ((1, "frozen"), (4, "frozen"), (4, "adaptive")))
def test_output_at_any_alignment(ctx, rpw, mode, off, checksums):
    import torch
    nrec = N_RPW[rpw]
    assert rpw_of(nrec) == rpw
    fq = text(nrec, (1, 0, ".", 0))
    arch = _OnDevice(ctx, fq, **KW[mode])
    d_want = torch.from_numpy(np.frombuffer(fq, np.uint8).copy()).cuda()
    buf, at = _guarded(len(fq), off)
    assert (buf.data_ptr() + at) % 16 == off
    ctx.set_checksums(checksums)
    try:
        rc, n = arch.decode(buf.data_ptr() + at, len(fq))
        crcs, whole = ctx.checksums()
    finally:
        ctx.set_checksums(False)
    assert rc == 0 and n == len(fq)
    assert torch.equal(buf[at:at + n], d_want)
    assert _all_a5(buf[:at]) and _all_a5(buf[at + n:])
    if checksums:
        rs = _record_starts(fq)
        br = 1024
        assert crcs == [zlib.crc32(fq[int(rs[r]): int(rs[min(r + br, nrec)])]) for r in range(0, nrec, br)]
        assert whole == zlib.crc32(fq)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,repeat", (("frozen", 0), ("frozen", 1), ("adaptive", 0)))
def test_slack_does_not_show_in_the_text(ctx, mode, repeat):
    import torch
    nrec = N_RPW[4]
    assert rpw_of(nrec) == 4
    fq = text(nrec, (1, 0, "N", repeat))
    nbytes = len(fq)
    assert nbytes // nrec < 128 and nbytes < 128 * nrec - 1 < 4 * nbytes
    arch = _OnDevice(ctx, fq, **KW[mode])
    if mode == "frozen":
        flags = util.unpack_chains(arch.chains)["flags"]
        assert (flags & 32) if repeat else (flags & 192 == 128 and flags & 16 and not flags & (1 | 32))
    else:
        assert not arch.chains
    d_want = torch.from_numpy(np.frombuffer(fq, np.uint8).copy()).cuda()
    buf, at = _guarded(4 * nbytes)
    for cap in (nbytes, 128 * nrec - 1, 128 * nrec, 4 * nbytes):
        assert (cap // nrec >= 128) == (cap >= 128 * nrec)                     # the rule that picks qpad / spad, on either side
        buf.fill_(0xA5)
        rc, n = arch.decode(buf.data_ptr() + at, cap)
        assert rc == 0 and n == nbytes, cap
        assert torch.equal(buf[at:at + nbytes], d_want), cap
        assert _all_a5(buf[:at]) and _all_a5(buf[at + nbytes:]), cap           # the bytes behind *out_bytes are the caller's

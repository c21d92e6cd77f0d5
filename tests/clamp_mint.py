"""FASTQ text that makes the range coder take its interval clamp (coder.hpp:76-77), minted on the CPU from a seed.

The clamp runs where [low, low + range) crosses a multiple of 2^56 during renormalisation: with range < 2^24 that needs bits 24..55 of
low all ones, once in 2^32 steps -- no ordinary text gets there.  A DECODER fed the bytes X, 0xFF x 6, 0x00 (X != 0xFF) does, when X
becomes its top byte: the code value lies just below the multiple, the interval around it crosses it, and the value is still inside
after the clamp.  The text such a decoder writes is a symbol sequence whose ENCODING runs through the same (low, range) states, so it
clamps in the same places.  The oracle's steered decoders (sfq_oracle.c "MINTING") keep that text legal: they take only admitted
symbols and repair a code value that ends up outside its interval.

Every text here is a function of its arguments (a seed among them) and nothing else, cached for the tests that qualify it on the CPU
(test_clamp_inputs.py) and for GPU tests that encode it.  The crafted bytes go to the CPU oracle alone: a GPU only ever sees the text."""
import functools

import numpy as np

import util
from oracle import oracle as O
from slimfastq_amd import capi

PRIOR_SYMBOLS = 4096
LEVEL_BITS = {1: 18, 2: 22, 3: 24, 4: 26}
GEN_STEP = 4
MIN_CLAMPS = 8


def q_rows(level):
    return 4096 if level == 1 else 65536


def target_streams(rng, n, nbytes, gap):
    """n target streams of nbytes each: the pattern, `gap` random bytes, the pattern, ...  (the streams start with random bytes)."""
    out = []
    for _ in range(n):
        s = bytearray()
        while len(s) < nbytes:
            s += bytes(rng.integers(0, 256, gap, dtype=np.uint8))
            s += bytes([int(rng.integers(0, 255))]) + b"\xff" * 6 + b"\x00"
        out.append(bytes(s[:nbytes]))
    return b"".join(out), np.full(n, nbytes, np.uint32)


def records(fq):
    lines = fq.split(b"\n")[:-1]
    return [lines[i:i + 4] for i in range(0, len(lines), 4)]


def join(recs):
    return b"".join(b"\n".join(r) + b"\n" for r in recs)


def with_lines(fq, which, buf):
    """fq with line `which` (1 = bases, 3 = qualities) of every record taken from buf, which holds them at the places fq has them."""
    starts, lens = util.line_table(fq)
    out = bytearray(fq)
    for o, n in zip(starts[which::4], lens[which::4]):
        out[int(o):int(o) + int(n)] = buf[int(o):int(o) + int(n)]
    return bytes(out)


def ordinary(nrec, lens, seed):
    """Synthetic records with the given line lengths (each at most 150) and no N: what the minted lines replace."""
    recs = records(capi.synth_fastq(nrec, 150, seed=seed).replace(b"N", b"A"))
    for r, n in zip(recs, lens):
        r[1], r[3] = r[1][:n], r[3][:n]
    return join(recs)


def pack_prior(rows66):
    """Prior rows [q_rows, 66] -> "qlt.pri" (util.unpack_prior's inverse; api.cpp pack_prior)."""
    out = bytearray()
    util.put_v(out, len(rows66))
    prev = 0
    for c in np.flatnonzero(rows66[:, 65]):
        r = rows66[c]
        iend = int(r[65])
        nnz = 0
        while nnz < iend and r[nnz] & 0xffff:
            nnz += 1
        util.put_v(out, int(c) - prev + 1); prev = int(c)
        out += bytes([iend, nnz])
        for j in range(nnz):
            out.append(int(r[j]) >> 16)
            util.put_v(out, int(r[j]) & 0xffff)
    util.put_v(out, 0)
    return bytes(out)


def pack_rec_prior(f):
    """Header prior frequencies [66 * 16 * 256] -> "rec.pri" (util.unpack_rec_prior's inverse; api.cpp pack_rec_prior_f)."""
    out = bytearray()
    f = np.asarray(f).reshape(-1, 256)
    util.put_v(out, len(f))
    prev = 0
    for r in np.flatnonzero(f.any(axis=1)):
        util.put_v(out, int(r) - prev + 1); prev = int(r)
        nz = np.flatnonzero(f[r])
        util.put_v(out, len(nz))
        for s in nz:
            out.append(int(s))
            util.put_v(out, int(f[r, s]))
    util.put_v(out, 0)
    return bytes(out)


def rec_sample(nrec):
    run = 6                                       # api.cpp REC_PRIOR_RUN / REC_PRIOR_RUNS (short headers)
    nruns = min(32768, max(1, nrec // run))
    return max(run, nrec // nruns), run, nruns


ADMITTED = tuple(range(1, 63))                # every quality symbol but '!' (which would also mark its base) and the escape: legal text, '"' .. '^'


def is_legal(fq):
    for r in records(fq):
        if len(r[1]) != len(r[3]) or r[2] != b"+" or not r[0].startswith(b"@"):
            return False
        if set(r[1]) - set(b"ACGT") or (r[3] and not (33 <= min(r[3]) and max(r[3]) <= 126)):
            return False
    return True


# ---- frozen tables, qualities ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frozen_qlt(level, seed, nchains, cr, minted, lens=None, seg=0, gap=6):
    """nchains chains of cr records (seg: every record cut into segments of seg symbols, the chains), chains `minted` (a tuple of chain
    numbers, or "all") minted under the frozen rows of the ordinary text's prior.  -> dict(fq, plain, prior, rec_prior, rows66, br, cr)."""
    nrec = nchains * cr if not seg else nchains
    lens = tuple(lens) if lens is not None else (150,) * nrec
    plain = ordinary(nrec, lens, seed)
    starts, ll = util.line_table(plain)
    qoff, qlen, glen = starts[3::4], ll[3::4], ll[1::4]
    rows66 = O.qlt_prior_rows(O.qlt_histogram(plain, qoff, np.minimum(qlen, PRIOR_SYMBOLS), level, 0, 1))
    frozen = O.qlt_frozen_rows(rows66)
    rng = np.random.default_rng(seed)
    if seg:
        nseg = O.seg_counts(qlen, glen, seg)
        first = np.concatenate([[0], np.cumsum(nseg)])
        streams, sizes = target_streams(rng, int(nseg.sum()), 2 * seg, gap)
        buf = O.qlt_decode_segs(streams, sizes, qoff, qlen, glen, level, seg, frozen, ADMITTED)
        chain_recs = lambda c: [int(np.searchsorted(first, c, side="right")) - 1]
    else:
        streams, sizes = target_streams(rng, nchains, 2 * 150 * cr, gap)
        buf = O.qlt_decode_chains(streams, sizes, qoff, qlen, level, nrec, cr, frozen, ADMITTED)
        chain_recs = lambda c: range(c * cr, (c + 1) * cr)
    mint = with_lines(plain, 3, buf)
    if minted == "all":
        fq = mint
    else:
        recs, mrecs = records(plain), records(mint)
        for c in minted:
            for r in chain_recs(c):
                recs[r] = mrecs[r]
        fq = join(recs)
    hoff, hlen = starts[0::4] + 1, ll[0::4] - 1
    f = O.rec_prior_freqs(O.rec_count(fq, hoff, hlen, *rec_sample(nrec)))
    return dict(fq=fq, plain=plain, prior=pack_prior(rows66), rec_prior=pack_rec_prior(f), rec_f=f, rows66=rows66, frozen=frozen, br=nrec, cr=cr,
                seg=seg, level=level)


def frozen_qlt_streams(t, fq=None):
    """The oracle's quality chains of a frozen_qlt text (or of another text under its rows) -> (streams, sizes, escapes)."""
    fq = t["fq"] if fq is None else fq
    starts, ll = util.line_table(fq)
    if t["seg"]:
        return O.qlt_encode_segs(fq, starts[3::4], ll[3::4], ll[1::4], t["level"], t["seg"], t["frozen"])
    return O.qlt_encode_chains(fq, starts[3::4], ll[3::4], t["level"], t["br"], t["cr"], t["frozen"])


def frozen_qlt_back(t, streams, sizes):
    starts, ll = util.line_table(t["fq"])
    if t["seg"]:
        buf = O.qlt_decode_segs(streams, sizes, starts[3::4], ll[3::4], ll[1::4], t["level"], t["seg"], t["frozen"])
    else:
        buf = O.qlt_decode_chains(streams, sizes, starts[3::4], ll[3::4], t["level"], t["br"], t["cr"], t["frozen"])
    return with_lines(t["fq"], 3, buf)


# ---- adaptive tables: format 6 (br = 0) and the block format -------------------------------------------------------
ADAPTIVE_QUALITIES = tuple(range(2, 42))      # what cold adaptive rows are steered through: '#' .. 'J' (fresh rows give the escape 1 / 64: a plain decode would take it)


@functools.lru_cache(maxsize=None)
def adaptive(level, seed, nrec, br, gen_bits, given_prior=False, mint_qlt=True, gap=6):
    """nrec records of 120 symbols in blocks of br (0: format 6, one stream each), their base lines minted under cold Base2 rows of
    gen_bits, their quality lines under the adaptive rows: cold, or (given_prior) started from the prior of the ordinary text, which
    the encoder must then be GIVEN.  -> dict(fq, plain, rows66, prior)."""
    plain = ordinary(nrec, (120,) * nrec, seed)
    starts, ll = util.line_table(plain)
    rng = np.random.default_rng(seed)
    per = br if br else nrec
    nb = -(-nrec // per)
    streams, sizes = target_streams(rng, nb, 60 * per, gap)
    fq = with_lines(plain, 1, O.gen_steer_blocks(streams, sizes, starts[1::4], ll[1::4], gen_bits, per))
    rows66 = None
    if given_prior:
        rows66 = O.qlt_prior_rows(O.qlt_histogram(plain, starts[3::4], np.minimum(ll[3::4], PRIOR_SYMBOLS), level, 0, 1))
    if mint_qlt:
        streams, sizes = target_streams(rng, nb, 120 * per, gap)
        adm = ADMITTED if given_prior else ADAPTIVE_QUALITIES
        fq = with_lines(fq, 3, O.qlt_steer_blocks(streams, sizes, starts[3::4], ll[3::4], level, per, adm, rows66))
    return dict(fq=fq, plain=plain, rows66=rows66, prior=pack_prior(rows66) if given_prior else b"", level=level, br=br, per=per, gen_bits=gen_bits)


def adaptive_qlt_streams(t, fq=None):
    fq = t["fq"] if fq is None else fq
    starts, ll = util.line_table(fq)
    return O.qlt_encode_blocks(fq, starts[3::4], ll[3::4], t["level"], t["per"], t["rows66"])


def adaptive_gen_streams(t, fq=None):
    """The blocks' base streams, each the reference's for a file holding that block."""
    fq = t["fq"] if fq is None else fq
    out = []
    for chunk in util.split_records(fq, t["per"]):
        starts, ll = util.line_table(chunk)
        out.append(O.gen_encode(chunk, starts[1::4], ll[1::4], starts[3::4], ll[3::4], t["gen_bits"])[0])
    return out


# ---- frozen tables, bases: the match model, and the generation tables of kernel = 2 -------------------------------------
def folded_genome_reads(n, seed):
    """Reads of a tiny genome (rotated copies of 300 reads), so that the base models pay at test size."""
    recs = records(capi.synth_fastq(n, 150, seed=seed, kind=3).replace(b"N", b"A"))
    reads = [r[1] for r in recs[:300]]
    rng = np.random.default_rng(seed)
    for r in recs:
        src = reads[rng.integers(len(reads))]
        k = int(rng.integers(0, 40))
        r[1] = src[k:] + src[:k]
    return join(recs)


def generation_bounds(nblocks):
    bound = [0]; b = max(1, -(-nblocks // 64))
    while b < nblocks and len(bound) + 1 < 40:
        bound.append(b); b = max(b + 1, b * 2)
    bound.append(nblocks)
    return bound


def gm_table_bits(nbytes):
    tb = 16
    while tb < 24 and (1 << tb) < nbytes // 16:
        tb += 1
    return tb


@functools.lru_cache(maxsize=None)
def frozen_bases(model, seed, nrec=6000, br=32, cr=8, gen_bits=16, gap=6):
    """Reads the base model pays for, the base chains of the LAST generation (which no later one learns from... and which learns from all
    before it) minted: decoded from target streams under the model as the earlier generations leave it.  model: "gm" (the match model) or
    "tables" (kernel = 2's generation tables).  -> dict(fq, plain, first: the first minted chain)."""
    plain = folded_genome_reads(nrec, seed)
    starts, ll = util.line_table(plain)
    goff, glen = starts[1::4], ll[1::4]
    tb = gm_table_bits(len(plain))
    if model == "gm":
        streams, sizes, on = O.gm_encode_chains(plain, goff, glen, tb, br, cr)
    else:
        streams, sizes, on = O.gen_encode_chains(plain, goff, glen, gen_bits, br, cr, GEN_STEP)
    assert on == 1
    bound = generation_bounds(-(-nrec // br))
    first = bound[-2] * (br // cr)
    at = int(sizes[:first].sum())
    rng = np.random.default_rng(seed)
    t_streams, t_sizes = target_streams(rng, len(sizes) - first, 2 * 40 * cr, gap)
    streams = streams[:at] + t_streams
    sizes = np.concatenate([sizes[:first], t_sizes])
    if model == "gm":
        codes = O.gm_decode_chains(streams, sizes, glen, tb, br, cr, steer=True)
        letters = np.frombuffer(b"ACGT", np.uint8)[codes].tobytes()
        recs, p = records(plain), 0
        for r in recs:
            r[1] = letters[p:p + len(r[1])]; p += len(r[1])
        fq = join(recs)
    else:
        fq = with_lines(plain, 1, O.gen_decode_chains(streams, sizes, goff, glen, gen_bits, br, cr, GEN_STEP, 1, steer=True))
    return dict(fq=fq, plain=plain, first=first, br=br, cr=cr, tb=tb, gen_bits=gen_bits, model=model)


def frozen_bases_streams(t, fq=None):
    fq = t["fq"] if fq is None else fq
    starts, ll = util.line_table(fq)
    if t["model"] == "gm":
        return O.gm_encode_chains(fq, starts[1::4], ll[1::4], t["tb"], t["br"], t["cr"])
    return O.gen_encode_chains(fq, starts[1::4], ll[1::4], t["gen_bits"], t["br"], t["cr"], GEN_STEP)


def clamps_of(fn, *a, **k):
    """(fn's result, the clamps the oracle's coders took while it ran)."""
    O.rc_clamps(True)
    out = fn(*a, **k)
    return out, O.rc_clamps(True)


# ---- the texts: test_clamp_inputs.py qualifies every one on the CPU; they are the inputs for GPU cases, one per row ---------------------------
_RAGGED = tuple(20 + 2 * (r // 2) for r in range(128))          # 64 chains of two records, chain c's lines 20 + 2 c symbols long
FROZEN_QLT = {        # name -> frozen_qlt's arguments
    "all-lanes-level1": (1, 21, 128, 4, "all"),
    "all-lanes-level3": (3, 23, 128, 4, "all"),
    "all-lanes-level4": (4, 24, 64, 4, "all"),
    "lane0": (3, 30, 64, 8, (0,)),
    "lane31": (3, 31, 64, 8, (31,)),
    "lane63": (3, 32, 64, 8, (63,)),
    "unequal-lengths": (2, 33, 64, 2, "all", _RAGGED),
    "segments": (3, 34, 256, 0, "all", None, 75),
}
FORMAT6 = {level: (level, 40 + level, 600, 0, LEVEL_BITS[level]) for level in (1, 2, 3, 4)}                # adaptive()'s arguments
BLOCKS = {            # name -> (adaptive()'s arguments, the encoder's prior_step)
    "cold-level3": ((3, 50, 64 * 32, 32, 12), 0),
    "cold-level1": ((1, 51, 64 * 16, 16, 12), 0),
    "counted-prior": ((3, 52, 64 * 32, 32, 12, False, False), 1),           # the prior is counted over the text itself: only the bases are minted
    "given-prior": ((3, 53, 64 * 32, 32, 12, True), capi.PRIOR_GIVEN),
}
FROZEN_BASES = {"gm": ("gm", 60, 6000, 32, 4), "tables": ("tables", 61, 6000, 32, 8)}

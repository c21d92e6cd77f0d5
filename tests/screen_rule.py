"""The rule of the screened records (slimfastq_amd.h "screened records") restated in Python, independently of the C code: canonical
k-mers as integers, the set as a Python set, a FASTA file flattened line by line.  What the tests of scr.hip stand against."""
CODE = {ord(c): i for i, c in enumerate("ACGT")}
CODE.update({ord(c): i for i, c in enumerate("acgt")})
TO_END = 0xFFFFFFFFFFFFFFFF
MULT = 0x9E3779B97F4A7C15


def canon(window: bytes):
    """the canonical value of k bytes without a break"""
    f = r = 0
    for b in window:
        f = 4 * f + CODE[b]
    for b in reversed(window):
        r = 4 * r + 3 - CODE[b]
    return min(f, r)


def windows(seq: bytes, k):
    """the canonical values of the windows of a line or a sequence text, by position"""
    return [canon(seq[i:i + k]) for i in range(len(seq) - k + 1) if all(b in CODE for b in seq[i:i + k])]


def kmer_set(k, *texts):
    return {v for t in texts for v in windows(t, k)}


def home_slot(value, slots):
    """where the documented table looks for a k-mer first: the top bits of value * MULT mod 2^64"""
    return ((value * MULT) & (2 ** 64 - 1)) >> (64 - (slots.bit_length() - 1))


def slots_of(max_kmers):
    s = 2
    while s < 2 * max_kmers:
        s *= 2
    return s


def flat_fasta(fa: bytes):
    """sfq_fasta_sequences' rule: a '>' line is one '\\n'; every other line without its '\\n' and a '\\r' in front of it"""
    out = []
    lines = fa.split(b"\n")
    ends = [True] * (len(lines) - 1) + [False]                         # whether the line ended in '\n'
    if lines[-1] == b"":
        lines, ends = lines[:-1], ends[:-1]
    for l, nl in zip(lines, ends):
        if l[:1] == b">":
            out.append(b"\n")
        else:
            out.append(l[:-1] if nl and l[-1:] == b"\r" else l)
    return b"".join(out)


def records(fq: bytes):
    lines = fq.split(b"\n")
    lines = [l + b"\n" for l in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    assert len(lines) % 4 == 0
    return [b"".join(lines[i:i + 4]) for i in range(0, len(lines), 4)]


def hw(rec: bytes, k, kset):
    """(H, W) of a record"""
    w = windows(rec.split(b"\n")[1], k)
    return sum(1 for v in w if v in kset), len(w)


def screen(fq: bytes, rule, k, kset):
    """(the kept records' numbers, n_units, the matched records, the sum of W, the sum of H)"""
    rs = records(fq)
    G = 2 if rule.pairs else 1
    hi = len(rs) if rule.n_records == TO_END else rule.first_record + rule.n_records
    assert hi <= len(rs) and (hi - rule.first_record) % G == 0
    kept, nm, sw, sh = [], 0, 0, 0
    for r in range(rule.first_record, hi, G):
        m = []
        for g in range(G):
            H, W = hw(rs[r + g], k, kset)
            m.append(H >= rule.min_hits and 100 * H >= rule.min_pct * W)
            sw, sh = sw + W, sh + H
        nm += sum(m)
        matched = all(m) if rule.pairs == 2 else any(m)
        if matched == bool(rule.keep_matched):
            kept += list(range(r, r + G))
    return kept, (hi - rule.first_record) // G, nm, sw, sh

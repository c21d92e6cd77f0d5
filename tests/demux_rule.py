"""The rule of slimfastq_amd.h "demultiplexed records", restated in Python independently of the C and HIP code: lines by bytes.split,
fields by rfind and find, distances by a loop over bytes.  demux() gives what sfq_demux_records must give, byte for byte, or raises
Refused with the code the call must return."""
from operator import ne

TO_END = 2 ** 64 - 1
HEADER, BASES = 1, 2
E_ARG, E_FORMAT, E_OVERFLOW, E_UNSUPPORTED = -1, -4, -5, -7
ACGT = b"ACGT"


class Refused(Exception):
    def __init__(self, code, what, record=None, offset=None):
        super().__init__("%d: %s" % (code, what))
        self.code, self.record, self.offset = code, record, offset


def lines(fq):
    """the text's lines without their '\\n'; a text without a final '\\n' still ends in a line"""
    ls = fq.split(b"\n")
    if fq.endswith(b"\n"):
        ls.pop()
    return ls


def records(fq):
    """the records as lists of four lines"""
    ls = lines(fq)
    return [ls[i:i + 4] for i in range(0, len(ls) - len(ls) % 4, 4)]


def text_of(rec):
    return b"".join(l + b"\n" for l in rec)


def check(rule, barcodes):
    """sfq_demux_check: True where the rule and the barcode rows are accepted"""
    if rule is None or barcodes is None:
        return False
    if rule.n_records == 0 or rule.pairs > 1 or (rule.pairs and rule.first_record % 2) or (rule.split_mates and not rule.pairs):
        return False
    p0, p1 = rule.part[0], rule.part[1]
    if p0.len == 0:
        return False
    for p in (p0, p1):
        if p.len == 0:
            continue
        if p.src not in (HEADER, BASES) or p.mate > 1 or (p.mate and not rule.pairs) or p.sub > 1 or (p.sub and p.src == BASES):
            return False
        if p.pos + p.len >= 2 ** 32:
            return False
    B = p0.len + p1.len
    if not 1 <= B <= 32 or rule.max_mm > B or not 1 <= rule.n_samples <= 4096:
        return False
    rows = [bytes(b) for b in barcodes]
    if len(rows) != rule.n_samples or any(len(r) != B or any(c not in ACGT for c in r) for r in rows):
        return False
    return len(set(rows)) == len(rows)


def observed(part, unit):
    """the part's observed bytes in the unit (a list of records), None where the part is short"""
    rec = unit[part.mate]
    if part.src == HEADER:
        colon = rec[0].rfind(b":")
        if colon < 0:
            return None
        F = rec[0][colon + 1:]
        plus = F.find(b"+")
        if part.sub == 0:
            sub = F if plus < 0 else F[:plus]
        elif plus < 0:
            return None
        else:
            sub = F[plus + 1:]
    else:
        sub = rec[1]
    if len(sub) < part.pos + part.len:
        return None
    return sub[part.pos:part.pos + part.len]


def distance(obs, barcode):
    """an observed byte matches a barcode base where it is that letter in either case; N, '.', anything else mismatches"""
    return sum(1 for o, b in zip(obs, barcode) if bytes([o]).upper() != bytes([b]))


def verdict(obs, barcodes, max_mm, memo=None):
    """'far', 'ambiguous' or (sample, distance)"""
    if memo is not None and obs in memo:
        return memo[obs]
    up = obs.upper()                                                    # (distance(obs, b), a barcode being upper case)
    ds = [sum(map(ne, up, b)) for b in barcodes]
    m = min(ds)
    v = "far" if m > max_mm else "ambiguous" if ds.count(m) > 1 else (ds.index(m), m)
    if memo is not None:
        memo[obs] = v
    return v


def clip_of(rule, mate):
    """c_R of the unit's record mate"""
    if not rule.clip:
        return 0
    return max([p.pos + p.len for p in (rule.part[0], rule.part[1]) if p.len and p.src == BASES and p.mate == mate], default=0)


def demux(fq, rule, barcodes, out_cap=None):
    """(parts, part_units, counts): parts = NP byte strings, part_units = n_samples + 1 numbers, counts = a dict of the report's fields"""
    if len(fq) == 0 or not check(rule, barcodes):
        raise Refused(E_ARG, "the arguments")
    ls = lines(fq)
    if len(ls) % 4:
        raise Refused(E_FORMAT, "lines")
    if not fq.endswith(b"\n"):
        raise Refused(E_FORMAT, "no final line end")
    rs = records(fq)
    r0 = rule.first_record
    if rule.n_records == TO_END:
        if r0 >= len(rs):
            raise Refused(E_ARG, "the range")
        nr = len(rs) - r0
    else:
        nr = rule.n_records
        if r0 + nr > len(rs):
            raise Refused(E_ARG, "the range")
    G = 2 if rule.pairs else 1
    if nr % G:
        raise Refused(E_FORMAT, "an odd count")
    if rule.clip:
        at = 0
        offs = []
        for r in rs:
            offs.append(at)
            at += len(text_of(r))
        for r in range(r0, r0 + nr):
            if len(rs[r][1]) != len(rs[r][3]):
                raise Refused(E_FORMAT, "unequal lines", record=r, offset=offs[r])
    ns = rule.n_samples
    rows = [bytes(b) for b in barcodes]
    parts = [p for p in (rule.part[0], rule.part[1]) if p.len]
    NP = (2 if rule.split_mates else 1) * (ns + 1)
    out = [[] for _ in range(NP)]
    units = [0] * (ns + 1)
    c = dict(n_in_range=nr, n_units=nr // G, n_assigned=0, n_perfect=0, n_short=0, n_far=0, n_ambiguous=0, text_bytes=len(fq), bases_clipped=0)
    memo = {}
    for u in range(nr // G):
        unit = rs[r0 + u * G:r0 + u * G + G]
        obs = [observed(p, unit) for p in parts]
        if any(o is None for o in obs):
            v = "short"
        else:
            v = verdict(b"".join(obs), rows, rule.max_mm, memo)
        if isinstance(v, tuple):
            s = v[0]
            c["n_assigned"] += 1
            c["n_perfect"] += v[1] == 0
        else:
            s = ns
            c["n_" + v] += 1
        units[s] += 1
        for g, rec in enumerate(unit):
            if s < ns:
                k = clip_of(rule, g)
                c["bases_clipped"] += k
                rec = [rec[0], rec[1][k:], rec[2], rec[3][k:]]
            out[2 * s + g if rule.split_mates else s].append(text_of(rec))
    parts_bytes = [b"".join(p) for p in out]
    c["out_bytes"] = sum(len(p) for p in parts_bytes)
    if out_cap is not None and c["out_bytes"] > out_cap:
        e = Refused(E_OVERFLOW, "room")
        e.needed = c["out_bytes"]
        raise e
    return parts_bytes, units, c

"""Times the demux pass alone (sfq_demux_records, dmx.hip) on the benchmark's text (kind 0, 10 M reads of 150 bases)
resident on the device, beside sfq_select_records with max_n on and a stateless sfq_dedup_records on the same text, all calls
alternating in one process: one warm-up of each, then ROUNDS rounds, host clocks around calls that end in a synchronise; medians and
ranges.

    python profiles/demux_pass.py                        # the three cases, each in a child process under its own time limit
    python profiles/demux_pass.py --case hdr             # (a) the header's field, 96 samples of 6 bases, one of them the text's own
                                                         #     ATCACG: every unit lands in one class, the degenerate partition
    python profiles/demux_pass.py --case inline          # (b) the reads' first 6 bases, 96 random samples, mm=1: every class is
                                                         #     populated, about half of the units are unassigned
    python profiles/demux_pass.py --case inline4096      # (c) the first 12 bases, 4096 random samples: two digit passes
    ... --reads N --rounds N --out FILE.json

For the kernels' own times run ONE case under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/demux_pass.py --case inline --rounds 3"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"hdr": dict(samples=96, B=6, limit=600), "inline": dict(samples=96, B=6, limit=600), "inline4096": dict(samples=4096, B=12, limit=600)}


def device_text(capi, torch, reads, seed=1, step=250_000):
    """the synthetic text on the device, built in pieces; returns (tensor, bytes)"""
    parts, n = [], 0
    for first in range(0, reads, step):
        piece = capi.synth_fastq(min(step, reads - first), 150, seed=seed, kind=0, first_read=first)
        parts.append(torch.frombuffer(bytearray(piece), dtype=torch.uint8).cuda())
        n += len(piece)
    t = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    at = 0
    for p in parts:
        t[at:at + p.numel()] = p
        at += p.numel()
    del parts
    return t, n


def run_case(case, reads, rounds, out_path):
    import numpy as np
    import torch
    from slimfastq_amd import capi
    from slimfastq_amd.capi import Dedup, Demux, DemuxPart, Select, DEMUX_HEADER, DEMUX_BASES

    text, n = device_text(capi, torch, reads)
    out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    ns, B = CASES[case]["samples"], CASES[case]["B"]
    rng = np.random.default_rng(96)
    ids = rng.choice(4 ** B, ns, replace=False)
    rows = [bytes(b"ACGT"[(int(v) >> (2 * i)) & 3] for i in range(B)) for v in ids]
    if case == "hdr":
        if b"ATCACG" not in rows:
            rows[17] = b"ATCACG"
        rule = Demux([DemuxPart(DEMUX_HEADER, 0, 0, 0, B)], n_samples=ns, max_mm=1)
    else:
        rule = Demux([DemuxPart(DEMUX_BASES, 0, 0, 0, B)], n_samples=ns, max_mm=1)
    c = capi.Context(0)
    calls = {"demux/" + case: lambda: c.demux_records(text.data_ptr(), n, rule, rows, out.data_ptr(), n),
             "select/max_n": lambda: c.select_records(text.data_ptr(), n, Select(max_n=2), out.data_ptr(), n),
             "dedup/stateless": lambda: c.dedup_records(text.data_ptr(), n, Dedup(), out.data_ptr(), n)}
    found, times = {}, {name: [] for name in calls}
    for name, f in calls.items():                                      # the warm-up: working buffers are reserved here
        res = f()
        rep = res[-1]
        found[name] = {fld: int(getattr(rep, fld)) for fld, _ in rep._fields_ if not hasattr(getattr(rep, fld), "__len__")}
        if name.startswith("demux/"):
            units = res[2]
            found[name]["parts_with_units"] = sum(1 for u in units[:ns] if u)
            found[name]["largest_sample"] = max(units[:ns])
            found[name]["unassigned"] = units[ns]
    for _ in range(rounds):
        for name, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[name].append((time.perf_counter() - t0) * 1e3)
    result = {"case": case, "reads": reads, "text_bytes": n, "samples": ns, "barcode_bases": B, "max_mm": 1, "rounds": rounds, "found": found,
              "ms": {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for name, v in times.items()}}
    for name, v in result["ms"].items():
        print("%-12s %-18s %9.3f ms  (%.3f .. %.3f)" % (case, name, v["median"], v["min"], v["max"]), flush=True)
    print(json.dumps(found["demux/" + case]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.reads, a.rounds, a.out)
        return 0
    for case, c in CASES.items():                                      # every GPU step under a time limit of its own; the first that fails ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--rounds", str(a.rounds), "--reads", str(a.reads)]
        if a.out:
            cmd += ["--out", "%s.%s.json" % (a.out.rsplit(".json", 1)[0], case)]
        try:
            rc = subprocess.run(cmd, timeout=c["limit"]).returncode
        except subprocess.TimeoutExpired:
            print("%s: ended at its time limit of %d s" % (case, c["limit"]), file=sys.stderr)
            return 124
        if rc:
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Times the screen pass alone (sfq_screen_records, scr.hip) on a text that is resident on the device, beside
sfq_select_records with max_n on and a stateless sfq_dedup_records on the same text, all calls alternating in one process: one
warm-up of each, then ROUNDS rounds, host clocks around calls that end in a synchronise; medians and ranges.

    python profiles/screen_pass.py                       # both cases, each in a child process under its own time limit
    python profiles/screen_pass.py --case phix           # the benchmark's text (kind 0, 10 M reads of 150 bases) against the k-mers of a
                                                         #   random sequence of 5 386 bases: nothing matches, the table stays in the cache
    python profiles/screen_pass.py --case hits           # kind 3, 2 M reads, against the k-mers of its first 100 000 reads' bases: many
                                                         #   hits, a table of hundreds of MB
    ... --reads N --rounds N --lanes 8,4,16,1 --out FILE.json

THE LAYOUT SWITCH: k_scr_count shares a record among 8 lanes; the environment variable SFQ_SCR_LANES (1, 4, 8 or 16), read when a
set is created, chooses another number, with the same results.  --lanes names the layouts to time: the script makes a context and a
set per layout, so that all of them alternate inside the rounds.  For the kernels' own times run ONE case under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/screen_pass.py --case hits --rounds 3"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"phix": dict(kind=0, reads=10_000_000, limit=900), "hits": dict(kind=3, reads=2_000_000, limit=600)}
K = 27


def device_text(capi, torch, kind, reads, seed=1, step=250_000):
    """the synthetic text on the device, built in pieces; returns (tensor, bytes, the first 100 000 reads' text)"""
    parts, head, n = [], b"", 0
    for first in range(0, reads, step):
        piece = capi.synth_fastq(min(step, reads - first), 150, seed=seed, kind=kind, first_read=first)
        if first < 100_000:
            head += piece
        parts.append(torch.frombuffer(bytearray(piece), dtype=torch.uint8).cuda())
        n += len(piece)
    t = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    at = 0
    for p in parts:
        t[at:at + p.numel()] = p
        at += p.numel()
    del parts
    return t, n, head


def run_case(case, reads, rounds, lanes, out_path):
    import numpy as np
    import torch
    from slimfastq_amd import capi
    from slimfastq_amd.capi import Dedup, Screen, Select

    kind = CASES[case]["kind"]
    text, n, head = device_text(capi, torch, kind, reads)
    out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    if case == "phix":
        rng = np.random.default_rng(5386)
        ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 5386)].tobytes()
    else:
        ref = b"\n".join(head.split(b"\n")[1:4 * min(reads, 100_000):4])
    ctxs = {}
    for g in lanes:
        os.environ["SFQ_SCR_LANES"] = str(g)
        c = capi.Context(0)
        c.screen_set_create(K, max(len(ref), 1))
        c.screen_set_add(ref)
        ctxs[g] = c
    os.environ.pop("SFQ_SCR_LANES", None)
    main = ctxs[lanes[0]]
    calls = {"screen/lanes%d" % g: (lambda c=c: c.screen_records(text.data_ptr(), n, Screen(), out.data_ptr(), n)) for g, c in ctxs.items()}
    calls["select/max_n"] = lambda: main.select_records(text.data_ptr(), n, Select(max_n=2), out.data_ptr(), n)
    calls["dedup/stateless"] = lambda: main.dedup_records(text.data_ptr(), n, Dedup(), out.data_ptr(), n)
    found, times = {}, {name: [] for name in calls}
    for name, f in calls.items():                                      # the warm-up: working buffers are reserved here
        got, rep = f()
        found[name] = {fld: int(getattr(rep, fld)) for fld, _ in rep._fields_ if not hasattr(getattr(rep, fld), "__len__")}
        found[name]["out_bytes"] = int(got)
    same = {json.dumps(v, sort_keys=True) for k, v in found.items() if k.startswith("screen/")}
    assert len(same) == 1, "the layouts disagree: %s" % found
    for _ in range(rounds):
        for name, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[name].append((time.perf_counter() - t0) * 1e3)
    result = {"case": case, "kind": kind, "reads": reads, "text_bytes": n, "k": K, "reference_bytes": len(ref),
              "set": dict(zip(("k", "kmers", "max_kmers"), main.screen_set_info())), "rounds": rounds, "found": found,
              "ms": {name: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v} for name, v in times.items()}}
    for name, v in result["ms"].items():
        print("%-10s %-18s %9.3f ms  (%.3f .. %.3f)" % (case, name, v["median"], v["min"], v["max"]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    for c in ctxs.values():
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reads", type=int)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--lanes", default="8,4,16,1")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.reads or CASES[a.case]["reads"], a.rounds, [int(x) for x in a.lanes.split(",")], a.out)
        return 0
    for case, c in CASES.items():                                      # every GPU step under a time limit of its own; the first that fails ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--case", case, "--rounds", str(a.rounds), "--lanes", a.lanes]
        if a.reads:
            cmd += ["--reads", str(a.reads)]
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

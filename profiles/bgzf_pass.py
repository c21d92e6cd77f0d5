"""Times the BGZF pass (sfq_bgzf_deflate, bgz.hip) on the benchmark's text (kind 0, 10 M reads of 150 bases): one
warm-up, then ROUNDS rounds, host clocks around calls that end in a synchronise; medians and ranges.

    python profiles/bgzf_pass.py                         # both cases, each in a child process under its own time limit
    python profiles/bgzf_pass.py --case deflate          # (a) sfq_bgzf_deflate alone on the text resident on the device: ms, GB/s of
                                                         #     text, and its deflate bytes against zlib level 1 on a 64 MB sample
    python profiles/bgzf_pass.py --case decode           # (b) sfq_decode_blocks_host with and without the switch, alternating
    ... --reads N --rounds N --out FILE.json

For the kernels' own times run ONE case under the profiler:
    rocprofv3 --kernel-trace --stats --output-format csv -- python profiles/bgzf_pass.py --case deflate --rounds 3"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from profiles.demux_pass import device_text      # noqa: E402

CASES = {"deflate": dict(limit=600), "decode": dict(limit=900)}
PIECE = 65280
SAMPLE = 64 << 20


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}


def run_deflate(reads, rounds):
    import torch
    from slimfastq_amd import capi
    text, n = device_text(capi, torch, reads)
    cap = capi.bgzf_bound(n, 1)
    out = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    c = capi.Context(0)
    off, rep = c.bgzf_deflate(text.data_ptr(), [0, n], out.data_ptr(), cap)          # the warm-up: buffers are reserved here
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.bgzf_deflate(text.data_ptr(), [0, n], out.data_ptr(), cap)
        ms.append((time.perf_counter() - t0) * 1e3)
    # the ratio on a sample: whole pieces from the text's start
    m = min(n, SAMPLE) // PIECE * PIECE
    sample = text[:m].cpu().numpy().tobytes()
    soff, srep = c.bgzf_deflate(text.data_ptr(), [0, m], out.data_ptr(), cap)
    ours = int(srep.out_bytes) - 26 * int(srep.members)
    theirs = 0
    for at in range(0, m, PIECE):
        z = zlib.compressobj(1, zlib.DEFLATED, -15)
        theirs += len(z.compress(sample[at:at + PIECE]) + z.flush())
    c.close()
    r = {"case": "deflate", "reads": reads, "text_bytes": n, "out_bytes": int(rep.out_bytes), "members": int(rep.members),
         "stored_members": int(rep.stored_members), "rounds": rounds, "ms": stats(ms), "gb_per_s_text": n / statistics.median(ms) / 1e6,
         "sample_bytes": m, "sample_deflate": ours, "sample_zlib1": theirs, "sample_ratio": ours / theirs if theirs else 0.0}
    print("deflate  %9.3f ms (%.3f .. %.3f)  %.2f GB/s of text, %d -> %d bytes; sample: %.4f of zlib level 1" % (
        r["ms"]["median"], r["ms"]["min"], r["ms"]["max"], r["gb_per_s_text"], n, r["out_bytes"], r["sample_ratio"]), flush=True)
    return r


def run_decode(reads, rounds):
    from slimfastq_amd import capi
    fq = capi.synth_fastq(reads, 150, seed=1, kind=0)
    c = capi.Context(0)
    enc = c.encode_host(fq, level=3, block_reads=4096, prior_step=capi.PRIOR_AUTO, tables=capi.TABLES_FROZEN)
    cap = len(fq) + 4096
    n = len(fq)
    del fq
    times = {"plain": [], "bgzf": []}
    sizes = {}
    for on in (False, True, False, True):                              # the warm-up of both
        c.set_bgzf(on)
        sizes["bgzf" if on else "plain"] = len(c.decode_host(enc, level=3, out_cap=cap))
    for _ in range(rounds):
        for name, on in (("plain", False), ("bgzf", True)):
            c.set_bgzf(on)
            t0 = time.perf_counter()
            c.decode_host(enc, level=3, out_cap=cap)
            times[name].append((time.perf_counter() - t0) * 1e3)
    c.set_bgzf(False)
    c.close()
    r = {"case": "decode", "reads": reads, "text_bytes": n, "returned_bytes": sizes, "rounds": rounds, "ms": {k: stats(v) for k, v in times.items()}}
    for k, v in r["ms"].items():
        print("decode   %-6s %9.3f ms (%.3f .. %.3f)  %d bytes returned" % (k, v["median"], v["min"], v["max"], sizes[k]), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.case:
        r = (run_deflate if a.case == "deflate" else run_decode)(a.reads, a.rounds)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(r, f, indent=1)
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

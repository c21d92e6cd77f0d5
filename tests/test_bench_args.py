"""bench.py's argument handling (no GPU): defaults per workload kind, workload names, what a plain run leaves to --full,
and what --dump-outputs writes."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def parse(mod, argv):
    old = sys.argv
    sys.argv = ["bench.py"] + argv
    try:
        return mod.parse()
    finally:
        sys.argv = old


def test_defaults_follow_the_workload_kind():
    b = load_bench()
    a = parse(b, [])
    assert (a.gpus, a.reads, a.read_len, a.level, a.block_reads, a.kind) == (1, 10_000_000, 150, 3, 1024, 0)
    assert a.tables == 1
    assert b.workload_name(a) == "synthetic 10M x 150 bp Illumina reads per GPU, full qlts+gens+recs, frozen tables (one chain per lane), -l 3"
    assert "adaptive tables" in b.workload_name(parse(b, ["--tables", "0"]))
    a = parse(b, ["--kind", "1"])
    assert a.reads == 60_000 and a.block_reads == b.capi.BLOCK_AUTO and a.cpu_sample_reads <= 6_000
    assert "long reads" in b.workload_name(a)
    a = parse(b, ["--workload", "qlt", "--reads", "2500000", "--block-reads", "512"])
    assert a.reads == 2_500_000 and a.block_reads == 512 and "qlts-only kernel" in b.workload_name(a)
    a = parse(b, ["--gpus", "8", "--steps", "5", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (8, 5, 2)


def test_a_plain_run_leaves_every_secondary_leg_to_full():
    b = load_bench()
    legs = ("no_decode", "no_adaptive_leg", "no_cpu_baseline", "no_format6_leg", "no_genome_leg", "no_host_leg", "no_size_sweep", "no_c4_leg")
    a = parse(b, ["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and all(getattr(a, k) for k in legs)
    a = parse(b, ["--full"])
    assert a.full and not any(getattr(a, k) for k in legs)
    a = parse(b, ["--full", "--no-decode"])
    assert a.no_decode and not a.no_size_sweep
    a = parse(b, ["--sweep-only"])
    assert a.full and not a.no_size_sweep and a.no_decode and a.no_cpu_baseline
    assert parse(b, ["--dump-outputs", "out"]).dump_outputs == "out"
    with pytest.raises(SystemExit):
        parse(b, ["--steps", "0"])


def test_dump_outputs_writes_float_arrays_within_64_mb(tmp_path):
    """dump_outputs on host stand-ins for the context and the output buffer: every file is float32 / float64, the byte
    values and counts come through exactly, the sample of a large output is seeded and sorted, and all of it stays under 64 MB."""
    import numpy as np
    import torch
    b = load_bench()
    capi = b.capi

    class Ctx:
        def index(self, n):
            blocks = (capi.BlockInfo * n)()
            for i in range(n):
                blocks[i].first_record, blocks[i].n_records, blocks[i].size[2] = 1024 * i, 1024, 7 + i
            return blocks

        def first_headers(self, n):
            return bytes(range(n))

        def prior(self):
            return b"\x01\x02\xff"

        def chains(self):
            return b""

        def rec_prior(self):
            return b"\x80" * 5

    res = capi.Result()
    res.n_records, res.n_blocks, res.first_hdr_bytes, res.n_chains = 3072, 3, 10, 12
    for total in (1000, b.DUMP_SAMPLE + 12345):
        res.total_bytes = total
        res.stream_bytes[0], res.stream_offset[1] = total, total
        out = torch.from_numpy((np.arange(total + 64) * 7 % 251).astype(np.uint8))
        d = tmp_path / str(total)
        b.dump_outputs(str(d), Ctx(), res, out)
        got = {p.stem: np.load(p) for p in d.iterdir()}
        assert sorted(got) == ["block_index", "chain_index", "first_headers", "qlt_prior", "rec_prior", "result", "stream_bytes",
                               "stream_offset", "streams_sample", "streams_sample_pos"]
        assert all(a.dtype in (np.float32, np.float64) for a in got.values())
        assert sum(a.nbytes for a in got.values()) <= 64 << 20
        assert got["result"].tolist() == [3072, 3, total, 10, 12]
        assert got["stream_bytes"][0] == total and got["stream_offset"][1] == total
        assert got["block_index"].shape == (3, 26) and got["block_index"][2, 0] == 2048 and got["block_index"][2, 10 + 2] == 9
        assert got["first_headers"].tolist() == list(range(10)) and got["qlt_prior"].tolist() == [1, 2, 255] and got["chain_index"].size == 0
        pos = got["streams_sample_pos"].astype(np.int64)
        assert len(pos) == min(total, b.DUMP_SAMPLE) and (np.diff(pos) >= 0).all() and pos[-1] < total
        assert np.array_equal(got["streams_sample"], out.numpy()[pos].astype(np.float32))
        again = tmp_path / ("again%d" % total)
        b.dump_outputs(str(again), Ctx(), res, out)
        assert np.array_equal(np.load(again / "streams_sample_pos.npy"), got["streams_sample_pos"])

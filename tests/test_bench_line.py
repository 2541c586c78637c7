"""The driver parses ONE stdout line of bench.py: it must stay short (round 5's 22 KB line was not parsed) and carry the contract's
keys plus `roofline` and `cpu_baseline`.  compact_line() is exercised on committed full result objects of earlier runs."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULLS = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_bench_full.json")))


@pytest.mark.parametrize("path", FULLS, ids=[os.path.basename(p) for p in FULLS])
def test_compact_line_is_short_and_complete(path):
    import bench
    full = json.load(open(path))
    if "metric" not in full:            # (2-rank dry-run logs hold other things)
        pytest.skip("not a bench result object")
    line = bench.compact_line(full, "bench_full.json")
    assert "\n" not in line and len(line) < bench.COMPACT_LIMIT
    o = json.loads(line)
    for k in bench.COMPACT_KEYS:
        assert k in o, k
    assert o["dtype"] == "f32" and o["data"] == "synthetic" and o["higher_is_better"] is True
    assert "workload" in o["config"] and "model" not in o["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms_avg"):
        assert k in o["roofline"], k
    assert abs(o["roofline"]["frac"] - o["roofline"]["achieved"] / o["roofline"]["peak"]) < 1e-3
    if full.get("cpu_baseline"):
        for k in ("value", "unit", "cores", "kind", "sample"):
            assert o["cpu_baseline"][k] is not None, k
    assert abs(o["value"] - full["value"]) <= 1e-6 * full["value"]
    # no prose: every string value is short
    def strings(x):
        if isinstance(x, dict):
            for v in x.values():
                yield from strings(v)
        elif isinstance(x, str):
            yield x
    assert max(len(s_) for s_ in strings(o)) <= 160


def test_compact_line_survives_oversized_extras():
    import bench
    full = json.load(open(FULLS[-1]))
    full["comm_error"] = "x" * 100000
    full["per_rank_users_per_s"] = [1.0] * 4096
    line = bench.compact_line(full, "bench_full.json")
    assert len(line) < bench.COMPACT_LIMIT
    assert json.loads(line)["value"]


def test_gpus_mismatch_with_launcher_world_is_refused():
    """`--gpus 4` under a launcher that started 2 ranks must not print a line labelled with either number."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr and r.stdout.strip() == ""


EXTRAS = ("cpu_users", "recall_users", "host_buffer_steps", "trained_recall_steps", "train", "small", "dr", "other_scorer", "diverse",
          "long_history", "jtm_full", "otm64")


def test_plain_run_times_the_headline_only_and_full_keeps_every_extra(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (3, 1, False, None)
    for k in EXTRAS:
        assert getattr(a, k) == 0, k
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    f = bench.parse()
    assert f.full and f.cpu_users == -1 and f.recall_users == 1024 and f.host_buffer_steps == 3 and f.trained_recall_steps == 6000
    for k in ("train", "small", "dr", "other_scorer", "diverse", "long_history", "jtm_full", "otm64"):
        assert getattr(f, k) == 1, k


def test_dump_outputs_writes_a_fixed_float_sample_of_the_step(tmp_path):
    """--dump-outputs: float32 / float64 .npy files, at most 64 MB, the same users on every run, values equal to the step's rows."""
    import bench

    class HostEngine:                   # d2h from "device" buffers that are host arrays here
        def d2h(self, host, dev):
            host[...] = dev

    U, topk = 40000, 200
    rng = np.random.default_rng(3)
    ids = rng.integers(-1, 10_000_000, (U, topk)).astype(np.int32)
    sc = rng.standard_normal((U, topk)).astype(np.float32)
    cnt = rng.integers(0, topk + 1, U).astype(np.int32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), HostEngine(), U, topk, ids, sc, cnt)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["counts.npy", "item_ids.npy", "scores.npy", "users.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 << 20
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert got[n].dtype in (np.float32, np.float64), n
        assert np.array_equal(got[n], np.load(tmp_path / "b" / n)), n
    users = got["users.npy"].astype(np.int64)
    assert users.size == bench.DUMP_USERS and np.unique(users).size == users.size
    assert np.array_equal(got["item_ids.npy"], ids[users]) and np.array_equal(got["scores.npy"], sc[users])
    assert np.array_equal(got["counts.npy"], cnt[users])

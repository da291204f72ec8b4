"""bench.py's plain run and its two options: a plain `bench.py --gpus N --steps K --warmup W` times the headline and nothing
else (the CPU baseline, side figures, scaling model and detail record run under `--full`), and `--dump-outputs DIR` writes what
the last timed step left a caller holding, in float32/float64, at most 64 MB, the same arrays in every run of the same arguments."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT

DUMP_LIMIT_BYTES = 64 << 20


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_a_plain_run_has_no_side_figures_and_full_keeps_them():
    bench = _bench()
    plain = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not plain.full and plain.steps == 7 and plain.warmup == 3 and plain.dump_outputs is None
    assert plain.no_cpu_baseline and plain.detail == "-"
    assert plain.actor_boards == plain.carved_pool == plain.chunk == plain.sustained == plain.shard_ranks == 0
    assert plain.no_config1 and plain.no_weak_job and plain.no_out_of_cache
    # side-figure options alone do not bring the figures back: only --full does
    assert bench.parse_args(["--chunk", "50", "--sustained", "100"]).chunk == 0
    full = bench.parse_args(["--full"])
    assert full.full and not full.no_cpu_baseline and full.detail is None
    assert (full.actor_boards, full.carved_pool, full.chunk, full.sustained, full.shard_ranks) == (262144, 65536, 50, 2000, 8)
    assert not (full.no_config1 or full.no_weak_job or full.no_out_of_cache)
    quiet = bench.parse_args(["--full", "--no-side-figures"])
    assert quiet.chunk == quiet.sustained == 0 and not quiet.no_cpu_baseline
    assert bench.parse_args(["--dump-outputs", "some/dir"]).dump_outputs == "some/dir"


class _FakeEnv:
    """What dump_outputs() reads from a BatchedTetris: packed_state() and stats(), here host tensors."""

    def __init__(self, n, seed):
        import torch
        g = torch.Generator().manual_seed(seed)
        self.state = {"rows": torch.randint(-32768, 32767, (n, 20), generator=g, dtype=torch.int16)}
        for k in ("cur", "nxt", "lines", "moves", "state", "pieces_left"):
            self.state[k] = torch.randint(0, 41, (n,), generator=g, dtype=torch.uint8)

    def packed_state(self):
        return self.state

    def stats(self):
        return {"episodes": 5, "lines": 7, "wins": 1, "topouts": 4}


def _dumped(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path)) if f.endswith(".npy")}


@pytest.mark.parametrize("n", [1000, (1 << 20) + 1000])
def test_dump_outputs_are_float_arrays_within_64_mb_and_a_fixed_sample_of_a_large_batch(tmp_path, n):
    import torch
    bench = _bench()
    env = _FakeEnv(n, seed=1)
    reward = torch.arange(n, dtype=torch.float32) * 0.5
    done = (torch.arange(n) % 3 == 0).to(torch.uint8)
    bench.dump_outputs(str(tmp_path / "a"), env, reward, done, -0.25)
    bench.dump_outputs(str(tmp_path / "b"), env, reward, done, -0.25)
    a, b = _dumped(tmp_path / "a"), _dumped(tmp_path / "b")
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)                     # the same arrays every time
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= DUMP_LIMIT_BYTES
    assert {"reward", "done", "rows", "cur", "nxt", "lines", "moves", "state", "pieces_left", "stats", "mean_episodic_return"} <= set(a)
    assert a["stats"].tolist() == [5, 7, 1, 4] and a["mean_episodic_return"].tolist() == [-0.25]
    rows = env.state["rows"].numpy().view(np.uint16)
    if n <= bench.DUMP_BOARDS:
        assert "board_index" not in a and np.array_equal(a["reward"], reward.numpy()) and np.array_equal(a["done"], done.numpy())
    else:
        idx = a["board_index"].astype(np.int64)
        assert len(idx) == bench.DUMP_BOARDS and np.all(np.diff(idx) > 0) and idx[-1] < n
        assert np.array_equal(a["reward"], reward.numpy()[idx]) and np.array_equal(a["lines"], env.state["lines"].numpy()[idx])
    ridx = a["rows_index"].astype(np.int64) if "rows_index" in a else np.arange(n)
    assert len(ridx) == min(n, bench.DUMP_ROWS_BOARDS) and np.array_equal(a["rows"], rows[ridx].astype(np.float32))


def _plain_bench(extra, boards=65536):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--boards", str(boards), *extra]
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "TPL_BENCH_BACKEND", "TPL_BENCH_ONE_GPU", "TPL_BENCH_FORCE_DIST"):
        env.pop(k, None)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lines = res.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_dumps_what_the_oracle_computes_in_either_launch_mode(oracle):
    """A plain run of 65,536 boards, 5 + 20 steps: the line carries the headline and no side figure, and the dumped outputs of
    the last timed step are the oracle's after the same 25 steps -- in eager mode and with the K steps replayed as a graph."""
    L, M, n, seed, steps = 10, 40, 65536, 0, 25
    with tempfile.TemporaryDirectory() as tmp:
        eager_dir, graph_dir = os.path.join(tmp, "eager"), os.path.join(tmp, "graph")
        line = _plain_bench(["--dump-outputs", eager_dir])
        graph_line = _plain_bench(["--dump-outputs", graph_dir, "--launch-mode", "graph"])
        got, graph = _dumped(eager_dir), _dumped(graph_dir)
        size = sum(os.path.getsize(os.path.join(eager_dir, f)) for f in os.listdir(eager_dir))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 20 and line["warmup"] == 5 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert "cpu_baseline" not in line and "scaling_model" not in line and line["side"] == {} and line["detail"] is None
    assert line["config"]["launch_mode"] == "eager" and graph_line["config"]["launch_mode"] == "graph"
    assert size <= DUMP_LIMIT_BYTES and all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert set(got) == set(graph) and all(np.array_equal(got[k], graph[k], equal_nan=True) for k in got), \
        [k for k in got if not np.array_equal(got[k], graph[k], equal_nan=True)]

    cpu = oracle.Env(n, L, M, 0, seed)
    cpu.set_pool(oracle.synth_boards(seed, 0, n, L), oracle.synth_pieces(seed, 0, n, M))
    cpu.set_options(auto_reset=True, assign_mode=0)
    cpu.reset()
    for t in range(steps):
        r, d = cpu.step(oracle.synth_actions(seed, 0, n, t))
    assert np.array_equal(got["reward"], r.astype(np.float32)) and np.array_equal(got["done"], d.astype(np.float32))
    want = cpu.get_state()
    for k in ("cur", "nxt", "lines", "moves", "state", "pieces_left"):
        if k in want:
            assert np.array_equal(got[k], want[k].astype(np.float32)), k
    assert np.array_equal(got["rows"], want["rows"].view(np.uint16).astype(np.float32))
    st = cpu.stats()
    assert got["stats"].tolist() == [st[k] for k in ("episodes", "lines", "wins", "topouts")] and st["episodes"] > 0
    assert got["mean_episodic_return"][0] == line["mean_episodic_return"]

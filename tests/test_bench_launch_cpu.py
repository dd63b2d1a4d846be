"""`python bench.py --gpus N` must be launchable as the driver calls it: without
torch.distributed.run around it, the script re-executes itself as N ranks on 127.0.0.1 and prints ONE JSON
line from rank 0.  Run here end to end on CPU: T4R_BENCH_STUB=1 swaps the HIP model for bench._StubModel
(same gradient plumbing: tied table + row-sparse sink + head-backward hook) and RCCL for gloo; the launcher,
`setup`/`make_train_step`/`timed_region` and the JSON contract are bench.py's own code."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(argv, extra_env=None):
    env = os.environ.copy()
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(T4R_BENCH_STUB="1", OMP_NUM_THREADS="1")
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True,
                          text=True, timeout=300)


def _json_lines(stdout):
    return [json.loads(l) for l in stdout.splitlines() if l.startswith("{")]


def test_bench_self_launches_two_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, r.stdout                      # rank 0 only
    res = lines[0]
    assert res["stub"] is True and res["n_gpus"] == 2 and res["steps"] == 3 and res["warmup"] == 1
    assert res["config"]["global_batch"] == 32 and res["config"]["parallelism"] == "dp2"
    assert res["scaling"] == "weak" and res["higher_is_better"] is True and res["value"] > 0
    assert res["config"]["label_rows"] == 3 * 16 * 5


def test_bench_picks_the_faster_table_exchange_on_the_fabric_it_runs_on():
    """VERDICT r3 next #10 (first-contact safety of the N > 1 run): by default both forms of the table-gradient exchange are
    timed (MAX over ranks, so the ranks agree), the faster is kept, both times are reported, and the world size is in the line"""
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    (res,) = _json_lines(r.stdout)
    assert res["config"]["world_size"] == 2 and res["config"]["table_exchange"] in ("sparse", "dense")
    ms = res["comm"]["table_exchange_ms_per_step"]
    assert set(ms) == {"sparse", "dense"} and all(v > 0 for v in ms.values())
    assert res["config"]["table_exchange"] == min(ms, key=ms.get)
    assert res["ms_per_step_windows"]["n_windows"] == 2 and res["ms_per_step_windows"]["min"] <= res["ms_per_step_windows"]["median"]
    # an explicit choice is honoured
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1"], {"T4R_BENCH_TABLE_EXCHANGE": "dense"})
    assert r.returncode == 0, r.stderr[-2000:]
    (res,) = _json_lines(r.stdout)
    assert res["config"]["table_exchange"] == "dense" and res["comm"]["table_exchange_ms_per_step"] is None


def test_bench_single_rank_needs_no_launcher():
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    (res,) = _json_lines(r.stdout)
    assert res["n_gpus"] == 1 and res["config"]["parallelism"] == "dp1"


def test_bench_rejects_a_launcher_world_size_mismatch():
    r = _run(["--gpus", "4", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_bench_plain_run_is_lean_and_full_adds_the_windows():
    """a plain run times exactly --steps steps and prints the headline only; --full adds the extra timed windows"""
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    (res,) = _json_lines(r.stdout)
    assert res["full"] is False and "ms_per_step_windows" not in res
    assert res["steps"] == 3 and res["config"]["label_rows"] == 3 * 16 * 5 and res["ms_per_step"] > 0
    r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    (res,) = _json_lines(r.stdout)
    assert res["full"] is True and res["ms_per_step_windows"]["n_windows"] == 2


def test_bench_dump_outputs_are_reproducible(tmp_path):
    """--dump-outputs DIR: the last timed step's outputs as float .npy files; the same arguments give the same inputs, so
    two runs dump the same arrays"""
    import numpy as np

    dumps = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-2000:]
        (res,) = _json_lines(r.stdout)
        files = sorted(p.name for p in d.iterdir())
        assert {"loss.npy", "labels.npy", "params0.npy", "params1.npy"} <= set(files), files
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert abs(float(arrays["loss.npy"][0]) - res["config"]["final_loss"]) < 1e-4
        assert arrays["labels.npy"].shape == (16 * 5,)
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for f in dumps[0]:
        np.testing.assert_array_equal(dumps[0][f], dumps[1][f])

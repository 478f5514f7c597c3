"""bench.py contract: runs under torch.distributed.run exactly as the
driver launches it, emits one valid JSON line from rank 0."""

import json
import subprocess
import sys

from tests.internal.multi_process import find_free_port


def test_bench_distributed_cpu():
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--standalone", "--local-addr",
         "127.0.0.1", "bench.py", "--gpus", "2", "--steps", "3",
         "--warmup", "1", "--model", "mnist", "--batch-size", "8",
         "--dtype", "fp32"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    json_lines = [ln for ln in out.stdout.splitlines()
                  if ln.startswith("{")]
    assert len(json_lines) == 1, out.stdout
    rec = json.loads(json_lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in rec, "missing %s" % key
    assert rec["n_gpus"] == 2
    assert rec["steps"] == 3
    assert rec["data"] == "synthetic"
    assert rec["value"] > 0


def _run_single(tmp_path, *extra):
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--model", "mnist", "--batch-size", "4", "--dtype", "fp32",
         *extra],
        capture_output=True, text=True, timeout=240,
        env={"PATH": "/usr/bin:/bin:/usr/local/bin",
             "PYTHONPATH": ".",
             "MASTER_PORT": str(find_free_port()), "HOME": str(tmp_path)})
    assert out.returncode == 0, out.stderr[-3000:]
    json_lines = [ln for ln in out.stdout.splitlines()
                  if ln.startswith("{")]
    assert len(json_lines) == 1, out.stdout
    return json.loads(json_lines[0])


def test_bench_single_process_cpu(tmp_path):
    rec = _run_single(tmp_path)
    assert rec["n_gpus"] == 1


def _expected_dump(out_dir, warmup, steps):
    """What bench.py's mnist CPU path computes, redone here with plain
    torch (world 1: the gradient allreduce is the identity): same seed,
    model, batch and optimizer, `warmup` steps, then back to the seeded
    state (fresh momentum) and `steps` steps, as a dumping run does when
    it has fewer timed steps than its reproducible window."""
    import copy

    import torch
    import torch.nn.functional as F

    import bench
    from bagua_amd.models import create_model

    assert steps <= bench.DUMP_WINDOW_STEPS
    torch.manual_seed(42)
    model = create_model("mnist")
    seed_state = copy.deepcopy(model.state_dict())
    data = torch.randn(4, 1, 28, 28)
    target = torch.randint(0, 10, (4,))

    def run(n):
        opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9)
        for _ in range(n):
            opt.zero_grad()
            out = model(data)
            loss = F.nll_loss(out, target)
            loss.backward()
            opt.step()
        return {"output": out.detach(), "loss": loss.detach()}

    run(warmup)  # consumes the same random numbers (dropout) as warmup
    model.load_state_dict(seed_state)
    last = run(steps)
    bench.dump_outputs(str(out_dir), last, model)
    return seed_state


def _load(d):
    import numpy as np

    return {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}


def test_bench_dump_outputs_and_full_cpu(tmp_path):
    """--dump-outputs writes what the last timed step computed, as float32
    .npy files, identical from run to run; --full is accepted and keeps
    the result line's contract."""
    import numpy as np

    dumps = []
    for name, extra in (("a", ()), ("b", ("--full",))):
        d = tmp_path / name
        rec = _run_single(tmp_path, "--dump-outputs", str(d), *extra)
        assert rec["steps"] == 2
        assert rec["ms_per_step"] > 0
        assert rec["dtype"] == "fp32"
        dumps.append(_load(d))
    a, b = dumps
    assert set(a) == {"loss", "output", "params_sample"}
    assert a["output"].shape == (4, 10)
    assert a["loss"].shape == ()
    total = 0
    for k, arr in a.items():
        assert arr.dtype == np.float32, k
        assert np.isfinite(arr).all(), k
        total += arr.nbytes
        # CPU fp32 math on seeded inputs: bit-identical between runs
        np.testing.assert_array_equal(arr, b[k])
    assert total <= 64 * 2 ** 20

    # the values are those of the step: 1 warmup + 2 timed steps redone
    # with plain torch (fp32 sums in another order: a few ulp)
    seed_state = _expected_dump(tmp_path / "want", warmup=1, steps=2)
    want = _load(tmp_path / "want")
    for k in a:
        np.testing.assert_allclose(a[k], want[k], rtol=1e-4, atol=1e-6,
                                   err_msg=k)
    # ... and not those of the seed state or of a shorter run
    _expected_dump(tmp_path / "one", warmup=1, steps=1)
    one = _load(tmp_path / "one")
    assert np.abs(a["params_sample"] - one["params_sample"]).max() > 1e-5
    assert abs(float(a["loss"]) - float(one["loss"])) > 1e-5
    n_seed = sum(v.numel() for k, v in seed_state.items())
    assert n_seed >= a["params_sample"].size


def test_bench_refuses_dump_with_hip_graph_before_any_work(tmp_path):
    out = subprocess.run(
        [sys.executable, "bench.py", "--hip-graph", "--dump-outputs",
         str(tmp_path / "d"), "--model", "mnist"],
        capture_output=True, text=True, timeout=120,
        env={"PATH": "/usr/bin:/bin:/usr/local/bin", "PYTHONPATH": ".",
             "MASTER_PORT": "1", "HOME": str(tmp_path)})
    assert out.returncode != 0
    assert "--dump-outputs is not supported with --hip-graph" in out.stderr
    # refused in argument handling: no rendezvous on the unusable port,
    # no result line, nothing written
    assert "{" not in out.stdout
    assert not (tmp_path / "d").exists()


def test_tune_child_env_leaves_the_launchers_gang():
    """The tuning child must not inherit what ties a worker to its
    launcher: rank variables, the master port, and above all the elastic
    agent's store, on which it would wait out the whole group timeout."""
    import bench

    launcher = {
        "PATH": "/usr/bin", "HOME": "/h", "MIOPEN_USER_DB_PATH": "/db",
        "RANK": "3", "LOCAL_RANK": "3", "WORLD_SIZE": "8",
        "LOCAL_WORLD_SIZE": "8", "GROUP_RANK": "0", "NODE_RANK": "0",
        "ROLE_RANK": "3", "ROLE_WORLD_SIZE": "8", "MASTER_PORT": "29400",
        "MASTER_ADDR": "10.0.0.1", "TORCHELASTIC_USE_AGENT_STORE": "True",
        "TORCHELASTIC_RESTART_COUNT": "2", "TORCHELASTIC_MAX_RESTARTS": "5",
        "TORCHELASTIC_RUN_ID": "x", "BAGUA_PG_TIMEOUT_S": "1800",
    }
    env = bench.tune_child_env(launcher)
    assert not [k for k in env if k.startswith("TORCHELASTIC_")]
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE",
              "GROUP_RANK", "NODE_RANK", "ROLE_RANK", "MASTER_PORT"):
        assert k not in env, k
    assert env["MASTER_ADDR"] == "127.0.0.1"
    assert int(env["BAGUA_PG_TIMEOUT_S"]) < bench.TUNE_TIMEOUT_S
    # what the child needs to find the same caches stays
    assert env["HOME"] == "/h" and env["MIOPEN_USER_DB_PATH"] == "/db"
    assert launcher["RANK"] == "3"  # the caller's mapping is untouched


def test_tuned_marker_needs_the_find_db(tmp_path, monkeypatch):
    """A recorded tuning run counts only while MIOpen's user find-db is
    there and in use."""
    import bench

    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(tmp_path))
    monkeypatch.delenv("MIOPEN_DEBUG_DISABLE_FIND_DB", raising=False)
    assert not bench.is_tuned("k1")
    bench.record_tuned_key("k1")
    bench.record_tuned_key("k1")
    assert bench.load_tuned_keys() == ["k1"]
    assert not bench.is_tuned("k1")  # marker alone is not enough
    (tmp_path / "gfx950100.HIP.3_5_0.ufdb.txt").write_text("x")
    assert bench.is_tuned("k1")
    assert not bench.is_tuned("k2")
    monkeypatch.setenv("MIOPEN_DEBUG_DISABLE_FIND_DB", "1")
    assert not bench.is_tuned("k1")

"""Checks of what bench.py quotes: a PMC entry in profiles/hbm_traffic.json is evidence only for the kernel source
it was measured on, so the headline entry must carry the sha256 of the CURRENT csrc/mcq_hip.hip (tools/pmc_refresh.sh /
pmc_refresh.py write it); bench.py itself prints traffic: null for a stale entry.  What --dump-outputs writes (CPU), and a plain
run against a --full one on the GPU."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_headline_pmc_entry_matches_the_kernel_source():
    with open(os.path.join(ROOT, "profiles", "hbm_traffic.json")) as f:
        e = json.load(f)["board_N12_c65536_s100000"]
    assert e["kernel_sha256"] == bench.kernel_sha(), "profiles/hbm_traffic.json is stale: run tools/pmc_refresh.sh on the GPU box, then tools/pmc_refresh.py"
    assert e["bytes_per_launch"] == e["read_bytes"] + e["write_bytes"] > 0
    pmc, why = bench.measured_traffic("board_N12_c65536_s100000")
    assert pmc is not None and why is None


def test_stale_or_missing_entries_yield_null():
    pmc, why = bench.measured_traffic("no_such_workload")
    assert pmc is None and "no PMC entry" in why


def test_usable_cpus_is_positive():
    assert 1 <= bench.usable_cpus() <= (os.cpu_count() or 1)


def test_hardware_queues_are_raised_on_demand_only(monkeypatch):
    """Importing the package leaves GPU_MAX_HW_QUEUES alone (RCCL-only processes, single launches); an entry point that is about
    to run more than 4 streams raises it before the first GPU call, and never over the user's own value."""
    import mcq_amd

    monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
    assert mcq_amd._lib.ensure_hw_queues(1) is None and "GPU_MAX_HW_QUEUES" not in os.environ
    assert mcq_amd._lib.ensure_hw_queues(4) is None
    assert mcq_amd._lib.ensure_hw_queues(18) == "24" and os.environ["GPU_MAX_HW_QUEUES"] == "24"
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "8")
    assert mcq_amd._lib.ensure_hw_queues(18) == "8"
    with open(os.path.join(ROOT, "monte-carlo-collective_amd", "_lib.py")) as f:
        src = f.read()
    assert src.count('os.environ["GPU_MAX_HW_QUEUES"]') == 1  # only inside ensure_hw_queues


def test_per_rank_table_and_pmc_roofline_helpers():
    import torch

    t = bench.per_rank_table(torch, None, 0, 1, torch.device("cpu"), {"sweep_ms": 1.5, "reduce_ms": 0.25})
    assert t == {"reduce_ms": [0.25], "sweep_ms": [1.5]}
    line = {"roofline": {"traffic": None}}
    bench.roofline_from_pmc(line, None, "no PMC entry for x", 10.0, 0.0, 1)
    assert line["roofline"]["traffic"] is None and line["roofline"]["traffic_note"] == "no PMC entry for x"
    pmc = {"bytes_per_launch": 8e9, "valu_insts_per_launch": 2e9, "kernel_sha256": "x", "read_bytes": 5e9, "write_bytes": 3e9, "sweep_launches": 18}
    bench.roofline_from_pmc(line, pmc, None, 10.0, 0.0, 10**9)
    r = line["roofline"]
    assert r["traffic"] == 8e9 and abs(r["traffic_rate"] - 800.0) < 1e-9 and abs(r["valu_issue"]["achieved"] - 200.0) < 1e-9
    assert r["valu_issue"]["per_move"] == 2.0 and r["traffic_source"]["sweep_launches"] == 18 and "traffic_ratio" not in r


def _fake_run(n=48, n_steps=100, stride=104, words=2, seed=0):
    """A DeviceRun stand-in on the CPU: the output buffers of a c2 launch, padding included, two chains stopped early."""
    import types

    import numpy as np
    import torch

    rng = np.random.default_rng(seed)
    hist_len = np.full(n, n_steps + 1, dtype=np.int64)
    hist_len[[3, 17]] = [40, 7]
    t = {"energy_hist": torch.from_numpy(rng.integers(-50, 500, (n, stride)).astype(np.int32)),
         "accept_bits": torch.from_numpy(rng.integers(-2**63, 2**63 - 1, (n, words), dtype=np.int64)),
         "hist_len": torch.from_numpy(hist_len), "steps_executed": torch.from_numpy(hist_len - 1),
         "best_energy": torch.from_numpy(rng.integers(0, 90, n).astype(np.int32)),
         "stream_words": torch.from_numpy(rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)),
         "best_state": torch.from_numpy(rng.integers(0, 12, (n, 144)).astype(np.uint8))}
    return types.SimpleNamespace(t=t, p=types.SimpleNamespace(n_chains=n))


def _logical(run, n_steps):
    """What a caller of the path receives, computed directly: histories cut at hist_len, accept bits unpacked up to steps_executed."""
    import numpy as np

    t = {k: v.numpy() for k, v in run.t.items()}
    out = {k: v for k, v in t.items() if k not in ("energy_hist", "accept_bits")}
    out["stream_words"] = t["stream_words"].view(np.uint32)
    h = t["energy_hist"][:, : n_steps + 1].copy()
    for r, L in enumerate(t["hist_len"]):
        h[r, L:] = 0
    out["energy_hist"] = h
    bits = np.unpackbits(t["accept_bits"].view(np.uint8), axis=1, bitorder="little")[:, :n_steps]
    for r, s in enumerate(t["steps_executed"]):
        bits[r, s:] = 0
    out["accept_bits"] = bits
    return out


def test_dump_outputs_fits_its_budget_and_is_reproducible(tmp_path, monkeypatch):
    """--dump-outputs: float64 files whose values are the caller's arrays (whole, or at the stored flat indices of a seeded sample),
    under the byte budget, identical from run to run."""
    import numpy as np

    import mcq_amd

    monkeypatch.setattr(bench, "DUMP_BYTES", 60_000)
    n_steps = 100
    run = _fake_run(n_steps=n_steps)
    want = _logical(run, n_steps)
    for d in ("a", "b"):
        fields = bench.run_fields(run, n_steps, mcq_amd.abi)
        fields["summary"] = ((3,), lambda flat: np.array([25.0, float("nan"), 0.5])[flat])
        bench.dump_outputs(str(tmp_path / d), fields)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= bench.DUMP_BYTES
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True), f
    sampled = {f[: -len("_index.npy")] for f in names if f.endswith("_index.npy")}
    assert {"energy_hist", "accept_bits", "best_state"} <= sampled and "hist_len" not in sampled
    for k, v in want.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        if k in sampled:
            idx = np.load(tmp_path / "a" / f"{k}_index.npy").astype(np.int64)
            assert len(idx) == len(got) > 0 and np.all(np.diff(idx) > 0)
            np.testing.assert_array_equal(got, v.reshape(-1)[idx].astype(np.float64), err_msg=k)
        else:
            np.testing.assert_array_equal(got, v.astype(np.float64), err_msg=k)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "summary.npy"), [25.0, np.nan, 0.5])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_is_lean_and_full_run_adds_the_cpu_baseline(tmp_path):
    """A plain run prints the headline line and, with --dump-outputs, what its last timed step computed; --full adds the cpu_baseline
    leg (the oracle against the same chains) and computes the same outputs."""
    import subprocess

    import numpy as np

    def run(*extra):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--n-steps", "3000",
               "--chains", "4096", "--cpu-chains", "64"] + list(extra)
        out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout.strip().splitlines()[-1])

    plain = run("--dump-outputs", str(tmp_path / "plain"))
    full = run("--full", "--dump-outputs", str(tmp_path / "full"))
    for line in (plain, full):
        assert line["unit"] == "moves/s" and line["higher_is_better"] is True and line["dtype"] == "int32+f64"
        assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert "cpu_baseline" not in plain
    cb = full["cpu_baseline"]
    assert cb["sample_matches_gpu"] is True and cb["fast_port"]["sample_matches_gpu"] is True and cb["value"] > 0
    for k in ("min_energy", "mean_best_energy", "acceptance_rate"):
        assert plain[k] == full[k], k
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full"))
    assert {"energy_hist.npy", "accept_bits.npy", "best_energy.npy", "final_state.npy", "summary.npy"} <= set(names)
    assert sum(os.path.getsize(tmp_path / "plain" / f) for f in names) < 64 << 20
    for f in names:
        a, b = np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True), f
    sm = dict(zip(bench.SUMMARY_FIELDS, np.load(tmp_path / "plain" / "summary.npy")))
    assert sm["min_best"] == plain["min_energy"] and sm["n_chains"] == 4096 and sm["proposed"] == 4096 * 3000
    assert np.load(tmp_path / "plain" / "best_energy.npy").min() == plain["min_energy"]

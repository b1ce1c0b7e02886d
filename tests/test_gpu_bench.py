"""bench.py end to end on the GPU, as child processes (the way the driver
runs it), at small sizes:

* a plain N = 1 run: the headline line alone, and --dump-outputs checked
  against the oracle;
* --full, N = 2 under the gloo rehearsal backend (two ranks sharing cuda:0): the
  self-launch, the stripe-local headline with per-rank bytes (no CPU
  baseline: it is timed at N = 1 only), and the configs[3] gather leg -- survivors exchanged between the
  ranks on a communication stream, reconstructed through rs_reconstruct_ptrs
  and checked against locally re-encoded stripes over the last two timed
  steps (the step whose receive slots the next step reused, and the last);
* --full, N = 1 with rank 0's CPU baseline and the configs[0] (per-message latency, checked against the oracle
  inside the leg) and configs[4] (RS(64,16)) legs.

The driver's 8-GPU run uses RCCL instead of gloo; everything else is this
code."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.lstrip().startswith("{")]
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_two_ranks_gloo_with_gather_leg(torch_dev):
    d = _run(["--full", "--gpus", "2", "--stripes", "64", "--shard", "65536", "--steps", "2", "--warmup", "1",
              "--cpu-seconds", "0.5", "--gather-stripes", "16", "--gather-timeout", "150"],
             {"RSMI_BENCH_BACKEND": "gloo"})
    assert d["n_gpus"] == 2 and len(d["per_rank"]) == 2
    # value = the two ranks' own bytes over the slower rank's time
    secs = max(r["ms_per_step"] for r in d["per_rank"]) * d["steps"] / 1e3
    total = sum(r["bytes"] for r in d["per_rank"])
    assert abs(d["value"] - total / secs / 1e9) <= 0.01 * d["value"] + 0.02
    assert d["cpu_baseline"] is None  # timed at N = 1 only
    g = d["gather"]
    assert g["status"] == "ok", g
    assert g["backend"] == "gloo" and "gloo" in g["what"] and "RCCL (" not in g["what"]
    assert g["verified"]["mismatched_shards"] == 0 and g["verified"]["stripes"] >= 2
    assert g["verified"]["steps"] == [0, 1]
    assert g["xgmi"]["gathered_GB"] > 0
    assert "communication stream" in g["overlap"]
    assert "device_set" not in d  # N = 1 only


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_its_outputs(torch_dev, tmp_path):
    """A plain run times its steps and prints the line -- no leg beside the
    headline -- and --dump-outputs writes what the last timed step left in the
    buffers.  At this size (240 data and 96 parity shards of one window) the
    sample is the whole output, so it is checked byte for byte against the
    oracle on the inputs the arguments fix: the splitmix64 data (seed 0x5EED),
    its parity, and the shards the last step's erasure set (bench.py's
    generator and seed) names."""
    import numpy as np

    import bench
    from oracle import oracle
    k, n, S, stripes, steps, warmup = 10, 14, 4096, 24, 2, 1
    d = _run(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--stripes", str(stripes),
              "--shard", str(S), "--dump-outputs", str(tmp_path)])
    assert d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "GB/s" and d["dtype"] == "u8"
    assert d["higher_is_better"] is True and d["roofline"]["frac"] > 0
    assert d["cpu_baseline"] is None
    assert not {"config1", "config5", "config3_worst", "device_set", "gather"} & set(d)
    assert sorted(os.listdir(tmp_path)) == ["data.npy", "parity.npy", "reconstructed.npy"]
    got = {name: np.load(tmp_path / f"{name}.npy") for name in ("data", "parity", "reconstructed")}
    assert all(a.dtype == np.float32 for a in got.values())
    data = oracle.splitmix_bytes(stripes * k * S, 0x5EED)
    E = oracle.fec_matrix(k, n)
    parity = np.concatenate([np.frombuffer(oracle.encode(E, k, n, data[s * k * S:(s + 1) * k * S].tobytes()),
                                           dtype=np.uint8) for s in range(stripes)])
    data, parity = data.reshape(stripes, k, S), parity.reshape(stripes, n - k, S)
    assert np.array_equal(got["data"], data.reshape(-1, S).astype(np.float32))
    assert np.array_equal(got["parity"], parity.reshape(-1, S).astype(np.float32))
    e = bench.erasure_sets(np.random.default_rng(0xE4A5), warmup + steps, stripes, n, 1, n - k)[-1].astype(bool)
    want = np.concatenate([data[e[:, :k]], parity[e[:, k:]]]).astype(np.float32)
    assert np.array_equal(got["reconstructed"], want)


@pytest.mark.gpu
def test_bench_single_gpu_extra_legs(torch_dev):
    d = _run(["--full", "--stripes", "64", "--shard", "65536", "--steps", "2", "--warmup", "1", "--cpu-seconds", "0.2",
              "--config1-reps", "3", "--config5-stripes", "64", "--config5-steps", "2", "--config5-warmup", "1",
              "--config3-steps", "2", "--device-set-stripes", "24"])
    assert d["n_gpus"] == 1 and d["roofline"]["frac"] > 0
    assert d["cpu_baseline"] and d["cpu_baseline"]["value"] > 0
    c1 = d["config1"]
    assert c1["status"] == "ok", c1
    assert c1["message_bytes"] == 1048580 and len(c1["dropped"]) == 4
    assert c1["codec"]["encode_ms"] > 0 and c1["codec"]["decode4_ms"] > 0 and c1["codec"]["decode4_arena_ms"] > 0
    assert c1["codec"]["decode4_batch64_ms_per_message"] > 0
    assert c1["codec"]["encode_batch64_ms_per_message"] > 0 and c1["gpu_vs_1core"]["encode_batch64"] > 0
    assert set(c1["cpu_1t"]) == {"scalar_1t", "avx2_1t"}
    c5 = d["config5"]
    assert c5["status"] == "ok", c5
    assert c5["encode"]["GBps"] > 0 and c5["reconstruct"]["GBps"] > 0
    assert c5["encode"]["bytes"] == 64 * 80 * 65536
    c3 = d["config3_worst"]
    assert c3["status"] == "ok", c3
    assert c3["reconstruct"]["bytes"] == 64 * 14 * 65536 and c3["reconstruct"]["GBps"] > 0
    ds = d["device_set"]
    assert ds["status"] == "ok" and ds["checked"], ds
    assert ds["members"] == max(2, ds["members"]) and ds["stripes_per_member"] == 24
    assert ds["encode"]["GBps"] > 0 and ds["reconstruct"]["GBps"] > 0
    assert ds["spread"]["status"] == "ok" and ds["spread"]["GBps"] > 0, ds["spread"]

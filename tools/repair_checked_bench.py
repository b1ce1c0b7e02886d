#!/usr/bin/env python3
"""Cost of the checked repair (rs_reconstruct_checked) against the calls it fuses.

For BASELINE config 2 (6,553 stripes x RS(10,4) x 1 MiB shards) and config 5
(16,384 stripes x RS(64,16) x 64 KiB shards), for two erasure mixes -- `one`:
one erasure in every stripe; `mixed`: a fresh pattern of 1..m erasures per
stripe -- and for the strided layout and the pointer placement (a device table
that names the same slots), this times, in one process and on the same buffers,
  * fused:        the checked repair on a context that runs the repair kernel
                  (RSMI_REPAIR_FUSED=1),
  * split:        the checked repair on a context that queues the check and the
                  reconstruct launches (RSMI_REPAIR_FUSED=0),
  * two_calls:    rs_verify_degraded then rs_reconstruct_stripes on one stream
                  (rs_verify_ptrs, rs_reconstruct_ptrs), timed as one,
  * verify:       rs_verify_stripes of the intact image: the yardstick, the same
                  n * S bytes and k * m multiplies per column,
  * reconstruct:  rs_reconstruct_stripes alone.
Before the first call the first byte of every erased slot is made wrong; the
first checked repair must report every stripe clean and leave an image that
rs_verify_stripes finds clean, so the slots were written and never read.
HIP events around each arm on the caller's stream, --warmup untimed rounds,
then the median, minimum and maximum of --reps; the arms alternate inside one
loop so drift of the box hits all alike.  `enqueue_ms` is the host's time in
the call (planning, pattern lookup, staging), which the event time includes:
the stream is idle when the first event is recorded.  One JSON line per (config, mix,
placement), appended to --out when given.

    python tools/repair_checked_bench.py [--configs 2 5] [--mixes one mixed] [--placements strided ptrs]
                                         [--reps 10] [--out profiles/repair_checked/FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "noise-erasurecode-plugin_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = {2: (10, 14, 1 << 20, 6553), 5: (64, 80, 65536, 16384)}


def timed(stream, fn):
    """(ms between HIP events around the call, ms the host spent queueing it).
    The stream is idle when the first event is recorded, so the event time
    holds the host's planning and staging ahead of the first launch too."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), host


def context(k, n, fused):
    """A context whose checked repair takes the given route (read at rs_new)."""
    import rsmi

    old = os.environ.get("RSMI_REPAIR_FUSED")
    os.environ["RSMI_REPAIR_FUSED"] = "1" if fused else "0"
    try:
        return rsmi.FEC(k, n, device=0)
    finally:
        if old is None:
            del os.environ["RSMI_REPAIR_FUSED"]
        else:
            os.environ["RSMI_REPAIR_FUSED"] = old


def run_config(cfg, stripes, reps, warmup, want_mixes=("one", "mixed"), placements=("strided", "ptrs")):
    import rsmi

    k, n, S, default_stripes = CONFIGS[cfg]
    st = stripes or default_stripes
    m = n - k
    dev = torch.device("cuda", 0)
    plain = rsmi.FEC(k, n, device=0)
    f_fused, f_split = context(k, n, True), context(k, n, False)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    data = torch.empty(st * k * S, dtype=torch.uint8, device=dev)
    parity = torch.empty(st * m * S, dtype=torch.uint8, device=dev)
    first_bad = torch.zeros(st, dtype=torch.int32, device=dev)
    plain.fill_splitmix(data.data_ptr(), data.numel(), 0x5C2B, sh)
    geom = (data.data_ptr(), k * S, parity.data_ptr(), m * S, S, S, st)
    plain.encode_stripes(*geom, sh)
    addr = np.empty((st, n), dtype=np.int64)
    addr[:, :k] = data.data_ptr() + (np.arange(st, dtype=np.int64)[:, None] * k + np.arange(k)) * S
    addr[:, k:] = parity.data_ptr() + (np.arange(st, dtype=np.int64)[:, None] * m + np.arange(m)) * S
    table = torch.from_numpy(addr.reshape(-1)).to(dev)
    tab = (table.data_ptr(), S, st)
    fbp = first_bad.data_ptr()

    rng = np.random.default_rng(0x4EA)
    mixes = {"one": np.zeros((st, n), dtype=np.uint8), "mixed": np.zeros((st, n), dtype=np.uint8)}
    for s in range(st):
        mixes["one"][s, rng.integers(n)] = 1
        mixes["mixed"][s, rng.choice(n, size=int(rng.integers(1, m + 1)), replace=False)] = 1

    def clean(what):
        stream.synchronize()
        assert int((first_bad != -1).sum()) == 0, what

    out = []
    for mix, er in mixes.items():
        if mix not in want_mixes:
            continue
        flags = er.tobytes()
        e = er.sum(axis=1).astype(np.int64)
        ss, ii = np.nonzero(er)
        dpos = torch.from_numpy(np.array([s * k * S + i * S for s, i in zip(ss, ii) if i < k], dtype=np.int64)).to(dev)
        ppos = torch.from_numpy(np.array([s * m * S + (i - k) * S for s, i in zip(ss, ii) if i >= k], dtype=np.int64)).to(dev)
        for placement in placements:
            p = placement == "ptrs"
            arms = {
                "fused": (lambda: f_fused.reconstruct_checked_ptrs(*tab, flags, fbp, sh)) if p else
                         (lambda: f_fused.reconstruct_checked(*geom, flags, fbp, sh)),
                "split": (lambda: f_split.reconstruct_checked_ptrs(*tab, flags, fbp, sh)) if p else
                         (lambda: f_split.reconstruct_checked(*geom, flags, fbp, sh)),
                "two_calls": (lambda: (plain.verify_ptrs(*tab, fbp, erased=flags, stream=sh),
                                       plain.reconstruct_ptrs(*tab, flags, sh))) if p else
                             (lambda: (plain.verify_degraded(*geom, flags, fbp, sh),
                                       plain.reconstruct_stripes(*geom, flags, sh))),
                "verify": (lambda: plain.verify_ptrs(*tab, fbp, stream=sh)) if p else
                          (lambda: plain.verify_stripes(*geom, fbp, sh)),
                "reconstruct": (lambda: plain.reconstruct_ptrs(*tab, flags, sh)) if p else
                               (lambda: plain.reconstruct_stripes(*geom, flags, sh)),
            }
            # every repairing arm fills wrong slots, reports clean and leaves a clean image
            for name in ("fused", "split", "two_calls"):
                data[dpos] ^= 0x5A
                parity[ppos] ^= 0x5A
                arms[name]()
                clean(f"{name}: a degraded stripe does not verify")
                arms["verify"]()
                clean(f"{name}: the repaired image does not verify")
            repaired0 = f_fused.stat(f_fused.STAT_REPAIR_CHECKED)
            times = {name: [] for name in arms}
            hosts = {name: [] for name in arms}
            for r in range(warmup + reps):
                for name, fn in arms.items():
                    ms, host = timed(stream, fn)
                    if r >= warmup:
                        times[name].append(ms)
                        hosts[name].append(host)
            per_call = (f_fused.stat(f_fused.STAT_REPAIR_CHECKED) - repaired0) / (warmup + reps)

            def row(name, nbytes):
                ts = times[name]
                ms = statistics.median(ts)
                return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                        "enqueue_ms": round(statistics.median(hosts[name]), 4),
                        "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1)}

            one_pass = st * n * S
            two_pass = int(((k + m - e) * (e < m) + k + e).sum()) * S
            res = {"config": cfg, "code": f"RS({k},{m})", "shard": S, "stripes": st, "mix": mix,
                   "placement": placement, "reps": reps, "warmup": warmup, "mean_e": round(float(e.mean()), 3),
                   "repair_kernel": f_fused.kernel_name(13 if p else 12),
                   "repair_stripes_per_call": per_call,
                   "fused": row("fused", one_pass), "split": row("split", two_pass),
                   "two_calls": row("two_calls", two_pass), "verify": row("verify", one_pass),
                   "reconstruct": row("reconstruct", int((k + e).sum()) * S)}
            for name in ("fused", "split", "two_calls", "reconstruct"):
                res[name + "_over_verify"] = round(res[name]["ms"] / res["verify"]["ms"], 4)
            res["fused_over_two_calls"] = round(res["fused"]["ms"] / res["two_calls"]["ms"], 4)
            res["bytes_fused_over_two_calls"] = round(one_pass / two_pass, 4)
            out.append(res)
    for f in (plain, f_fused, f_split):
        f.close()
    del data, parity, table
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 5], choices=sorted(CONFIGS))
    ap.add_argument("--stripes", type=int, default=0, help="stripes (default: the config's)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mixes", nargs="+", default=["one", "mixed"], choices=["one", "mixed"])
    ap.add_argument("--placements", nargs="+", default=["strided", "ptrs"], choices=["strided", "ptrs"])
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("at least 5 repetitions")
    if not torch.cuda.is_available():
        sys.exit("repair_checked_bench needs the GPU")
    for cfg in a.configs:
        for res in run_config(cfg, a.stripes, a.reps, a.warmup, a.mixes, a.placements):
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the parity update of stripes with missing shards.

For BASELINE config 2 (6,553 stripes x RS(10,4) x 1 MiB shards) and config 5
(16,384 stripes x RS(64,16) x 64 KiB shards), with one changed data shard in
every stripe (shard s % k of stripe s), this times, in one process and on the
same buffers,
  * a_intact:       rs_update_stripes, no flags -- the yardstick; (3 + 2m)*S
                    per stripe,
  * b_parity_gone:  rs_update_degraded, the changed shard present and one
                    parity shard (row s % m) erased; (3 + 2(m - 1))*S,
  * c_shard_gone:   rs_update_degraded, the changed shard erased, e = 1;
                    (k + 1 + 2m)*S,
  * d_e_is_m:       rs_update_degraded, the changed shard and parity rows
                    0 .. m - 2 erased, e = m: the one present parity shard is a
                    survivor, read and patched in place; (k + 1 + 2)*S,
  * e_read_combine: the way round for c without rs_update_degraded --
                    rs_read_stripes of the old contents into scratch, then one
                    accumulating rs_combine job per stripe over (old, new);
                    (k + 1)*S + (2 + 2m)*S.
HIP events around each arm on the caller's stream, --warmup untimed rounds,
then the median of --reps; the arms alternate inside one loop so drift of the
box hits all alike.  The lists and tables are built once, outside the timed
calls; what a call does on the host (planning, pattern lookups) is inside.
GB/s counts the bytes the arm moves; `hbm` is that over 8 TB/s.  The first
update changes every stripe; later calls rewrite the same contents (old ==
new), which moves the same bytes and keeps every stripe a codeword, so the
stripes are verified (rs_verify_stripes) after the first update and at the
end.  One JSON line per config, appended to --out
(profiles/update_degraded/update_degraded_bench.jsonl unless told otherwise).

    python tools/update_degraded_bench.py [--configs 2 5] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "noise-erasurecode-plugin_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = {2: (10, 14, 1 << 20, 6553), 5: (64, 80, 65536, 16384)}
HBM_PEAK = 8e12  # bytes/s


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def run_config(cfg, stripes, reps, warmup):
    import rsmi

    k, n, S, default_stripes = CONFIGS[cfg]
    st = stripes or default_stripes
    m = n - k
    dev = torch.device("cuda", 0)
    f = rsmi.FEC(k, n, device=0)
    E = np.frombuffer(f.matrix(), dtype=np.uint8).reshape(n, k)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    data = torch.empty(st * k * S, dtype=torch.uint8, device=dev)
    parity = torch.empty(st * m * S, dtype=torch.uint8, device=dev)
    new = torch.empty(st * S, dtype=torch.uint8, device=dev)      # stripe s's new shard at new[s * S]
    scratch = torch.empty(st * S, dtype=torch.uint8, device=dev)  # arm e: the regenerated old shard
    first_bad = torch.zeros(st, dtype=torch.int32, device=dev)
    f.fill_splitmix(data.data_ptr(), data.numel(), 0x5C2B, sh)
    f.fill_splitmix(new.data_ptr(), new.numel(), 0x0DD5, sh)
    geom = (data.data_ptr(), k * S, parity.data_ptr(), m * S, S, S, st)
    # the tables are built once, outside the timed calls
    updates = rsmi.shard_updates([(s, s % k, new.data_ptr() + s * S) for s in range(st)])
    reads = rsmi.shard_reads([(s, s % k, scratch.data_ptr() + s * S) for s in range(st)])
    fl_b = np.zeros((st, n), dtype=np.uint8)
    fl_c = np.zeros((st, n), dtype=np.uint8)
    fl_d = np.zeros((st, n), dtype=np.uint8)
    for s in range(st):
        fl_b[s, k + s % m] = 1
        fl_c[s, s % k] = 1
        fl_d[s, s % k] = 1
        fl_d[s, k:k + m - 1] = 1
    fl_b, fl_c, fl_d = fl_b.tobytes(), fl_c.tobytes(), fl_d.tobytes()
    jobs = rsmi.combine_jobs([([scratch.data_ptr() + s * S, new.data_ptr() + s * S],
                               [parity.data_ptr() + (s * m + r) * S for r in range(m)],
                               bytes(int(E[k + r, s % k]) for r in range(m) for _ in range(2)), 1)
                              for s in range(st)])

    def clean():
        f.verify_stripes(*geom, first_bad.data_ptr(), sh)
        stream.synchronize()
        return int((first_bad != -1).sum()) == 0

    def read_combine():
        f.read_stripes(*geom, fl_c, reads, sh)
        f.combine(jobs, S, sh)

    arms = {"a_intact": lambda: f.update_stripes(*geom, updates, sh),
            "b_parity_gone": lambda: f.update_degraded(*geom, fl_b, updates, sh),
            "c_shard_gone": lambda: f.update_degraded(*geom, fl_c, updates, sh),
            "d_e_is_m": lambda: f.update_degraded(*geom, fl_d, updates, sh),
            "e_read_combine": read_combine}

    f.encode_stripes(*geom, sh)
    assert clean(), "encoded stripes do not verify"
    # The first update changes every stripe; every later call, whatever its
    # flags, finds old == new (read or regenerated) and patches by zero.
    arms["a_intact"]()
    assert clean(), "updated stripes do not verify"
    for s in (0, st // 2, st - 1):
        assert torch.equal(data[(s * k + s % k) * S:(s * k + s % k + 1) * S], new[s * S:(s + 1) * S]), "data not committed"

    times = {name: [] for name in arms}
    for r in range(warmup + reps):
        for name, fn in arms.items():
            ms = timed(stream, fn)
            if r >= warmup:
                times[name].append(ms)
    assert clean(), "stripes do not verify after the timed calls"

    per_stripe = {"a_intact": 3 + 2 * m, "b_parity_gone": 3 + 2 * (m - 1), "c_shard_gone": k + 1 + 2 * m,
                  "d_e_is_m": k + 1 + 2, "e_read_combine": (k + 1) + (2 + 2 * m)}

    def row(name):
        ts = times[name]
        ms = statistics.median(ts)
        moved = per_stripe[name] * S * st
        return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "bytes": moved,
                "GBps": round(moved / ms / 1e6, 1), "hbm": round(moved / (ms * 1e-3) / HBM_PEAK, 4)}

    res = {"config": cfg, "code": f"RS({k},{m})", "shard": S, "stripes": st, "reps": reps, "warmup": warmup,
           "kernel": f.kernel_name(7), "update_kernel": f.kernel_name(3), "read_kernel": f.kernel_name(4),
           "degraded_stripes": f.stat(f.STAT_UPDATE_DEGRADED), "absorbed": f.stat(f.STAT_UPDATE_ABSORBED)}
    for name in arms:
        res[name] = row(name)
    a_ms, e_ms = res["a_intact"]["ms"], res["e_read_combine"]["ms"]
    for name in ("b_parity_gone", "c_shard_gone", "d_e_is_m", "e_read_combine"):
        res[name + "_over_a"] = round(res[name]["ms"] / a_ms, 4)
        res[name + "_over_a_bytes"] = round(per_stripe[name] / per_stripe["a_intact"], 4)
    res["c_over_e"] = round(res["c_shard_gone"]["ms"] / e_ms, 4)
    res["c_over_e_bytes"] = round(per_stripe["c_shard_gone"] / per_stripe["e_read_combine"], 4)
    f.close()
    del data, parity, new, scratch
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 5], choices=sorted(CONFIGS))
    ap.add_argument("--stripes", type=int, default=0, help="stripes (default: the config's)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_degraded", "update_degraded_bench.jsonl"),
                    help="append the JSON lines to this file ('' for none)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("update_degraded_bench needs the GPU")
    for cfg in a.configs:
        line = json.dumps(run_config(cfg, a.stripes, a.reps, a.warmup))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

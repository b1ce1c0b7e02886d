#!/usr/bin/env python3
"""Cost of the in-place parity update against copy plus re-encode.

For BASELINE config 2 (6,553 stripes x RS(10,4) x 1 MiB shards) and config 5
(16,384 stripes x RS(64,16) x 64 KiB shards) this times, in one process and on
the same buffers,
  * update_all:   rs_update_stripes with one changed data shard in every
                  stripe (shard s % k of stripe s); moves (3 + 2m)*S per stripe,
  * copy_encode:  the yardstick -- a device copy of the same new shards into
                  place (k strided copies, one per shard id) followed by
                  rs_encode_stripes of all stripes; moves (2 + k + m)*S per
                  stripe.  `copy` and `encode` are the two halves, timed in the
                  same loop,
  * update_1pct:  rs_update_stripes with one changed shard in 1% of the
                  stripes.
HIP events around each arm on the caller's stream, --warmup untimed rounds,
then the median of --reps; the arms alternate inside one loop so drift of the
box hits all alike.  GB/s counts the bytes the arm moves; `hbm` is that over
8 TB/s.  The stripes are verified (rs_verify_stripes) after the first update
and again at the end.  One JSON line per config, appended to --out
(profiles/update/update_bench.jsonl unless told otherwise).

    python tools/update_bench.py [--configs 2 5] [--reps 20] [--out FILE]
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
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    data = torch.empty(st * k * S, dtype=torch.uint8, device=dev)
    parity = torch.empty(st * m * S, dtype=torch.uint8, device=dev)
    new = torch.empty(st * S, dtype=torch.uint8, device=dev)  # stripe s's new shard at new[s * S]
    first_bad = torch.zeros(st, dtype=torch.int32, device=dev)
    f.fill_splitmix(data.data_ptr(), data.numel(), 0x5C2B, sh)
    f.fill_splitmix(new.data_ptr(), new.numel(), 0x0DD5, sh)
    geom = (data.data_ptr(), k * S, parity.data_ptr(), m * S, S, S, st)
    all_updates = [(s, s % k, new.data_ptr() + s * S) for s in range(st)]
    few = np.sort(np.random.default_rng(0xD1127).choice(st, size=max(1, st // 100), replace=False))
    few_updates = rsmi.shard_updates([all_updates[int(s)] for s in few])
    all_updates = rsmi.shard_updates(all_updates)  # the tables are built once, outside the timed calls
    # 8-byte views for the yardstick's strided copies (S is a multiple of 8)
    dv = data.view(torch.int64).view(st, k, S // 8)
    nv = new.view(torch.int64).view(st, S // 8)

    def clean():
        f.verify_stripes(*geom, first_bad.data_ptr(), sh)
        stream.synchronize()
        return int((first_bad != -1).sum()) == 0

    def copy_in():
        for i in range(min(k, st)):
            dv[i::k, i].copy_(nv[i::k])

    encode = lambda: f.encode_stripes(*geom, sh)  # noqa: E731
    update_all = lambda: f.update_stripes(*geom, all_updates, sh)  # noqa: E731
    update_few = lambda: f.update_stripes(*geom, few_updates, sh)  # noqa: E731

    def copy_encode():
        copy_in()
        encode()

    encode()
    assert clean(), "encoded stripes do not verify"
    # The first update changes every stripe; later ones rewrite the same
    # contents (old == new), which moves the same bytes.
    update_all()
    assert clean(), "updated stripes do not verify"
    probe = [0, st // 2, st - 1]
    for s in probe:
        assert torch.equal(data[(s * k + s % k) * S:(s * k + s % k + 1) * S], new[s * S:(s + 1) * S]), "data not committed"

    arms = {"update_all": update_all, "copy_encode": copy_encode, "copy": copy_in, "encode": encode,
            "update_1pct": update_few}
    times = {name: [] for name in arms}
    for r in range(warmup + reps):
        for name, fn in arms.items():
            ms = timed(stream, fn)
            if r >= warmup:
                times[name].append(ms)
    assert clean(), "stripes do not verify after the timed calls"

    moved = {"update_all": (3 + 2 * m) * S * st, "copy_encode": (2 + k + m) * S * st, "copy": 2 * S * st,
             "encode": (k + m) * S * st, "update_1pct": (3 + 2 * m) * S * len(few)}

    def row(name):
        ts = times[name]
        ms = statistics.median(ts)
        return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "bytes": moved[name],
                "GBps": round(moved[name] / ms / 1e6, 1), "hbm": round(moved[name] / (ms * 1e-3) / HBM_PEAK, 4)}

    res = {"config": cfg, "code": f"RS({k},{m})", "shard": S, "stripes": st, "reps": reps, "warmup": warmup,
           "update_kernel": f.kernel_name(3), "encode_kernel": f.kernel_name(0), "stripes_1pct": len(few),
           "copy_commits": f.stat(f.STAT_UPDATE_COPY_COMMITS)}
    for name in arms:
        res[name] = row(name)
    res["update_over_copy_encode"] = round(res["update_all"]["ms"] / res["copy_encode"]["ms"], 4)
    res["expected_from_bytes"] = round((3 + 2 * m) / (2 + k + m), 4)
    f.close()
    del data, parity, new, dv, nv
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 5], choices=sorted(CONFIGS))
    ap.add_argument("--stripes", type=int, default=0, help="stripes (default: the config's)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update", "update_bench.jsonl"),
                    help="append the JSON lines to this file ('' for none)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("update_bench needs the GPU")
    for cfg in a.configs:
        line = json.dumps(run_config(cfg, a.stripes, a.reps, a.warmup))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

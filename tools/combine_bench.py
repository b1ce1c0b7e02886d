#!/usr/bin/env python3
"""Cost of rs_combine next to the engine-matrix calls it can stand in for.

Each arm times rs_combine and its yardstick in one process, on the same
buffers and alternating in one loop:
  * delta_update:  BASELINE config 2 (6,553 stripes x RS(10,4) x 1 MiB).  One
                   job per stripe, nsrc = 2 (the old and the new contents of
                   data shard s % k), nout = 4 (the stripe's stored parity),
                   both columns E[k + r][s % k], accumulate: the delta form of
                   the update, 10*S per job.  Yardstick: rs_update_stripes
                   with the same changed shard per stripe, 11*S (it also
                   commits the data).  Held to 1.05x the yardstick's time.
  * partial_8:     the partial sum of RS(64,16) spread over 8 holders: 16,384
                   jobs, nsrc = 8, nout = 1, 64 KiB, 9*S.  No yardstick.
  * row_64:        BASELINE config 5 (16,384 stripes x RS(64,16) x 64 KiB),
                   data shard s % k of stripe s missing: one job per stripe,
                   nsrc = 64 (the survivors, rs_pattern_survivors), nout = 1
                   (the decode row, rs_pattern_rows).  Yardstick:
                   rs_read_stripes of the same shard.  Both move 65*S.
  * row_10:        the same for config 2: nsrc = 10, nout = 1, 1 MiB, 11*S.
The read kernel has K compiled in and the combine kernel has not; the row arms
show what that costs.  HIP events around each call on the caller's stream,
--warmup untimed rounds, then the median of --reps.  GB/s counts the bytes the
arm moves by the formula of rsmi.h; `hbm` is that over 8 TB/s.  Every arm's
output is compared with its yardstick's (or the pristine shard) before and
after the timed loop.  One JSON line per arm, appended to --out
(profiles/combine/combine_bench.jsonl unless told otherwise).

    python tools/combine_bench.py [--arms delta_update row_64] [--reps 20] [--out FILE]
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
ARMS = ("delta_update", "partial_8", "row_64", "row_10")


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def measure(stream, arms, reps, warmup):
    """Median-of-reps rows of the arms, alternating inside one loop."""
    times = {name: [] for name in arms}
    for r in range(warmup + reps):
        for name, (fn, _) in arms.items():
            ms = timed(stream, fn)
            if r >= warmup:
                times[name].append(ms)
    rows = {}
    for name, (_, moved) in arms.items():
        ts = times[name]
        ms = statistics.median(ts)
        rows[name] = {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "bytes": moved,
                      "GBps": round(moved / ms / 1e6, 1), "hbm": round(moved / (ms * 1e-3) / HBM_PEAK, 4)}
    return rows


def delta_update(stripes, reps, warmup):
    import rsmi

    k, n, S, default_stripes = CONFIGS[2]
    st, m = stripes or default_stripes, n - k
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
    E = np.frombuffer(f.matrix(), dtype=np.uint8).reshape(n, k)
    dp, pp, np_ = data.data_ptr(), parity.data_ptr(), new.data_ptr()
    # the tables are built once, outside the timed calls
    updates = rsmi.shard_updates([(s, s % k, np_ + s * S) for s in range(st)])
    jobs = rsmi.combine_jobs([([dp + (s * k + s % k) * S, np_ + s * S], [pp + (s * m + r) * S for r in range(m)],
                               bytes(int(E[k + r, s % k]) for r in range(m) for _ in range(2)), 1) for s in range(st)])

    def clean():
        f.verify_stripes(*geom, first_bad.data_ptr(), sh)
        stream.synchronize()
        return int((first_bad != -1).sum()) == 0

    combine = lambda: f.combine(jobs, S, sh)  # noqa: E731
    update = lambda: f.update_stripes(*geom, updates, sh)  # noqa: E731

    f.encode_stripes(*geom, sh)
    assert clean(), "encoded stripes do not verify"
    # The delta form first, on stripes whose data is still the old one: the
    # parity it leaves must be the parity of the stripes with the new shards
    # in place, which the copy below puts there.
    combine()
    dv, nv = data.view(torch.int64).view(st, k, S // 8), new.view(torch.int64).view(st, S // 8)
    for i in range(min(k, st)):
        dv[i::k, i].copy_(nv[i::k])
    assert clean(), "stripes patched by the delta form do not verify"
    # From here on old == new: both arms move the same bytes as before and
    # leave the parity as it is.
    arms = {"combine": (combine, 10 * S * st), "update": (update, 11 * S * st)}
    rows = measure(stream, arms, reps, warmup)
    assert clean(), "stripes do not verify after the timed calls"
    res = {"arm": "delta_update", "code": f"RS({k},{m})", "len": S, "jobs": st, "nsrc": 2, "nout": m, "accumulate": 1,
           "reps": reps, "warmup": warmup, "combine_kernel": f.kernel_name(6), "yardstick": "rs_update_stripes",
           "yardstick_kernel": f.kernel_name(3), **rows,
           "combine_over_yardstick": round(rows["combine"]["ms"] / rows["update"]["ms"], 4), "bar": 1.05}
    f.close()
    return res


def partial_8(stripes, reps, warmup):
    import rsmi

    k, n, S, default_stripes = CONFIGS[5]
    st, held = stripes or default_stripes, 8
    dev = torch.device("cuda", 0)
    f = rsmi.FEC(k, n, device=0)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    src = torch.empty(st * held * S, dtype=torch.uint8, device=dev)  # a holder's 8 survivors of every stripe
    out = torch.empty(st * S, dtype=torch.uint8, device=dev)
    f.fill_splitmix(src.data_ptr(), src.numel(), 0x8A27, sh)
    rng = np.random.default_rng(0x9A27)
    coef = rng.integers(1, 256, size=held, dtype=np.uint8)
    jobs = rsmi.combine_jobs([([src.data_ptr() + (s * held + c) * S for c in range(held)], [out.data_ptr() + s * S],
                               coef.tobytes(), 0) for s in range(st)])
    combine = lambda: f.combine(jobs, S, sh)  # noqa: E731
    combine()
    stream.synchronize()
    from oracle import oracle
    for s in (0, st // 2, st - 1):
        shards = [src[(s * held + c) * S:(s * held + c + 1) * S].cpu().numpy() for c in range(held)]
        want = oracle.matmul_stripe(coef.reshape(1, held), shards)[0]
        assert np.array_equal(out[s * S:(s + 1) * S].cpu().numpy(), want), "partial sum mismatch"
    rows = measure(stream, {"combine": (combine, (held + 1) * S * st)}, reps, warmup)
    res = {"arm": "partial_8", "code": f"RS({k},{n - k})", "len": S, "jobs": st, "nsrc": held, "nout": 1,
           "accumulate": 0, "reps": reps, "warmup": warmup, "combine_kernel": f.kernel_name(6), "yardstick": None,
           **rows}
    f.close()
    return res


def row_arm(cfg, stripes, reps, warmup):
    import rsmi

    k, n, S, default_stripes = CONFIGS[cfg]
    st, m = stripes or default_stripes, n - k
    dev = torch.device("cuda", 0)
    f = rsmi.FEC(k, n, device=0)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    data = torch.empty(st * k * S, dtype=torch.uint8, device=dev)
    parity = torch.empty(st * m * S, dtype=torch.uint8, device=dev)
    out_c = torch.zeros(st * S, dtype=torch.uint8, device=dev)
    out_r = torch.zeros(st * S, dtype=torch.uint8, device=dev)
    f.fill_splitmix(data.data_ptr(), data.numel(), 0x5C2B, sh)
    geom = (data.data_ptr(), k * S, parity.data_ptr(), m * S, S, S, st)
    f.encode_stripes(*geom, sh)
    erased = np.zeros((st, n), dtype=np.uint8)
    erased[np.arange(st), np.arange(st) % k] = 1
    # one decode row and survivor list per missing id
    row, ids = {}, {}
    for i in range(min(k, st)):
        rows, cnt = f.pattern_rows(erased[i].tobytes())
        assert cnt == 1
        row[i], ids[i] = rows[:k], f.pattern_survivors(erased[i].tobytes())
    dp, pp = data.data_ptr(), parity.data_ptr()

    def shard(s, i):
        return dp + (s * k + i) * S if i < k else pp + (s * m + i - k) * S

    jobs = rsmi.combine_jobs([([shard(s, i) for i in ids[s % k]], [out_c.data_ptr() + s * S], row[s % k], 0)
                              for s in range(st)])
    reads = rsmi.shard_reads([(s, s % k, out_r.data_ptr() + s * S) for s in range(st)])
    flags = erased.tobytes()
    combine = lambda: f.combine(jobs, S, sh)  # noqa: E731
    read = lambda: f.read_stripes(*geom, flags, reads, sh)  # noqa: E731

    def same():
        stream.synchronize()
        want = data.view(st, k, S)[torch.arange(st, device=dev), torch.arange(st, device=dev) % k]
        return torch.equal(out_c.view(st, S), want) and torch.equal(out_r.view(st, S), want)

    combine()
    read()
    assert same(), "regenerated shards differ from the stored ones"
    moved = (k + 1) * S * st
    rows = measure(stream, {"combine": (combine, moved), "read": (read, moved)}, reps, warmup)
    assert same(), "regenerated shards differ after the timed calls"
    res = {"arm": f"row_{k}", "code": f"RS({k},{m})", "len": S, "jobs": st, "nsrc": k, "nout": 1, "accumulate": 0,
           "reps": reps, "warmup": warmup, "combine_kernel": f.kernel_name(6), "yardstick": "rs_read_stripes",
           "yardstick_kernel": f.kernel_name(4), **rows,
           "combine_over_yardstick": round(rows["combine"]["ms"] / rows["read"]["ms"], 4)}
    f.close()
    return res


def run_arm(name, stripes, reps, warmup):
    if name == "delta_update":
        res = delta_update(stripes, reps, warmup)
    elif name == "partial_8":
        res = partial_8(stripes, reps, warmup)
    else:
        res = row_arm(5 if name == "row_64" else 2, stripes, reps, warmup)
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", nargs="+", default=list(ARMS), choices=ARMS)
    ap.add_argument("--stripes", type=int, default=0, help="jobs per arm (default: the arm's)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "combine", "combine_bench.jsonl"),
                    help="append the JSON lines to this file ('' for none)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("combine_bench needs the GPU")
    for name in a.arms:
        line = json.dumps(run_arm(name, a.stripes, a.reps, a.warmup))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the degraded read against the repair of the same stripes.

For BASELINE config 2 (6,553 stripes x RS(10,4) x 1 MiB shards, every stripe
with e = 1 and then e = 4 erasures) and config 5 (16,384 stripes x RS(64,16) x
64 KiB shards, a fresh pattern of 1..16 erasures per stripe) this times, in one
process and on the same buffers and erasure flags,
  * read_all:     rs_read_stripes of one missing data shard of every stripe
                  into a separate buffer; moves (k + 1)*S per stripe,
  * repair_all:   the yardstick -- rs_reconstruct_stripes of every stripe,
                  which regenerates all e erased shards in place; moves
                  (k + e)*S per stripe,
  * read_1pct / repair_1pct: the same for 1% of the stripes (the repair with
                  the flags of the other stripes cleared).
HIP events around each arm on the caller's stream, --warmup untimed rounds,
then the median of --reps; the arms alternate inside one loop so drift of the
box hits all alike.  GB/s counts the bytes the arm moves; `hbm` is that over
8 TB/s.  Before the first read the slots of the erased shards are zeroed; the
shards read are compared with copies taken before that, and the stripes are
verified (rs_verify_stripes) after the first repair and at the end.  One JSON
line per config and e, appended to --out (profiles/read/read_bench.jsonl unless
told otherwise).

    python tools/read_bench.py [--configs 2 5] [--reps 20] [--out FILE]
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
ERASURES = {2: (1, 4), 5: (0,)}  # 0: a fresh pattern of 1..m erasures per stripe
HBM_PEAK = 8e12  # bytes/s


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def flags_for(k, n, st, e, rng):
    """Erasure flags [st][n] and the wanted missing data shard of each stripe."""
    m = n - k
    er = np.zeros((st, n), dtype=np.uint8)
    want = np.arange(st) % k
    er[np.arange(st), want] = 1
    if e == 0:  # config 5: 1..m erasures anywhere, the wanted shard among them
        for s in range(st):
            extra = int(rng.integers(0, m))
            if extra:
                others = np.delete(np.arange(n), want[s])
                er[s, rng.choice(others, size=extra, replace=False)] = 1
    else:       # e erasures: two more data shards and a parity shard for e = 4
        for j, idx in enumerate([(want + 3) % k, (want + 6) % k, k + np.arange(st) % m][:e - 1]):
            er[np.arange(st), idx] = 1
        assert (er.sum(axis=1) == e).all()
    return er, want


def run_config(cfg, e, stripes, reps, warmup):
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
    dst = torch.zeros(st * S, dtype=torch.uint8, device=dev)  # stripe s's shard at dst[s * S]
    first_bad = torch.zeros(st, dtype=torch.int32, device=dev)
    f.fill_splitmix(data.data_ptr(), data.numel(), 0x5C2B, sh)
    geom = (data.data_ptr(), k * S, parity.data_ptr(), m * S, S, S, st)
    rng = np.random.default_rng(0xDE6 + cfg + e)
    er, want = flags_for(k, n, st, e, rng)
    few = np.sort(rng.choice(st, size=max(1, st // 100), replace=False))
    er_few = np.zeros_like(er)
    er_few[few] = er[few]
    flags, flags_few = er.tobytes(), er_few.tobytes()
    all_reads = [(s, int(want[s]), dst.data_ptr() + s * S) for s in range(st)]
    few_reads = rsmi.shard_reads([all_reads[int(s)] for s in few])
    all_reads = rsmi.shard_reads(all_reads)  # the tables are built once, outside the timed calls

    def clean():
        f.verify_stripes(*geom, first_bad.data_ptr(), sh)
        stream.synchronize()
        return int((first_bad != -1).sum()) == 0

    read_all = lambda: f.read_stripes(*geom, flags, all_reads, sh)  # noqa: E731
    read_few = lambda: f.read_stripes(*geom, flags, few_reads, sh)  # noqa: E731
    repair_all = lambda: f.reconstruct_stripes(*geom, flags, sh)  # noqa: E731
    repair_few = lambda: f.reconstruct_stripes(*geom, flags_few, sh)  # noqa: E731

    f.encode_stripes(*geom, sh)
    assert clean(), "encoded stripes do not verify"
    # Copies of the wanted shards of a few stripes, then every erased slot is zeroed.
    dv, pv = data.view(st, k, S), parity.view(st, m, S)
    probe = sorted({0, st // 2, st - 1, int(few[0]), int(few[-1])})
    keep = {s: dv[s, int(want[s])].clone() for s in probe}
    dv[torch.from_numpy(er[:, :k].astype(bool)).to(dev)] = 0
    pv[torch.from_numpy(er[:, k:].astype(bool)).to(dev)] = 0
    stream.synchronize()
    assert not clean(), "zeroed shards went unnoticed"
    read_all()
    stream.synchronize()
    for s in probe:
        assert torch.equal(dst[s * S:(s + 1) * S], keep[s]), f"stripe {s}: wrong bytes read"
        assert not dv[s, int(want[s])].any(), "the read wrote the stripe"
    dst.zero_()
    read_few()
    stream.synchronize()
    for s in (int(few[0]), int(few[-1])):
        assert torch.equal(dst[s * S:(s + 1) * S], keep[s]), f"stripe {s}: wrong bytes read (1%)"
    repair_all()
    assert clean(), "repaired stripes do not verify"

    arms = {"read_all": read_all, "repair_all": repair_all, "read_1pct": read_few, "repair_1pct": repair_few}
    times = {name: [] for name in arms}
    for r in range(warmup + reps):
        for name, fn in arms.items():
            ms = timed(stream, fn)
            if r >= warmup:
                times[name].append(ms)
    assert clean(), "stripes do not verify after the timed calls"

    e_all, e_few = int(er.sum()), int(er_few.sum())
    moved = {"read_all": (k + 1) * S * st, "repair_all": (k * st + e_all) * S,
             "read_1pct": (k + 1) * S * len(few), "repair_1pct": (k * len(few) + e_few) * S}

    def row(name):
        ts = times[name]
        ms = statistics.median(ts)
        return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "bytes": moved[name],
                "GBps": round(moved[name] / ms / 1e6, 1), "hbm": round(moved[name] / (ms * 1e-3) / HBM_PEAK, 4)}

    res = {"config": cfg, "code": f"RS({k},{m})", "shard": S, "stripes": st, "erasures": e or "1..%d" % m,
           "mean_erasures": round(e_all / st, 3), "reps": reps, "warmup": warmup, "read_kernel": f.kernel_name(4),
           "repair_kernel": f.kernel_name(1), "stripes_1pct": len(few), "patterns": f.pattern_count()}
    for name in arms:
        res[name] = row(name)
    res["read_over_repair"] = round(res["read_all"]["ms"] / res["repair_all"]["ms"], 4)
    res["expected_from_bytes"] = round(moved["read_all"] / moved["repair_all"], 4)
    res["read_over_repair_1pct"] = round(res["read_1pct"]["ms"] / res["repair_1pct"]["ms"], 4)
    f.close()
    del data, parity, dst, dv, pv
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 5], choices=sorted(CONFIGS))
    ap.add_argument("--stripes", type=int, default=0, help="stripes (default: the config's)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read", "read_bench.jsonl"),
                    help="append the JSON lines to this file ('' for none)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("read_bench needs the GPU")
    for cfg in a.configs:
        for e in ERASURES[cfg]:
            line = json.dumps(run_config(cfg, e, a.stripes, a.reps, a.warmup))
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()

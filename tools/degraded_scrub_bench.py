#!/usr/bin/env python3
"""Cost of the degraded scrub of device-resident stripes against the verify.

For BASELINE config 2 (6,553 stripes x RS(10,4) x 1 MiB shards) and config 5
(16,384 stripes x RS(64,16) x 64 KiB shards) this times, in one process and on
the same buffers,
  * verify:         rs_verify_stripes of the intact stripes (the yardstick),
  * noflags:        rs_verify_degraded with no flag set (the same kernel plus
                    a host pass over the flags),
  * one_erasure:    rs_verify_degraded with one erasure in every stripe
                    (config 5: 1..16 erasures, stripe s has 1 + s % 16),
  * one_percent:    rs_verify_degraded with 1% of the stripes degraded (the
                    verify kernel over a stripe list plus the check kernel),
  * correct:        rs_correct_degraded with the one_erasure flags and one
                    wholly wrong present shard in 1% of the stripes (corrupted
                    again before every call).
The first byte of every erased slot is overwritten, so a clean verdict also
says that the slot was not read.  HIP events around each call on the caller's
stream, --warmup untimed calls, then the median of --reps; the four verify arms
alternate inside one loop so drift of the box hits all alike.  GB/s counts the
bytes the call has to move ((k+m-e)*S per degraded stripe); `hbm` is that over
8 TB/s.  One JSON line per config, appended to --out when given.

    python tools/degraded_scrub_bench.py [--configs 2 5] [--reps 20] [--out FILE]
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
    first_bad = torch.zeros(st, dtype=torch.int32, device=dev)
    f.fill_splitmix(data.data_ptr(), data.numel(), 0x5C2B, sh)
    geom = (data.data_ptr(), k * S, parity.data_ptr(), m * S, S, S, st)
    f.encode_stripes(*geom, sh)

    rng = np.random.default_rng(0xDE6)
    none = np.zeros((st, n), dtype=np.uint8)
    every = np.zeros((st, n), dtype=np.uint8)  # config 2: one erasure per stripe; config 5: 1..16
    for s in range(st):
        every[s, rng.choice(n, size=1 if cfg == 2 else 1 + s % m, replace=False)] = 1
    few = np.zeros((st, n), dtype=np.uint8)    # 1% of the stripes degraded, with the same erasures
    some = np.sort(rng.choice(st, size=max(1, st // 100), replace=False))
    few[some] = every[some]

    def slot(s, i):
        return (data, s * k * S + i * S) if i < k else (parity, s * m * S + (i - k) * S)

    # the erased slots of `every` hold a wrong first byte from here on
    ss, ii = np.nonzero(every)
    dpos = torch.from_numpy(np.array([s * k * S + i * S for s, i in zip(ss, ii) if i < k], dtype=np.int64)).to(dev)
    ppos = torch.from_numpy(np.array([s * m * S + (i - k) * S for s, i in zip(ss, ii) if i >= k], dtype=np.int64)).to(dev)

    arms = {
        "verify": lambda: f.verify_stripes(*geom, first_bad.data_ptr(), sh),
        "noflags": lambda: f.verify_degraded(*geom, none.tobytes(), first_bad.data_ptr(), sh),
        "one_erasure": lambda: f.verify_degraded(*geom, every.tobytes(), first_bad.data_ptr(), sh),
        "one_percent": lambda: f.verify_degraded(*geom, few.tobytes(), first_bad.data_ptr(), sh),
    }
    for name in ("verify", "noflags"):
        arms[name]()
        stream.synchronize()
        assert int((first_bad != -1).sum()) == 0, f"{name}: encoded stripes do not verify"
    data[dpos] ^= 0x5A
    parity[ppos] ^= 0x5A
    arms["one_erasure"]()
    stream.synchronize()
    assert int((first_bad != -1).sum()) == 0, "one_erasure: degraded stripes do not verify"
    data[dpos] ^= 0x5A
    parity[ppos] ^= 0x5A

    # the intact arms run on intact buffers, the degraded ones with the wrong bytes in place
    def wrong(on):
        if wrong.on != on:
            data[dpos] ^= 0x5A
            parity[ppos] ^= 0x5A
            wrong.on = on
    wrong.on = False

    times = {name: [] for name in arms}
    for r in range(warmup + reps):
        for name, fn in arms.items():
            wrong(name == "one_erasure")
            ms = timed(stream, fn)
            if r >= warmup:
                times[name].append(ms)
    wrong(True)

    # one wholly wrong present shard in 1% of the stripes, one erasure (config 5: 1..15) in each
    bad = some[(every[some] != 0).sum(axis=1) <= m - 2]
    shard = np.array([int(rng.choice(np.flatnonzero(every[s] == 0))) for s in bad])

    def corrupt():
        for s, i in zip(bad, shard):
            buf, o = slot(int(s), int(i))
            buf[o:o + S] ^= 0xA5

    t_correct = []
    regen0 = f.stat(f.STAT_SCRUB_REGENERATED)
    for r in range(warmup + reps):
        corrupt()
        status = []
        ms = timed(stream, lambda: status.append(f.correct_degraded(*geom, every.tobytes(), sh)))
        st_list, rw = status[0]
        assert not any(st_list), "correct: a stripe was not repaired"
        assert np.flatnonzero(np.frombuffer(rw, dtype=np.uint8)).tolist() == [int(s) * n + int(i) for s, i in zip(bad, shard)]
        if r >= warmup:
            t_correct.append(ms)
    regenerated = f.stat(f.STAT_SCRUB_REGENERATED) - regen0
    arms["one_erasure"]()
    stream.synchronize()
    assert int((first_bad != -1).sum()) == 0, "stripes do not verify after the repairs"

    def moved(flags):
        e = (flags != 0).sum(axis=1)
        return int(((k + m - e) * (e < m)).sum()) * S

    def row(ts, nbytes):
        ms = statistics.median(ts)
        return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "bytes": nbytes,
                "GBps": round(nbytes / ms / 1e6, 1), "hbm": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}

    res = {"config": cfg, "code": f"RS({k},{m})", "shard": S, "stripes": st, "reps": reps, "warmup": warmup,
           "verify_kernel": f.kernel_name(2), "check_kernel": f.kernel_name(5),
           "degraded_stripes_one_percent": len(some), "corrupt_stripes": len(bad),
           "regenerated_per_call": regenerated / (warmup + reps),
           "verify": row(times["verify"], moved(none)), "noflags": row(times["noflags"], moved(none)),
           "one_erasure": row(times["one_erasure"], moved(every)),
           "one_percent": row(times["one_percent"], moved(few)), "correct": row(t_correct, moved(every))}
    for name in ("noflags", "one_erasure", "one_percent", "correct"):
        res[name + "_over_verify"] = round(res[name]["ms"] / res["verify"]["ms"], 4)
    f.close()
    del data, parity
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 5], choices=sorted(CONFIGS))
    ap.add_argument("--stripes", type=int, default=0, help="stripes (default: the config's)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("degraded_scrub_bench needs the GPU")
    for cfg in a.configs:
        line = json.dumps(run_config(cfg, a.stripes, a.reps, a.warmup))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

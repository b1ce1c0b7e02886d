#!/usr/bin/env python3
"""Cost of the per-stripe-length scrub (rs_verify_ptrs_lens,
rs_reconstruct_checked_ptrs_lens) on one MI355X.  Run by hand; not part of
bench.py.

(a) twin against original -- the same stripes in EQUAL lengths, RS(10,4) with
    1 MiB shards and RS(64,16) with 64 KiB shards, about 1 GiB moved each.  The
    process sets RSMI_SCRUB_LENS_FORCE=1 before the engine loads, so the _lens
    call stays on the per-stripe-length kernels (`twin`); the yardstick is the
    equal-length call itself (`equal`), which is what a _lens call of equal
    lengths runs without the knob.  The equal-length call is timed twice per
    round (`equal`, `equal_again`): the ratio of those two medians and the
    per-round ratios are the self-ratio spread the twin's ratio is judged
    against.
(b) the use case -- a seeded mix of lengths, log-uniform from 4 KiB to 1 MiB
    (rounded to --quantum bytes), about the same total bytes: one _lens call
    (`lens`) against the only other route, one equal-length call per distinct
    length over sub-tables (`by_length`), all queued on one stream and timed as
    one.
Three calls each: clean verify, verify with one erasure per stripe, checked
repair with one erasure per stripe.  The stripes lie in rows of the longest
length (a prefix of a coded stripe is a coded stripe), every table entry names
its shard's row.  Every arm's first call must report every stripe clean.
HIP events around each arm on the caller's stream, --warmup untimed rounds,
then --reps rounds in which the arms alternate; every rep is listed, with the
median, minimum and maximum.  One JSON line per (part, code, call), appended
to --out when given.

    python tools/scrub_lens_bench.py [--parts a b] [--reps 7] [--out profiles/scrub_lens/FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

os.environ["RSMI_SCRUB_LENS_FORCE"] = "1"  # read once, when the first _lens call runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "noise-erasurecode-plugin_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CODES = {"rs10_4": (10, 14, 1 << 20), "rs64_16": (64, 80, 1 << 16)}  # k, n, the equal length of part (a)
TOTAL = 1 << 30  # bytes a clean verify moves, about


def timed(stream, fn):
    """(ms between HIP events around the call, ms the host spent queueing it)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), host


def stats(ts):
    return {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "reps_ms": [round(t, 4) for t in ts]}


def mixed_lengths(n, quantum, seed):
    """Log-uniform lengths in [4 KiB, 1 MiB], rounded up to `quantum`, until n * sum reaches TOTAL."""
    rng = np.random.default_rng(seed)
    lens = []
    while n * sum(lens) < TOTAL:
        x = int(np.exp(rng.uniform(np.log(4096), np.log(1 << 20))))
        lens.append(min(-(-x // quantum) * quantum, 1 << 20))
    return lens


class Store:
    """Coded stripes in rows of `pitch` bytes, and the tables over them."""

    def __init__(self, f, k, n, lens, stream):
        self.f, self.k, self.n, self.m, self.lens = f, k, n, n - k, lens
        st, pitch = len(lens), max(lens)
        dev = torch.device("cuda", 0)
        self.data = torch.empty(st * k * pitch, dtype=torch.uint8, device=dev)
        self.parity = torch.empty(st * self.m * pitch, dtype=torch.uint8, device=dev)
        f.fill_splitmix(self.data.data_ptr(), self.data.numel(), 0x5C2B, stream)
        f.encode_stripes(self.data.data_ptr(), k * pitch, self.parity.data_ptr(), self.m * pitch, pitch, pitch, st, stream)
        addr = np.empty((st, n), dtype=np.int64)
        addr[:, :k] = self.data.data_ptr() + (np.arange(st, dtype=np.int64)[:, None] * k + np.arange(k)) * pitch
        addr[:, k:] = self.parity.data_ptr() + (np.arange(st, dtype=np.int64)[:, None] * self.m + np.arange(self.m)) * pitch
        self.addr = addr
        self.table = torch.from_numpy(addr.reshape(-1).copy()).to(dev)
        self.first_bad = torch.zeros(st, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(0x4EA)
        self.one = np.zeros((st, n), dtype=np.uint8)
        self.one[np.arange(st), rng.integers(n, size=st)] = 1
        # the sub-tables of the equal-length route: one per distinct length
        self.groups = []
        for S in sorted(set(lens)):
            idx = [s for s in range(st) if lens[s] == S]
            self.groups.append((S, len(idx), torch.from_numpy(addr[idx].reshape(-1).copy()).to(dev),
                                torch.zeros(len(idx), dtype=torch.int32, device=dev), self.one[idx].tobytes()))
        self.clens = (ctypes.c_size_t * st)(*lens)

    def arm(self, call, route, sh):
        """call: clean | degraded | repair; route: lens | by_length."""
        f, st = self.f, len(self.lens)
        flags = None if call == "clean" else self.one.tobytes()
        if route == "lens":
            if call == "repair":
                return lambda: f.reconstruct_checked_ptrs_lens(self.table.data_ptr(), self.clens, st, flags,
                                                               self.first_bad.data_ptr(), sh)
            return lambda: f.verify_ptrs_lens(self.table.data_ptr(), self.clens, st, self.first_bad.data_ptr(),
                                              erased=flags, stream=sh)

        def by_length():
            for S, cnt, tab, fb, one in self.groups:
                if call == "repair":
                    f.reconstruct_checked_ptrs(tab.data_ptr(), S, cnt, one, fb.data_ptr(), sh)
                else:
                    f.verify_ptrs(tab.data_ptr(), S, cnt, fb.data_ptr(), erased=None if call == "clean" else one, stream=sh)
        return by_length

    def all_clean(self, route):
        fbs = [self.first_bad] if route == "lens" else [g[3] for g in self.groups]
        return all(int((fb != -1).sum()) == 0 for fb in fbs)

    def moved(self, call):
        e = 0 if call == "clean" else 1
        per = self.n if call != "degraded" else (self.k + self.m - e if e < self.m else 0)
        return per * sum(-(-S // 16) * 16 for S in self.lens)


def run(part, code, reps, warmup, quantum):
    import rsmi

    k, n, S = CODES[code]
    f = rsmi.FEC(k, n, device=0)
    stream = torch.cuda.current_stream(torch.device("cuda", 0))
    sh = stream.cuda_stream
    lens = [S] * max(2, TOTAL // (n * S)) if part == "a" else mixed_lengths(n, quantum, seed=0x1E45 + k)
    store = Store(f, k, n, lens, sh)
    out = []
    for call in ("clean", "degraded", "repair"):
        if part == "a":  # by_length over one length is the equal-length call itself
            arms = {"equal": store.arm(call, "by_length", sh), "twin": store.arm(call, "lens", sh),
                    "equal_again": store.arm(call, "by_length", sh)}
        else:
            arms = {"lens": store.arm(call, "lens", sh), "by_length": store.arm(call, "by_length", sh)}
        for name, fn in arms.items():
            store.first_bad.fill_(7)
            fn()
            stream.synchronize()
            assert store.all_clean("lens" if name in ("twin", "lens") else "by_length"), f"{code} {call} {name}: not clean"
        launches0 = f.stat(f.STAT_SCRUB_LENS_LAUNCHES)
        times = {name: [] for name in arms}
        hosts = {name: [] for name in arms}
        for r in range(warmup + reps):
            for name, fn in arms.items():
                ms, host = timed(stream, fn)
                if r >= warmup:
                    times[name].append(ms)
                    hosts[name].append(host)
        assert f.stat(f.STAT_SCRUB_LENS_LAUNCHES) - launches0 == warmup + reps, "the _lens arm did not run the twins"
        nbytes = store.moved(call)
        res = {"part": part, "code": f"RS({k},{n - k})", "call": call, "stripes": len(lens), "distinct_lengths": len(set(lens)),
               "min_len": min(lens), "max_len": max(lens), "bytes": nbytes, "reps": reps, "warmup": warmup,
               "kernels": [f.kernel_name(w) for w in (14, 15, 16)]}
        for name in arms:
            res[name] = dict(stats(times[name]), enqueue_ms=round(statistics.median(hosts[name]), 4),
                             GBps=round(nbytes / statistics.median(times[name]) / 1e6, 1))
        if part == "a":
            res["twin_over_equal"] = round(res["twin"]["ms"] / res["equal"]["ms"], 4)
            res["equal_again_over_equal"] = round(res["equal_again"]["ms"] / res["equal"]["ms"], 4)
            self_r = [b / a for a, b in zip(times["equal"], times["equal_again"])]
            twin_r = [b / a for a, b in zip(times["equal"], times["twin"])]
            res["self_ratio_per_round"] = [round(x, 4) for x in self_r]
            res["twin_ratio_per_round"] = [round(x, 4) for x in twin_r]
            res["self_ratio_spread"] = [round(min(self_r), 4), round(max(self_r), 4)]
        else:
            res["lens_over_by_length"] = round(res["lens"]["ms"] / res["by_length"]["ms"], 4)
        out.append(res)
    f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", nargs="+", default=["a", "b"], choices=["a", "b"])
    ap.add_argument("--codes", nargs="+", default=sorted(CODES), choices=sorted(CODES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quantum", type=int, default=4096, help="part (b): lengths are rounded up to this many bytes")
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("at least 5 repetitions")
    if not torch.cuda.is_available():
        sys.exit("scrub_lens_bench needs the GPU")
    for part in a.parts:
        for code in a.codes:
            for res in run(part, code, a.reps, a.warmup, a.quantum):
                line = json.dumps(res)
                print(line, flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as fh:
                        fh.write(line + "\n")


if __name__ == "__main__":
    main()

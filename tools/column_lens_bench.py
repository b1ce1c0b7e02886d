#!/usr/bin/env python3
"""Cost of the per-stripe-length column scrub (rs_correct_columns_ptrs_lens) on
one MI355X.  Run by hand; not part of bench.py.

(a) twin against original -- the same stripes in EQUAL lengths, RS(10,4) with
    1 MiB shards and RS(64,16) with 64 KiB shards, about 1 GiB each.  The
    process sets RSMI_COLUMN_LENS_FORCE=1 before the engine loads, so the _lens
    call stays on the per-stripe-length kernels (`twin`: both verifies and the
    column launch); the yardstick is rs_correct_columns_ptrs itself (`equal`),
    which is what a _lens call of equal lengths runs without the knob.  The
    equal-length call is timed twice per round (`equal`, `equal_again`): the
    ratio of those two medians and the per-round ratios are the self-ratio
    spread the twin's ratio is judged against.
(b) the use case -- a seeded mix of lengths, log-uniform from 4 KiB to 1 MiB
    (rounded to --quantum bytes), about the same total bytes: one _lens call
    (`lens`) against the only other route, one rs_correct_columns_ptrs call per
    distinct length over sub-tables (`by_length`), timed as one.
Two inputs each: `clean`, and `dirty` -- 1% of the stripes (at least one) with a
wrong 4 KiB sector in each of up to three shards, at offsets of their own, so
every column is within the radius.  The call repairs what it finds, so the
sectors are damaged again, untimed, before every timed call; every timed call
must report every stripe RS_OK and exactly the damaged bytes.
The calls are synchronous (two host round trips each), so the figure is the
time between HIP events around the call on the caller's stream, which holds
those round trips; the host's wall time is listed next to it.  --warmup untimed
rounds, then --reps rounds in which the arms alternate; every rep is listed,
with the median, minimum and maximum.  One JSON line per (part, code, input),
appended to --out.

    python tools/column_lens_bench.py [--parts a b] [--reps 7] [--out profiles/column_lens/column_lens_bench.jsonl]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

os.environ["RSMI_COLUMN_LENS_FORCE"] = "1"  # read once, when the first _lens call runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "noise-erasurecode-plugin_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CODES = {"rs10_4": (10, 14, 1 << 20), "rs64_16": (64, 80, 1 << 16)}  # k, n, the equal length of part (a)
TOTAL = 1 << 30  # bytes of all shards, about
SECTOR = 4096


def timed(stream, fn):
    """(ms between HIP events around the call, ms of host wall time in it, its result)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    t0 = time.perf_counter()
    got = fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), host, got


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
    """Coded stripes in rows of `pitch` bytes, the tables over them, and the damage."""

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
        self.table = torch.from_numpy(addr.reshape(-1).copy()).to(dev)
        self.clens = (ctypes.c_size_t * st)(*lens)
        self.groups = []  # the sub-tables of the equal-length route: one per distinct length
        for S in sorted(set(lens)):
            idx = [s for s in range(st) if lens[s] == S]
            self.groups.append((S, idx, torch.from_numpy(addr[idx].reshape(-1).copy()).to(dev)))
        # the damage: every 100th stripe from a seeded start, a sector in each of up to three shards
        rng = np.random.default_rng(0xD1A7)
        self.dirty = list(range(int(rng.integers(min(st, 100))), st, 100))
        self.sectors = []  # (the sector, wrong bytes)
        self.counts = np.zeros((st, n), dtype=np.int64)
        torch.cuda.synchronize()
        for s in self.dirty:
            shards = rng.choice(n, size=3, replace=False)
            for j in range(min(3, lens[s] // SECTOR)):
                i = int(shards[j])
                buf, row = (self.data, s * k + i) if i < k else (self.parity, s * self.m + i - k)
                off = row * pitch + (lens[s] // SECTOR - 1 - j) * SECTOR
                self.sectors.append((buf[off:off + SECTOR], buf[off:off + SECTOR] ^ 0xFF))
                self.counts[s, i] = SECTOR
        self.bad_bytes = int(self.counts.sum())

    def damage(self):
        for sector, wrong in self.sectors:
            sector.copy_(wrong)

    def arm(self, route, sh):
        f, st = self.f, len(self.lens)
        if route == "lens":
            def lens_call():
                status, cnt = f.correct_columns_ptrs_lens(self.table.data_ptr(), self.clens, st, stream=sh)
                return status, np.asarray(cnt, dtype=np.int64).reshape(st, self.n)
            return lens_call

        def by_length():
            status, cnt = [0] * st, np.zeros((st, self.n), dtype=np.int64)
            for S, idx, tab in self.groups:
                st_s, cnt_s = f.correct_columns_ptrs(tab.data_ptr(), S, len(idx), stream=sh)
                for j, s in enumerate(idx):
                    status[s] = st_s[j]
                cnt[idx] = np.asarray(cnt_s, dtype=np.int64).reshape(len(idx), self.n)
            return status, cnt
        return by_length


def run(part, code, reps, warmup, quantum):
    import rsmi

    k, n, S = CODES[code]
    f = rsmi.FEC(k, n, device=0)
    stream = torch.cuda.current_stream(torch.device("cuda", 0))
    sh = stream.cuda_stream
    lens = [S] * max(2, TOTAL // (n * S)) if part == "a" else mixed_lengths(n, quantum, seed=0x1E45 + k)
    store = Store(f, k, n, lens, sh)
    out = []
    for inp in ("clean", "dirty"):
        if part == "a":  # by_length over one length is the equal-length call itself
            arms = {"equal": store.arm("by_length", sh), "twin": store.arm("lens", sh), "equal_again": store.arm("by_length", sh)}
        else:
            arms = {"lens": store.arm("lens", sh), "by_length": store.arm("by_length", sh)}
        launches0 = f.stat(f.STAT_COLUMN_LENS_LAUNCHES)
        times = {name: [] for name in arms}
        hosts = {name: [] for name in arms}
        for r in range(warmup + reps):
            for name, fn in arms.items():
                if inp == "dirty":
                    store.damage()
                stream.synchronize()
                ms, host, (status, cnt) = timed(stream, fn)
                assert status == [0] * len(lens), f"{code} {inp} {name}: a stripe failed"
                want = store.counts if inp == "dirty" else np.zeros_like(store.counts)
                assert np.array_equal(cnt, want), f"{code} {inp} {name}: corrected counts"
                if r >= warmup:
                    times[name].append(ms)
                    hosts[name].append(host)
        twin_launches = f.stat(f.STAT_COLUMN_LENS_LAUNCHES) - launches0
        assert twin_launches == (warmup + reps if inp == "dirty" else 0), "the _lens arm did not run the twin"
        nbytes = n * sum(-(-x // 16) * 16 for x in lens)
        res = {"part": part, "code": f"RS({k},{n - k})", "input": inp, "stripes": len(lens), "distinct_lengths": len(set(lens)),
               "min_len": min(lens), "max_len": max(lens), "bytes": nbytes, "dirty_stripes": len(store.dirty) if inp == "dirty" else 0,
               "wrong_bytes": store.bad_bytes if inp == "dirty" else 0, "reps": reps, "warmup": warmup,
               "kernels": [f.kernel_name(w) for w in (11, 17)]}
        for name in arms:
            res[name] = dict(stats(times[name]), host_ms=round(statistics.median(hosts[name]), 4),
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "column_lens", "column_lens_bench.jsonl"),
                    help="append the JSON lines to this file")
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("at least 5 repetitions")
    if not torch.cuda.is_available():
        sys.exit("column_lens_bench needs the GPU")
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

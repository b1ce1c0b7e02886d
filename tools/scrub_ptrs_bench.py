#!/usr/bin/env python3
"""Cost of the pointer-placement scrub (rs_verify_ptrs, rs_correct_columns_ptrs)
against the strided calls on the same stripes and against the only route the
pointer placement had before: copy every shard into a strided scratch image,
scrub there, copy back.

For RS(10,4) with 1 MiB shards and RS(64,16) with 64 KiB shards, in one process:
the stripes are encoded once into a dense strided image ([stripes][n][S], data
and parity of a stripe joined), then copied shard by shard to the rows of a
pool of the same size in shuffled order; the device table names those rows.
  1. clean:    rs_verify_ptrs against rs_verify_stripes;
  2. degraded: one erasure per stripe -- rs_verify_ptrs against
               rs_verify_degraded with the same flags;
  3. sectors:  1% of the stripes with one 4 KiB wrong run in each of three
               different shards at three different offsets --
               rs_correct_columns_ptrs against rs_correct_columns;
and every arm against the copy route on the pool: a gather of all stripes * n
shards into the strided image (torch.index_select of 8-byte words; its GB/s is
reported), the strided call there and, for arm 3, the scatter back
(index_copy_).  The verify arms need no copy back.
HIP events around each call on the caller's stream (the correct calls are
synchronous, so their host round trips are inside), --warmup untimed rounds,
then the median of --reps; the calls of an arm alternate inside one loop, and
the damage is put back before every timed correcting call.  One JSON line per
code, appended to --out when given.

    python tools/scrub_ptrs_bench.py [--codes 10_4 64_16] [--reps 20] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "noise-erasurecode-plugin_amd")
sys.path[:0] = [ROOT, PKG]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CODES = {"10_4": (10, 14, 1 << 20, 1024), "64_16": (64, 80, 65536, 2048)}
RUN = 4096  # bytes of a bad sector


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def run_code(name, stripes, reps, warmup):
    import rsmi

    k, n, S, default_stripes = CODES[name]
    st = stripes or default_stripes
    m = n - k
    dev = torch.device("cuda", 0)
    f = rsmi.FEC(k, n, device=0)
    lib = rsmi.load()
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    rows = st * n
    img = torch.empty(rows * S, dtype=torch.uint8, device=dev)
    pool = torch.empty(rows * S, dtype=torch.uint8, device=dev)
    first_bad = torch.zeros(st, dtype=torch.int32, device=dev)
    # the strided image: stripe s at img + s * n * S, its parity behind its data
    geom = (img.data_ptr(), n * S, img.data_ptr() + k * S, n * S, S, S, st)
    f.fill_splitmix(img.data_ptr(), img.numel(), 0x5C2B, sh)
    f.encode_stripes(*geom, sh)
    # the pool: shard (s, i) in row perm[s * n + i]
    rng = np.random.default_rng(0xD1127)
    perm = rng.permutation(rows)
    perm_t = torch.from_numpy(perm).to(dev)
    img_w = img.view(torch.int64).view(rows, S // 8)
    pool_w = pool.view(torch.int64).view(rows, S // 8)
    copy_in = lambda: torch.index_select(pool_w, 0, perm_t, out=img_w)  # noqa: E731
    copy_out = lambda: pool_w.index_copy_(0, perm_t, img_w)  # noqa: E731
    copy_out()
    table = torch.from_numpy(pool.data_ptr() + perm.astype(np.int64) * S).to(dev)
    tp = table.data_ptr()

    one = np.zeros((st, n), dtype=np.uint8)
    one[np.arange(st), rng.integers(0, n, size=st)] = 1
    flags = one.tobytes()
    status = (ctypes.c_int * st)()
    counts = np.zeros(rows, dtype=np.uint32)
    cp = counts.ctypes.data_as(ctypes.c_void_p)

    v_ptrs = lambda: f.verify_ptrs(tp, S, st, first_bad.data_ptr(), stream=sh)  # noqa: E731
    v_strided = lambda: f.verify_stripes(*geom, first_bad.data_ptr(), sh)  # noqa: E731
    d_ptrs = lambda: f.verify_ptrs(tp, S, st, first_bad.data_ptr(), erased=flags, stream=sh)  # noqa: E731
    d_strided = lambda: f.verify_degraded(*geom, flags, first_bad.data_ptr(), sh)  # noqa: E731
    # the C ABI itself: the binding's Python lists would be inside the timed span
    c_ptrs = lambda: lib.rs_correct_columns_ptrs(f._h, tp, S, st, None, status, cp, sh or None)  # noqa: E731
    c_strided = lambda: lib.rs_correct_columns(f._h, *geom, None, status, cp, sh or None)  # noqa: E731

    def all_clean(call):
        call()
        stream.synchronize()
        return int((first_bad != -1).sum()) == 0

    assert all_clean(v_strided) and all_clean(v_ptrs), "encoded stripes do not verify"
    assert all_clean(d_strided) and all_clean(d_ptrs), "degraded stripes do not verify"

    def route(call, back):
        copy_in()
        rc = call()
        if back:
            copy_out()
        return rc

    # copies alone, then 1. and 2.: the verify arms
    t = {key: [] for key in ("copy_in", "copy_out", "verify_ptrs", "verify_stripes", "verify_route",
                             "degraded_ptrs", "verify_degraded", "degraded_route",
                             "correct_ptrs", "correct_columns", "correct_route")}
    for r in range(warmup + reps):
        ms = {"copy_in": timed(stream, copy_in), "copy_out": timed(stream, copy_out),
              "verify_ptrs": timed(stream, v_ptrs), "verify_stripes": timed(stream, v_strided),
              "verify_route": timed(stream, lambda: route(v_strided, False)),
              "degraded_ptrs": timed(stream, d_ptrs), "verify_degraded": timed(stream, d_strided),
              "degraded_route": timed(stream, lambda: route(d_strided, False))}
        if r >= warmup:
            for key, v in ms.items():
                t[key].append(v)

    # 3. three bad sectors on three shards at three offsets in 1% of the stripes
    bad = np.sort(rng.choice(st, size=max(1, st // 100), replace=False))
    trio = [rng.choice(n, size=3, replace=False) for _ in bad]
    offs = (0, (S // 2) // 16 * 16, S - RUN)

    def corrupt(buf, row_of):
        for s, three in zip(bad, trio):
            for i, off in zip(three, offs):
                o = row_of(int(s) * n + int(i)) * S + off
                buf[o:o + RUN].bitwise_xor_(0x3C)

    want = len(bad) * 3 * RUN
    for r in range(warmup + reps):
        ms = {}
        for key, buf, row_of, call in (("correct_ptrs", pool, lambda x: int(perm[x]), c_ptrs),
                                       ("correct_columns", img, lambda x: x, c_strided),
                                       ("correct_route", pool, lambda x: int(perm[x]), lambda: route(c_strided, True))):
            corrupt(buf, row_of)
            got = []
            ms[key] = timed(stream, lambda: got.append(call()))
            assert got == [0] and int(counts.sum()) == want, f"{key}: not repaired"
        if r >= warmup:
            for key, v in ms.items():
                t[key].append(v)
    assert all_clean(v_strided) and all_clean(v_ptrs), "stripes do not verify after the repairs"

    nbytes = rows * S

    def row(ts):
        ms = statistics.median(ts)
        return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                "GBps": round(nbytes / ms / 1e6, 1)}

    res = {"code": f"RS({k},{m})", "shard": S, "stripes": st, "bytes": nbytes, "reps": reps, "warmup": warmup,
           "verify_kernel": f.kernel_name(2), "check_kernel": f.kernel_name(10), "column_kernel": f.kernel_name(11),
           "corrupt_stripes": len(bad)}
    res.update({key: row(ts) for key, ts in t.items()})
    ratio = lambda a, b: round(res[a]["ms"] / res[b]["ms"], 4)  # noqa: E731
    res["verify_ptrs_over_strided"] = ratio("verify_ptrs", "verify_stripes")
    res["degraded_ptrs_over_strided"] = ratio("degraded_ptrs", "verify_degraded")
    res["correct_ptrs_over_strided"] = ratio("correct_ptrs", "correct_columns")
    res["verify_route_over_ptrs"] = ratio("verify_route", "verify_ptrs")
    res["degraded_route_over_ptrs"] = ratio("degraded_route", "degraded_ptrs")
    res["correct_route_over_ptrs"] = ratio("correct_route", "correct_ptrs")
    f.close()
    del img, pool, img_w, pool_w
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codes", nargs="+", default=sorted(CODES), choices=sorted(CODES))
    ap.add_argument("--stripes", type=int, default=0, help="stripes (default: the code's)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scrub_ptrs_bench needs the GPU")
    for name in a.codes:
        line = json.dumps(run_code(name, a.stripes, a.reps, a.warmup))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

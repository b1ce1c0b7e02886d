#!/usr/bin/env python3
"""Cost of the pointer-placement I/O calls (rs_encode_ptrs, rs_update_ptrs,
rs_read_ptrs) against (a) the strided call on the same stripes, (b) the
rs_combine route each of them replaces and (c) copy-in, strided call, copy-out;
(d) every strided call is timed twice per round, and the ratio of the two
medians is the run's spread.

For RS(10,4) with 1 MiB shards and RS(64,16) with 64 KiB shards, in one
process: the stripes are encoded once into a dense strided image (data
[stripes][k][S] and parity [stripes][m][S]), then copied shard by shard to the
rows of a pool of the same size in shuffled order; the device table names those
rows.
  encode: every stripe.  Route (b): one rs_combine job per stripe, k sources
          and m destinations.  Route (c): gather the k data shards, encode,
          scatter the m parity shards.
  update: data shard 0 of every stripe (j = 1).  Route (b): a delta rs_combine
          (parity ^= E * (old ^ new), accumulate) and a commit rs_combine.
          Route (c): gather shard 0 and the parity, update, scatter them back.
  read:   data shard 0 of every stripe is missing and wanted (j = 1).  Route
          (b): one rs_combine job per stripe over the pattern's k survivors,
          its row from rs_pattern_rows.  Route (c): gather the k survivors,
          read there.
The host-side marshalling of (b) -- the per-stripe address lists built from a
host copy of the table, which the new calls do not need -- is timed apart with
a host clock and is not part of (b)'s time.  Route (c) gathers and scatters
with torch.index_select / index_copy_ of 8-byte words into dense scratch, one
pass each; scratch slots of shards a call never dereferences are not there.
HIP events around each call on the caller's stream, behind a short spin kernel
so that the call's host work is done before the device gets to it; --warmup
untimed rounds, then the median of --reps; the arms alternate inside one loop.
One JSON line per code, appended to --out when given.

--order identity puts shard (s, i) in pool row s * n + i: the pointer calls then
run on the addresses of a dense image, which separates what the kernels' table
loads cost from what the scattered placement costs.

    python tools/ptrs_io_bench.py [--codes 10_4 64_16] [--order shuffled] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "noise-erasurecode-plugin_amd")
sys.path[:0] = [ROOT, PKG]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CODES = {"10_4": (10, 14, 1 << 20, 1024), "64_16": (64, 80, 65536, 2048)}
GATE_CYCLES = 20_000_000  # the spin kernel in front of a timed call


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(GATE_CYCLES)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def run_code(name, stripes, reps, warmup, order):
    import rsmi

    k, n, S, default_stripes = CODES[name]
    st = stripes or default_stripes
    m, W = n - k, S // 8
    dev = torch.device("cuda", 0)
    f = rsmi.FEC(k, n, device=0)
    E = f.matrix()
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    u8 = lambda rows: torch.empty(rows * S, dtype=torch.uint8, device=dev)  # noqa: E731
    words = lambda t: t.view(torch.int64).view(-1, W)  # noqa: E731
    data, parity, pool = u8(st * k), u8(st * m), u8(st * n)
    new, out = u8(st), u8(st)  # the update's src buffers, the read's dst buffers
    geom = (data.data_ptr(), k * S, parity.data_ptr(), m * S, S, S, st)
    f.fill_splitmix(data.data_ptr(), data.numel(), 0x5C2B, sh)
    f.fill_splitmix(new.data_ptr(), new.numel(), 0x10AD, sh)
    f.encode_stripes(*geom, sh)
    # the pool: shard (s, i) in row perm[s, i]
    rng = np.random.default_rng(0xD1127)
    perm = (rng.permutation(st * n) if order == "shuffled" else np.arange(st * n)).reshape(st, n)
    rows_of = lambda ids: torch.from_numpy(np.ascontiguousarray(perm[:, ids]).reshape(-1)).to(dev)  # noqa: E731
    p_data, p_par, p_zero = rows_of(slice(0, k)), rows_of(slice(k, n)), rows_of(slice(0, 1))
    pool_w, data_w, par_w = words(pool), words(data), words(parity)
    pool_w.index_copy_(0, p_data, data_w)
    pool_w.index_copy_(0, p_par, par_w)
    host_table = pool.data_ptr() + perm.astype(np.int64) * S
    table = torch.from_numpy(host_table.reshape(-1).copy()).to(dev)
    tp = table.data_ptr()
    first_bad = torch.zeros(st, dtype=torch.int32, device=dev)

    def clean(call):
        call()
        stream.synchronize()
        return int((first_bad != -1).sum()) == 0

    v_ptrs = lambda er=None: f.verify_ptrs(tp, S, st, first_bad.data_ptr(), erased=er, stream=sh)  # noqa: E731
    v_strided = lambda: f.verify_stripes(*geom, first_bad.data_ptr(), sh)  # noqa: E731
    assert clean(v_ptrs) and clean(v_strided), "encoded stripes do not verify"

    # ---- the lists of the three calls ----------------------------------------
    upd_ptrs = rsmi.shard_updates([(s, 0, new.data_ptr() + s * S) for s in range(st)])
    rd = rsmi.shard_reads([(s, 0, out.data_ptr() + s * S) for s in range(st)])
    er = np.zeros((st, n), dtype=np.uint8)
    er[:, 0] = 1
    flags = er.tobytes()
    surv = f.pattern_survivors(er[0].tobytes())
    row0, _ = f.pattern_rows(er[0].tobytes())
    row0 = bytes(row0[:k])  # data shard 0 is the pattern's first erased id

    # ---- (b) the rs_combine routes, their marshalling timed apart --------------
    marshal = {}

    def marshalled(key, build):
        t0 = time.perf_counter()
        jobs = build()
        marshal[key] = (time.perf_counter() - t0) * 1e3
        return jobs

    ht = host_table
    enc_jobs = marshalled("encode", lambda: rsmi.combine_jobs(
        [(ht[s, :k].tolist(), ht[s, k:].tolist(), E[k * k:], 0) for s in range(st)]))
    # the delta job's m x 2 coefficients: E[k + r][0] for the old and for the new contents
    col0 = bytes(b for r in range(m) for b in (E[(k + r) * k], E[(k + r) * k]))
    new0 = new.data_ptr()
    upd_jobs = marshalled("update", lambda: (
        rsmi.combine_jobs([([int(ht[s, 0]), new0 + s * S], ht[s, k:].tolist(), col0, 1) for s in range(st)]),
        rsmi.combine_jobs([([new0 + s * S], [int(ht[s, 0])], b"\x01", 0) for s in range(st)])))
    out0 = out.data_ptr()
    read_jobs = marshalled("read", lambda: rsmi.combine_jobs(
        [(ht[s, surv].tolist(), [out0 + s * S], row0, 0) for s in range(st)]))

    # ---- (c) the copy routes: dense scratch for what a call dereferences -------
    # update: shard 0 of stripe s at scratch row s (dss = pitch = S: the slots of
    # shards 1 .. k-1 alias other rows and are never dereferenced)
    # (the scratch buffers cover the whole extent the strided calls check src and dst against)
    zero_s = u8(st + k)
    zero_w = words(zero_s)[:st]
    upd_geom = (zero_s.data_ptr(), S, parity.data_ptr(), m * S, S, S, st)
    upd_strided_list = rsmi.shard_updates([(s, 0, new.data_ptr() + s * S) for s in range(st)])
    # read: the survivors are data 1 .. k-1 and the highest parity; their scratch
    # is dense and the slots of the shards the call never dereferences lie outside it
    assert sorted(surv) == list(range(1, k)) + [n - 1], surv
    sv_d, sv_p = u8(st * (k - 1) + 1)[S:], u8(st + m - 1)[(m - 1) * S:]
    p_sv_d, p_sv_p = rows_of(slice(1, k)), rows_of(slice(n - 1, n))
    read_geom = (sv_d.data_ptr() - S, (k - 1) * S, sv_p.data_ptr() - (m - 1) * S, S, S, S, st)

    def enc_route():
        torch.index_select(pool_w, 0, p_data, out=data_w)
        f.encode_stripes(*geom, sh)
        pool_w.index_copy_(0, p_par, par_w)

    def upd_route():
        torch.index_select(pool_w, 0, p_zero, out=zero_w)
        torch.index_select(pool_w, 0, p_par, out=par_w)
        f.update_stripes(*upd_geom, upd_strided_list, sh)
        pool_w.index_copy_(0, p_zero, zero_w)
        pool_w.index_copy_(0, p_par, par_w)

    def read_route():
        torch.index_select(pool_w, 0, p_sv_d, out=words(sv_d))
        torch.index_select(pool_w, 0, p_sv_p, out=words(sv_p))
        f.read_stripes(*read_geom, flags, rd, sh)

    def upd_combine():
        f.combine(upd_jobs[0], S, sh)
        f.combine(upd_jobs[1], S, sh)

    arms = {
        "encode_ptrs": lambda: f.encode_ptrs(tp, S, st, sh),
        "encode_stripes": lambda: f.encode_stripes(*geom, sh),
        "encode_stripes_again": lambda: f.encode_stripes(*geom, sh),
        "encode_combine": lambda: f.combine(enc_jobs, S, sh),
        "encode_route": enc_route,
        "update_ptrs": lambda: f.update_ptrs(tp, S, st, upd_ptrs, stream=sh),
        "update_stripes": lambda: f.update_stripes(*geom, upd_strided_list, sh),
        "update_stripes_again": lambda: f.update_stripes(*geom, upd_strided_list, sh),
        "update_combine": upd_combine,
        "update_route": upd_route,
        "read_ptrs": lambda: f.read_ptrs(tp, S, st, flags, rd, stream=sh),
        "read_stripes": lambda: f.read_stripes(*geom, flags, rd, sh),
        "read_stripes_again": lambda: f.read_stripes(*geom, flags, rd, sh),
        "read_combine": lambda: f.combine(read_jobs, S, sh),
        "read_route": read_route,
    }
    t = {key: [] for key in arms}
    for r in range(warmup + reps):
        for key, call in arms.items():
            ms = timed(stream, call)
            if r >= warmup:
                t[key].append(ms)
    # the pool and the image hold the updated stripes now, and they are codewords
    assert clean(v_ptrs) and clean(v_strided), "stripes do not verify after the timed calls"
    out.zero_()
    arms["read_stripes"]()
    stream.synchronize()
    ref = out.clone()
    for key in ("read_ptrs", "read_combine", "read_route"):
        out.zero_()
        arms[key]()
        stream.synchronize()
        assert torch.equal(out, ref), f"{key} differs from rs_read_stripes"

    moved = {"encode": (k + m) * S * st, "update": (3 + 2 * m) * S * st, "read": (k + 1) * S * st}

    def row(key):
        ts = t[key]
        ms = statistics.median(ts)
        return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                "GBps": round(moved[key.split("_")[0]] / ms / 1e6, 1)}

    res = {"code": f"RS({k},{m})", "shard": S, "stripes": st, "order": order, "reps": reps, "warmup": warmup,
           "encode_kernel": f.kernel_name(20), "update_kernel": f.kernel_name(21), "read_kernel": f.kernel_name(22),
           "bytes": moved}
    res.update({key: row(key) for key in arms})
    ratio = lambda a, b: round(res[a]["ms"] / res[b]["ms"], 4)  # noqa: E731
    for op, strided in (("encode", "encode_stripes"), ("update", "update_stripes"), ("read", "read_stripes")):
        spread = ratio(strided + "_again", strided)
        res[op + "_spread"] = spread
        res[op + "_ptrs_over_strided"] = ratio(op + "_ptrs", strided)
        res[op + "_ptrs_over_combine"] = ratio(op + "_ptrs", op + "_combine")
        res[op + "_route_over_ptrs"] = ratio(op + "_route", op + "_ptrs")
        res[op + "_combine_marshal_ms"] = round(marshal[op], 3)
        # the one condition: at most the rs_combine route's time, the spread as margin
        res[op + "_within_combine"] = res[op + "_ptrs"]["ms"] <= res[op + "_combine"]["ms"] * max(spread, 1 / spread)
    f.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codes", nargs="+", default=sorted(CODES), choices=sorted(CODES))
    ap.add_argument("--stripes", type=int, default=0, help="stripes (default: the code's)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--order", default="shuffled", choices=("shuffled", "identity"),
                    help="pool rows in shuffled order, or in the strided image's order (the same kernels on the "
                         "same addresses as a dense image: what the placement itself costs)")
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ptrs_io_bench needs the GPU")
    for name in a.codes:
        line = json.dumps(run_code(name, a.stripes, a.reps, a.warmup, a.order))
        print(line, flush=True)
        torch.cuda.empty_cache()
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

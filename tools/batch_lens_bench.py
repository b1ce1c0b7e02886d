#!/usr/bin/env python3
"""What per-job lengths cost, and what they buy.

Part 1, the cost of the per-job block map: rs_combine_lens with every length
equal but forced through the per-job-length twin (RSMI_COMBINE_LENS_FORCE=1,
which this tool sets for its own process) against rs_combine on the same jobs
and buffers -- RS(10,4)-shaped jobs (nsrc 10, nout 4) of 1 MiB and of 64 KiB,
RS(64,16)-shaped jobs (nsrc 64, nout 16) of 64 KiB, enough jobs for 1 GiB
moved.  A third arm runs rs_combine a second time: the spread of that arm
against itself is what the twin's ratio is to be read against.  HIP events
around each call, the arms alternating inside one loop; ratios are taken rep
by rep and reported as min / median / max.

Part 2, what the feature is for: 64 RS(10,4) messages with seeded lengths
uniform between 0.5x and 1.5x of 1,048,580 bytes (rounded to a multiple of
k), encoded and -- with 4 seeded drops per message -- decoded
  * lens:     by one rs_encode_batch_lens / rs_decode_batch_lens call;
  * single:   the way without them, one equal-length call per distinct length,
              which for 64 distinct lengths is one rs_encode / rs_decode each;
  * ceiling:  by rs_encode_batch / rs_decode_batch on 64 equal messages of the
              same total bytes.
Decode runs twice, on pageable shares and on shares in an rs_arena.  Host
clock around the (synchronous) calls, the arms alternating inside one loop;
microseconds per message as min / median / max.  The outputs of the lens and
single arms are compared with each other and with the messages.

Prints one JSON object and writes it to --out.

    python tools/batch_lens_bench.py [--reps 7] [--out profiles/batch_lens/batch_lens_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

os.environ["RSMI_COMBINE_LENS_FORCE"] = "1"  # read once, when the engine first sees a mixed-length combine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "noise-erasurecode-plugin_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

GIB = 1 << 30
COMBINE_SHAPES = [("rs10_4_1MiB", 10, 4, 1 << 20), ("rs10_4_64KiB", 10, 4, 1 << 16), ("rs64_16_64KiB", 64, 16, 1 << 16)]


def spread(xs, digits=4):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits)}


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def combine_cost(f, name, nsrc, nout, length, reps, warmup):
    import rsmi

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    per_job = (nsrc + nout) * length
    njobs = (GIB + per_job - 1) // per_job
    src = torch.empty(njobs * nsrc * length, dtype=torch.uint8, device=dev)
    outs = {arm: torch.zeros(njobs * nout * length, dtype=torch.uint8, device=dev) for arm in ("combine", "lens", "combine_again")}
    f.fill_splitmix(src.data_ptr(), src.numel(), 0xB17C, sh)
    coef = np.random.default_rng(nsrc * 1000 + nout).integers(1, 256, size=nout * nsrc, dtype=np.uint8).tobytes()
    tables = {arm: rsmi.combine_jobs([([src.data_ptr() + (j * nsrc + c) * length for c in range(nsrc)],
                                       [out.data_ptr() + (j * nout + r) * length for r in range(nout)], coef, 0)
                                      for j in range(njobs)]) for arm, out in outs.items()}
    lens = (ctypes.c_size_t * njobs)(*[length] * njobs)  # built once, like the job tables
    arms = {"combine": lambda: f.combine(tables["combine"], length, sh),
            "lens": lambda: f.combine_lens(tables["lens"], lens, sh),
            "combine_again": lambda: f.combine(tables["combine_again"], length, sh)}
    launches0 = f.stat(f.STAT_COMBINE_LENS_LAUNCHES)
    times = {arm: [] for arm in arms}
    for r in range(warmup + reps):
        for arm, fn in arms.items():
            ms = timed(stream, fn)
            if r >= warmup:
                times[arm].append(ms)
    assert f.stat(f.STAT_COMBINE_LENS_LAUNCHES) - launches0 == warmup + reps, "the lens arm did not run the twin"
    stream.synchronize()
    assert torch.equal(outs["combine"], outs["lens"]) and torch.equal(outs["combine"], outs["combine_again"])
    moved = njobs * per_job
    return {"shape": name, "nsrc": nsrc, "nout": nout, "len": length, "jobs": njobs, "bytes": moved,
            "combine_ms": spread(times["combine"]), "lens_ms": spread(times["lens"]),
            "combine_GBps": round(moved / statistics.median(times["combine"]) / 1e6, 1),
            "lens_GBps": round(moved / statistics.median(times["lens"]) / 1e6, 1),
            "lens_over_combine": spread([a / b for a, b in zip(times["lens"], times["combine"])]),
            "combine_over_itself": spread([a / b for a, b in zip(times["combine_again"], times["combine"])])}


def addr(b):
    return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value


class Batch:
    """`count` RS(k, m) messages of the given lengths: inputs, parity buffers,
    and for the decode k survivors each (4 seeded drops), pageable and in an
    arena."""

    def __init__(self, f, lens, seed):
        import rsmi
        from oracle import oracle

        self.f, self.k, self.n, self.lens = f, f.k, f.n, list(lens)
        k, n, B = self.k, self.n, len(lens)
        rng = np.random.default_rng(seed)
        self.inputs = [oracle.splitmix_bytes(length, seed * 100 + b).tobytes() for b, length in enumerate(lens)]
        E = oracle.fec_matrix(k, n)
        self.S = [length // k for length in lens]
        self.keep = [sorted(int(i) for i in rng.permutation(n)[:k]) for _ in lens]
        self.shares, self.parity = [], []
        for inp, S, ids in zip(self.inputs, self.S, self.keep):
            par = oracle.encode(E, k, n, inp)
            allsh = [inp[i * S:(i + 1) * S] for i in range(k)] + [par[i * S:(i + 1) * S] for i in range(n - k)]
            self.shares.append([allsh[i] for i in ids])
            self.parity.append(par)
        self.arena = rsmi.Arena(sum((S + 255) // 256 * 256 * k for S in self.S) + 4096)
        self.ptrs = {"pageable": [[addr(s) for s in sh] for sh in self.shares],
                     "arena": [[self.arena.put(s) for s in sh] for sh in self.shares]}
        self.par_out = [ctypes.create_string_buffer(max(S * (n - k), 1)) for S in self.S]
        self.dec_out = [ctypes.create_string_buffer(max(S * k, 1)) for S in self.S]
        self.c_in = (ctypes.c_void_p * B)(*[addr(x) for x in self.inputs])
        self.c_lens = (ctypes.c_size_t * B)(*lens)
        self.c_par = (ctypes.c_void_p * B)(*[ctypes.addressof(o) for o in self.par_out])
        self.c_dst = (ctypes.c_void_p * B)(*[ctypes.addressof(o) for o in self.dec_out])
        self.c_S = (ctypes.c_size_t * B)(*self.S)
        self.c_counts = (ctypes.c_int * B)(*[k] * B)
        self.c_st = (ctypes.c_int * B)()

    def tables(self, where):
        B, k = len(self.lens), self.k
        nums = (ctypes.c_int * (B * k))(*[i for ids in self.keep for i in ids])
        ptrs = (ctypes.c_void_p * (B * k))(*[p for row in self.ptrs[where] for p in row])
        return nums, ptrs

    def check(self, what):
        for b, (S, par, inp) in enumerate(zip(self.S, self.parity, self.inputs)):
            assert self.par_out[b].raw[:S * (self.n - self.k)] == par, (what, "parity", b)
            assert self.dec_out[b].raw[:S * self.k] == inp, (what, "decode", b)

    def wipe(self):
        for o in self.par_out + self.dec_out:
            ctypes.memset(o, 0, len(o))


def batch_gain(f, reps, warmup, count=64, base=1048580):
    import rsmi

    lib = rsmi.load()
    k = f.k
    rng = np.random.default_rng(0x1E45)
    lens = [int(v) // k * k for v in rng.uniform(0.5 * base, 1.5 * base, size=count)]
    mixed = Batch(f, lens, seed=11)
    equal = Batch(f, [sum(lens) // count // k * k] * count, seed=12)
    h = f.handle

    def enc_lens():
        assert lib.rs_encode_batch_lens(h, count, mixed.c_in, mixed.c_lens, mixed.c_par, mixed.c_st) == 0

    def enc_single():
        for b in range(count):
            assert lib.rs_encode(h, mixed.c_in[b], lens[b], mixed.c_par[b]) == 0

    def enc_ceiling():
        assert lib.rs_encode_batch(h, count, equal.c_in, equal.lens[0], equal.c_par, equal.c_st) == 0

    def decoders(where):
        nums, ptrs = mixed.tables(where)
        enums, eptrs = equal.tables(where)
        vp, ip = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int)

        def dec_lens():
            assert lib.rs_decode_batch_lens(h, count, mixed.c_counts, nums, ptrs, mixed.c_S, mixed.c_dst, mixed.c_st) == 0

        def dec_single():
            for b in range(count):
                assert lib.rs_decode(h, ctypes.cast(ctypes.byref(nums, 4 * b * k), ip), ctypes.cast(ctypes.byref(ptrs, 8 * b * k), vp),
                                     k, mixed.S[b], mixed.c_dst[b]) == 0

        def dec_ceiling():
            assert lib.rs_decode_batch(h, count, equal.c_counts, enums, eptrs, equal.S[0], equal.c_dst, equal.c_st) == 0

        return {"lens": dec_lens, "single": dec_single, "ceiling": dec_ceiling}

    groups = {"encode": {"lens": enc_lens, "single": enc_single, "ceiling": enc_ceiling},
              "decode_pageable": decoders("pageable"), "decode_arena": decoders("arena")}
    # every arm's output, checked once before anything is timed
    for arm in ("lens", "single"):
        mixed.wipe()
        groups["encode"][arm]()
        for where in ("decode_pageable", "decode_arena"):
            groups[where][arm]()
            mixed.check(f"{arm} {where}")
    groups["encode"]["ceiling"]()
    groups["decode_pageable"]["ceiling"]()
    equal.check("ceiling")
    passes0 = f.stat(f.STAT_BATCH_LENS_PASSES)
    res = {"messages": count, "code": f"RS({k},{f.n - k})", "bytes_mixed": sum(lens), "bytes_equal": sum(equal.lens),
           "min_len": min(lens), "max_len": max(lens)}
    for gname, arms in groups.items():
        times = {arm: [] for arm in arms}
        for r in range(warmup + reps):
            for arm, fn in arms.items():
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if r >= warmup:
                    times[arm].append(dt * 1e6 / count)
        row = {arm + "_us_per_msg": spread(ts, 2) for arm, ts in times.items()}
        row["lens_over_single"] = spread([a / b for a, b in zip(times["lens"], times["single"])])
        row["lens_over_ceiling"] = spread([a / b for a, b in zip(times["lens"], times["ceiling"])])
        res[gname] = row
    res["lens_passes"] = f.stat(f.STAT_BATCH_LENS_PASSES) - passes0
    mixed.check("after the timed calls")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", nargs="+", default=["combine", "batch"], choices=["combine", "batch"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_lens", "batch_lens_bench.json"),
                    help="write the JSON object to this file ('' for none)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("batch_lens_bench needs the GPU")
    import rsmi

    f = rsmi.FEC(10, 14, device=0)
    res = {"reps": a.reps, "warmup": a.warmup, "combine_kernel": f.kernel_name(6), "lens_kernel": f.kernel_name(9)}
    if "combine" in a.parts:
        res["combine_cost"] = []
        for shape in COMBINE_SHAPES:
            res["combine_cost"].append(combine_cost(f, *shape, a.reps, a.warmup))
            torch.cuda.empty_cache()
    if "batch" in a.parts:
        res["batch"] = batch_gain(f, a.reps, a.warmup)
    f.close()
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

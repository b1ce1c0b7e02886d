#!/usr/bin/env python3
"""Cost of the column scrub (rs_correct_columns) of device-resident stripes.

For BASELINE config 2 (6,553 stripes x RS(10,4) x 1 MiB shards) and config 5
(16,384 stripes x RS(64,16) x 64 KiB shards), in one process and on the same
buffers:
  1. clean:    rs_correct_columns of consistent stripes against
               rs_verify_stripes (the call is the verify plus one read-back of
               the verdicts when nothing is wrong);
  2. shard:    1% of the stripes with one wholly wrong shard --
               rs_correct_columns against rs_correct_stripes on the same input
               (the arm of scrub_bench.py);
  3. sectors:  1% of the stripes with one 4 KiB wrong run in each of three
               different shards at three different offsets, which the
               shard-level scrub cannot repair -- against arm 1;
  4. host:     the engine's host Berlekamp-Welch (rsmi::bw_column) on single-
               error columns of the same code, timed in a stand-alone C++
               program on one core and scaled to arm 3's column count.
HIP events around each call on the caller's stream (the correct calls are
synchronous, so their host round trips are inside), --warmup untimed calls,
then the median of --reps; the two calls of an arm alternate inside one loop,
and the damage is put back before every timed call.  One JSON line per
config, appended to --out when given.

    python tools/column_scrub_bench.py [--configs 2 5] [--reps 20] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "noise-erasurecode-plugin_amd")
sys.path[:0] = [ROOT, PKG]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CONFIGS = {2: (10, 14, 1 << 20, 6553), 5: (64, 80, 65536, 16384)}
RUN = 4096  # bytes of a bad sector

HOST_PROGRAM = r"""
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gf256.hpp"
int main(int argc, char** argv) {
    const int k = std::atoi(argv[1]), n = std::atoi(argv[2]), columns = std::atoi(argv[3]);
    std::vector<int> nums(n);
    for (int i = 0; i < n; ++i) nums[i] = i;
    std::vector<uint8_t> p(k), y(n), out(n);
    unsigned seed = 12345u, sink = 0;
    auto rnd = [&] { return seed = seed * 1664525u + 1013904223u, seed >> 16; };
    double total = 0;
    for (int c = 0; c < columns; ++c) {
        for (auto& v : p) v = static_cast<uint8_t>(rnd());
        for (int i = 0; i < n; ++i) {
            uint8_t v = 0;
            for (int d = k - 1; d >= 0; --d) v = rsmi::gmul(v, rsmi::eval_point(i)) ^ p[d];
            y[i] = v;
        }
        y[rnd() % n] ^= static_cast<uint8_t>(1 + rnd() % 255);
        const auto t0 = std::chrono::steady_clock::now();
        sink += rsmi::bw_column(k, n, nums.data(), y.data(), n, out.data());
        total += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    std::printf("%.3f %u\n", total / columns * 1e6, sink);
    return sink == static_cast<unsigned>(columns) ? 0 : 1;
}
"""


def host_column_us(k, n, columns):
    """Microseconds per single-error column of rsmi::bw_column on one core."""
    csrc = os.path.join(PKG, "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "bw.cpp"), os.path.join(tmp, "bw")
        with open(src, "w") as fh:
            fh.write(HOST_PROGRAM)
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", csrc, src, os.path.join(csrc, "gf256.cpp"), "-o", exe],
                       check=True)
        out = subprocess.run([exe, str(k), str(n), str(columns)], check=True, capture_output=True, text=True).stdout
    return float(out.split()[0])


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
    verify = lambda: f.verify_stripes(*geom, first_bad.data_ptr(), sh)  # noqa: E731
    # the C ABI itself: the binding's Python lists of stripes * n counts would be inside the timed span
    lib = rsmi.load()
    status = (ctypes.c_int * st)()
    counts = np.zeros(st * n, dtype=np.uint32)
    rewritten = ctypes.create_string_buffer(st * n)
    columns = lambda: lib.rs_correct_columns(f._h, *geom, None, status,  # noqa: E731
                                             counts.ctypes.data_as(ctypes.c_void_p), sh or None)
    shards = lambda: lib.rs_correct_stripes(f._h, *geom, status,  # noqa: E731
                                            ctypes.cast(rewritten, ctypes.c_void_p), sh or None)

    def clean():
        verify()
        stream.synchronize()
        return int((first_bad != -1).sum()) == 0

    assert clean(), "encoded stripes do not verify"

    # 1. clean call against the verify
    for _ in range(warmup):
        verify()
        columns()
    t_verify, t_clean = [], []
    for _ in range(reps):
        t_verify.append(timed(stream, verify))
        t_clean.append(timed(stream, columns))

    rng = np.random.default_rng(0xD1127)
    bad = np.sort(rng.choice(st, size=max(1, st // 100), replace=False))

    def region(s, i, off, length):
        buf, o = (data, s * k * S + i * S) if i < k else (parity, s * m * S + (i - k) * S)
        return buf[o + off:o + off + length]

    # 2. one wholly wrong shard in 1% of the stripes
    shard = rng.integers(0, n, size=len(bad))

    def corrupt_shard():
        for s, i in zip(bad, shard):
            region(int(s), int(i), 0, S).bitwise_xor_(0xA5)

    t_shard_cols, t_shard_stripes = [], []
    for r in range(warmup + reps):
        corrupt_shard()
        got = []
        ms = timed(stream, lambda: got.append(columns()))
        assert got == [0] and int(counts.sum()) == len(bad) * S, "shard: not repaired by rs_correct_columns"
        corrupt_shard()
        got = []
        ms2 = timed(stream, lambda: got.append(shards()))
        assert got == [0], "shard: not repaired by rs_correct_stripes"
        if r >= warmup:
            t_shard_cols.append(ms)
            t_shard_stripes.append(ms2)
    assert clean(), "stripes do not verify after the shard repairs"

    # 3. three bad sectors on three shards at three offsets in 1% of the stripes
    trio = [rng.choice(n, size=3, replace=False) for _ in bad]
    offs = (0, (S // 2) // 16 * 16, S - RUN)

    def corrupt_sectors():
        for s, three in zip(bad, trio):
            for i, off in zip(three, offs):
                region(int(s), int(i), off, RUN).bitwise_xor_(0x3C)

    t_sectors = []
    for r in range(warmup + reps):
        corrupt_sectors()
        got = []
        ms = timed(stream, lambda: got.append(columns()))
        assert got == [0] and int(counts.sum()) == len(bad) * 3 * RUN, "sectors: not repaired"
        if r >= warmup:
            t_sectors.append(ms)
    assert clean(), "stripes do not verify after the sector repairs"

    # 4. the host's Berlekamp-Welch on as many columns, from a sample
    ncols = len(bad) * 3 * RUN
    us = host_column_us(k, n, 4000 if n <= 16 else 200)

    nbytes = (k + m) * S * st

    def row(ts):
        ms = statistics.median(ts)
        return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                "GBps": round(nbytes / ms / 1e6, 1)}

    res = {"config": cfg, "code": f"RS({k},{m})", "shard": S, "stripes": st, "bytes": nbytes, "reps": reps,
           "warmup": warmup, "column_kernel": f.kernel_name(8), "verify_kernel": f.kernel_name(2),
           "corrupt_stripes": len(bad), "sector_columns": ncols,
           "verify": row(t_verify), "columns_clean": row(t_clean),
           "columns_shard": row(t_shard_cols), "correct_stripes_shard": row(t_shard_stripes),
           "columns_sectors": row(t_sectors),
           "host_bw_column_us": round(us, 3), "host_sectors_ms": round(us * ncols / 1e3, 1)}
    res["clean_over_verify"] = round(res["columns_clean"]["ms"] / res["verify"]["ms"], 4)
    res["shard_columns_over_stripes"] = round(res["columns_shard"]["ms"] / res["correct_stripes_shard"]["ms"], 4)
    res["sectors_over_clean"] = round(res["columns_sectors"]["ms"] / res["columns_clean"]["ms"], 4)
    res["host_over_sectors_repair"] = round(
        res["host_sectors_ms"] / max(res["columns_sectors"]["ms"] - res["columns_clean"]["ms"], 1e-3), 1)
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
        sys.exit("column_scrub_bench needs the GPU")
    for cfg in a.configs:
        line = json.dumps(run_config(cfg, a.stripes, a.reps, a.warmup))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of the scrub of device-resident stripes against the encode.

For BASELINE config 2 (6,553 stripes x RS(10,4) x 1 MiB shards) and config 5
(16,384 stripes x RS(64,16) x 64 KiB shards) this times, in one process and on
the same buffers,
  * verify_clean:   rs_verify_stripes of consistent stripes,
  * encode:         rs_encode_stripes of the same stripes (the yardstick: it
                    moves the same (k+m)*S bytes per stripe and does the same
                    GF work; config 5's encode is the bit-sliced network),
  * verify_dirty:   rs_verify_stripes with one wrong byte in 1% of the stripes,
  * correct:        rs_correct_stripes with one wholly wrong shard in 1% of
                    the stripes (verify, gather, locate, reconstruct, verify of
                    the repaired stripes; corrupted again before every call).
HIP events around each call on the caller's stream, --warmup untimed calls,
then the median of --reps; verify_clean and encode alternate inside one loop so
drift of the box hits both alike.  GB/s counts (k+m)*S*stripes bytes; `hbm` is
that over 8 TB/s.  One JSON line per config, appended to --out when given.

    python tools/scrub_bench.py [--configs 2 5] [--reps 20] [--out FILE]
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
    encode = lambda: f.encode_stripes(*geom, sh)  # noqa: E731
    verify = lambda: f.verify_stripes(*geom, first_bad.data_ptr(), sh)  # noqa: E731
    encode()
    verify()
    stream.synchronize()
    assert int((first_bad != -1).sum()) == 0, "encoded stripes do not verify"

    for _ in range(warmup):
        verify()
        encode()
    t_verify, t_encode = [], []
    for _ in range(reps):
        t_verify.append(timed(stream, verify))
        t_encode.append(timed(stream, encode))

    # one wrong byte in 1% of the stripes, in a data or a parity shard
    rng = np.random.default_rng(0xD1127)
    bad = np.sort(rng.choice(st, size=max(1, st // 100), replace=False))
    shard = rng.integers(0, n, size=len(bad))
    off = rng.integers(0, S, size=len(bad))
    dpos = torch.from_numpy(np.array([s * k * S + i * S + o for s, i, o in zip(bad, shard, off) if i < k], dtype=np.int64)).to(dev)
    ppos = torch.from_numpy(np.array([s * m * S + (i - k) * S + o for s, i, o in zip(bad, shard, off) if i >= k], dtype=np.int64)).to(dev)
    data[dpos] ^= 0x5A
    parity[ppos] ^= 0x5A
    for _ in range(warmup):
        verify()
    t_dirty = [timed(stream, verify) for _ in range(reps)]
    stream.synchronize()
    got = first_bad.cpu().numpy().view(np.uint32)
    want = np.full(st, rsmi.RS_VERIFY_CLEAN, dtype=np.uint32)
    want[bad] = off
    assert np.array_equal(got, want), "verify_dirty: wrong verdicts"
    data[dpos] ^= 0x5A
    parity[ppos] ^= 0x5A

    # one wholly wrong shard in the same stripes
    def corrupt():
        for s, i in zip(bad, shard):
            buf, o = (data, s * k * S + i * S) if i < k else (parity, s * m * S + (i - k) * S)
            buf[o:o + S] ^= 0xA5

    t_correct = []
    for r in range(warmup + reps):
        corrupt()
        status = []
        ms = timed(stream, lambda: status.append(f.correct_stripes(*geom, sh)))
        st_list, rw = status[0]
        assert not any(st_list), "correct: a stripe was not repaired"
        assert np.flatnonzero(np.frombuffer(rw, dtype=np.uint8)).tolist() == [int(s) * n + int(i) for s, i in zip(bad, shard)]
        if r >= warmup:
            t_correct.append(ms)
    verify()
    stream.synchronize()
    assert int((first_bad != -1).sum()) == 0, "stripes do not verify after the repairs"

    nbytes = (k + m) * S * st

    def row(ts):
        ms = statistics.median(ts)
        return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                "GBps": round(nbytes / ms / 1e6, 1), "hbm": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}

    res = {"config": cfg, "code": f"RS({k},{m})", "shard": S, "stripes": st, "bytes": nbytes, "reps": reps,
           "warmup": warmup, "verify_kernel": f.kernel_name(2), "encode_kernel": f.kernel_name(0),
           "corrupt_stripes": len(bad),
           "verify_clean": row(t_verify), "encode": row(t_encode), "verify_dirty": row(t_dirty),
           "correct": row(t_correct)}
    res["verify_over_encode"] = round(res["verify_clean"]["ms"] / res["encode"]["ms"], 4)
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
        sys.exit("scrub_bench needs the GPU")
    for cfg in a.configs:
        line = json.dumps(run_config(cfg, a.stripes, a.reps, a.warmup))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

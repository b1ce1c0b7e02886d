#!/usr/bin/env python3
"""Cost of the sector checksums against the codeword verify.

For RS(10,4) with 1 MiB shards and RS(64,16) with 64 KiB shards, and sectors of
512 B, 4 KiB and 64 KiB, this times, in one process and on the same image,
  * verify / verify_again: rs_verify_stripes (it reads the same n * S bytes per
                    stripe; the yardstick, timed twice per round: the ratio of
                    the two is the self-ratio spread every other ratio is judged
                    against),
  * check:          rs_crc32c_check_stripes against stored checksums,
  * check_ptrs:     rs_crc32c_check_ptrs on the same shards through a table,
  * compute:        rs_crc32c_stripes,
  * blake2b:        rs_blake2b_device over the same bytes as 4 KiB messages with
                    32-byte digests -- the hash the engine had before (once per
                    code),
  * host:           rs_crc32c_host on one core over 64 MiB (once),
  * correct_crc / correct_columns (RS(10,4), 4 KiB sectors): rs_correct_crc32c
                    with three wholly wrong shards in 1% of the stripes against
                    rs_correct_columns with one wrong shard in 1% of the stripes
                    (a repair the columns call can make at all); corrupted again
                    before every call.
HIP events around each call on the caller's stream; --warmup untimed rounds,
then --reps rounds in which the legs alternate, so drift of the box hits all of
them alike; medians.  GB/s counts n * S * stripes bytes.  One JSON line per
(code, sector), appended to --out when given.

    python tools/crc_bench.py [--codes rs10_4 rs64_16] [--sectors 512 4096 65536] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "noise-erasurecode-plugin_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

CODES = {"rs10_4": (10, 14, 1 << 20, 1024), "rs64_16": (64, 80, 65536, 4096)}
HBM_PEAK = 8e12  # bytes/s


def timed(stream, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def host_leg():
    import rsmi
    buf = np.random.default_rng(1).integers(0, 256, size=64 << 20, dtype=np.uint8).tobytes()
    rsmi.crc32c_host([buf[:1 << 20]])
    t0 = time.perf_counter()
    rsmi.crc32c_host([buf])
    dt = time.perf_counter() - t0
    return {"bytes": len(buf), "ms": round(dt * 1e3, 3), "GBps": round(len(buf) / dt / 1e9, 3)}


def run_code(name, sectors, stripes, reps, warmup):
    import rsmi

    k, n, S, default_stripes = CODES[name]
    st = stripes or default_stripes
    m = n - k
    dev = torch.device("cuda", 0)
    f = rsmi.FEC(k, n, device=0)
    stream = torch.cuda.current_stream(dev)
    sh = stream.cuda_stream
    data = torch.empty(st * k * S, dtype=torch.uint8, device=dev)
    parity = torch.empty(st * m * S, dtype=torch.uint8, device=dev)
    f.fill_splitmix(data.data_ptr(), data.numel(), 0xC3C, sh)
    geom = (data.data_ptr(), k * S, parity.data_ptr(), m * S, S, S, st)
    f.encode_stripes(*geom, sh)
    vbad = torch.zeros(st, dtype=torch.int32, device=dev)
    cbad = torch.zeros(st * n, dtype=torch.int32, device=dev)
    addr = np.empty((st, n), dtype=np.int64)
    addr[:, :k] = data.data_ptr() + np.arange(st)[:, None] * (k * S) + np.arange(k)[None, :] * S
    addr[:, k:] = parity.data_ptr() + np.arange(st)[:, None] * (m * S) + np.arange(m)[None, :] * S
    table = torch.from_numpy(addr.reshape(-1)).to(dev)
    nbytes = n * S * st
    verify = lambda: f.verify_stripes(*geom, vbad.data_ptr(), sh)  # noqa: E731

    def row(ts):
        ms = statistics.median(ts)
        return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                "GBps": round(nbytes / ms / 1e6, 1), "hbm": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}

    # the alternative that exists today: BLAKE2b of the same bytes as 4 KiB messages
    nmsg = nbytes // 4096
    msg = np.concatenate([data.data_ptr() + np.arange(data.numel() // 4096, dtype=np.int64) * 4096,
                          parity.data_ptr() + np.arange(parity.numel() // 4096, dtype=np.int64) * 4096])
    msg_d = torch.from_numpy(msg).to(dev)
    len_d = torch.full((nmsg,), 4096, dtype=torch.int64, device=dev)
    dig = torch.empty(nmsg * 32, dtype=torch.uint8, device=dev)
    blake = lambda: f.blake2b_device(nmsg, msg_d.data_ptr(), len_d.data_ptr(), 0, 32, dig.data_ptr(), sh)  # noqa: E731
    blake()
    t_blake = [timed(stream, blake) for _ in range(max(3, reps // 2))]
    del msg_d, len_d, dig

    out = []
    for sector in sectors:
        nsec = (S + sector - 1) // sector
        crcs = torch.zeros(st * n * nsec, dtype=torch.int32, device=dev)
        cargs = (sector, crcs.data_ptr(), nsec)
        compute = lambda: f.crc32c_stripes(*geom, *cargs, stream=sh)  # noqa: E731
        check = lambda: f.crc32c_check_stripes(*geom, *cargs, cbad.data_ptr(), stream=sh)  # noqa: E731
        check_ptrs = lambda: f.crc32c_check_ptrs(table.data_ptr(), S, st, *cargs, cbad.data_ptr(), stream=sh)  # noqa: E731
        compute()
        legs = {"verify": verify, "check": check, "verify_again": verify, "check_ptrs": check_ptrs, "compute": compute}
        times = {name_: [] for name_ in legs}
        for r in range(warmup + reps):
            for name_, fn in legs.items():
                ms = timed(stream, fn)
                if r >= warmup:
                    times[name_].append(ms)
        stream.synchronize()
        assert int((vbad != -1).sum()) == 0 and int((cbad != -1).sum()) == 0, "the image does not check clean"
        res = {"code": f"RS({k},{m})", "shard": S, "stripes": st, "sector": sector, "bytes": nbytes, "reps": reps,
               "warmup": warmup, "kernel": f.kernel_name(18), "verify_kernel": f.kernel_name(2)}
        res.update({name_: row(ts) for name_, ts in times.items()})
        res["blake2b_4k"] = row(t_blake)
        for name_ in ("check", "check_ptrs", "compute", "blake2b_4k"):
            res[f"{name_}_over_verify"] = round(res[name_]["ms"] / res["verify"]["ms"], 4)
        res["check_ptrs_over_check"] = round(res["check_ptrs"]["ms"] / res["check"]["ms"], 4)
        res["compute_over_check"] = round(res["compute"]["ms"] / res["check"]["ms"], 4)
        self_r = [b / a for a, b in zip(times["verify"], times["verify_again"])]
        res["self_ratio_spread"] = [round(min(self_r), 4), round(max(self_r), 4)]
        res["check_ratio_per_round"] = [round(b / a, 4) for a, b in zip(times["verify"], times["check"])]

        if name == "rs10_4" and sector == 4096:
            rng = np.random.default_rng(0xC2C)
            bad = np.sort(rng.choice(st, size=max(1, st // 100), replace=False))
            three = [sorted(rng.choice(n, size=3, replace=False).tolist()) for _ in bad]

            def corrupt(count):
                for s, ids in zip(bad, three):
                    for i in ids[:count]:
                        buf, o = (data, s * k * S + i * S) if i < k else (parity, s * m * S + (i - k) * S)
                        buf[o:o + S] ^= 0xA5

            t_crc, t_col = [], []
            for r in range(warmup + reps):
                corrupt(3)
                got = []
                ms = timed(stream, lambda: got.append(f.correct_crc32c(*geom, *cargs, stream=sh)))
                status, rw = got[0]
                assert not any(status), "correct_crc32c: a stripe was not repaired"
                assert int(np.count_nonzero(np.frombuffer(rw, dtype=np.uint8))) == 3 * len(bad)
                corrupt(1)
                got = []
                ms_col = timed(stream, lambda: got.append(f.correct_columns(*geom, stream=sh)))
                assert not any(got[0][0]), "correct_columns: a stripe was not repaired"
                if r >= warmup:
                    t_crc.append(ms)
                    t_col.append(ms_col)
            check()
            verify()
            stream.synchronize()
            assert int((vbad != -1).sum()) == 0 and int((cbad != -1).sum()) == 0, "the repairs left damage"
            res["corrupt_stripes"] = len(bad)
            res["correct_crc"] = row(t_crc)
            res["correct_columns"] = row(t_col)
            res["correct_crc_over_columns"] = round(res["correct_crc"]["ms"] / res["correct_columns"]["ms"], 4)
        out.append(res)
        del crcs
    f.close()
    del data, parity
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codes", nargs="+", default=sorted(CODES), choices=sorted(CODES))
    ap.add_argument("--sectors", type=int, nargs="+", default=[512, 4096, 65536])
    ap.add_argument("--stripes", type=int, default=0, help="stripes (default: the code's)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("crc_bench needs the GPU")
    lines = [{"host_one_core": host_leg()}]
    for name in a.codes:
        lines += run_code(name, a.sectors, a.stripes, a.reps, a.warmup)
    for res in lines:
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""GPU: rs_read_stripes -- degraded read of listed shards of device-resident
stripes into caller buffers, the stripes themselves untouched (rs_read_kernel).

Stripes are laid out with a shard pitch above round_up(shard_len, 16) and
stripe strides with gaps; padding and gaps hold random bytes.  The expected
shard bytes come from the pristine payload and the oracle's parity
(oracle.encode_batch), or, where a survivor is deliberately wrong, from
oracle.reconstruct_batch on a host copy; every comparison is bit-exact.
Before each call the device slots of erased shards are overwritten with fresh
random bytes; after it the whole data and parity buffers must be byte-identical
to before, and so must the guard bytes around every dst -- only the <= 15 bytes
behind shard_len inside a dst are exempt.
"""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

if __name__ == "__main__":  # the RSMI_ITERS child of test_read_multi_iteration_child
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "noise-erasurecode-plugin_amd"), os.path.join(_root, "tests")):
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from oracle import oracle  # noqa: E402

# K10 | K4, m = 2 < MG | K8, m = 6: two row groups | K64 (the reconstruct is
# the syndrome network, the read is not) | runtime k, m = 32: eight row groups
CODES = {"rs10_14": (10, 14), "rs4_6": (4, 6), "rs8_14": (8, 14), "rs64_80": (64, 80), "rs17_49": (17, 49)}
VARIANT = {"rs10_14": "read_K10_MG4_B256", "rs4_6": "read_K4_MG4_B256", "rs8_14": "read_K8_MG4_B256",
           "rs64_80": "read_K64_MG4_B256", "rs17_49": "read_K0_MG4_B256"}
# one column | exactly one 4 KiB block chunk | a chunk plus one column (the
# second block is all tail lanes but one) | not a multiple of 16
SHAPES = [16, 4096, 4112, 5000]
CASES = [(c, S, st) for c in list(CODES) for S in (SHAPES if c != "rs64_80" else [4112, 5000]) for st in (1, 3, 37)]
CODES["rs6_6"] = (6, 6)
SLICE_S = 3 * 4096 + 40
GUARD = 16


def r16(x):
    return (x + 15) // 16 * 16


class Layout:
    """Pristine stripes of one geometry on the host (read-only) with their
    strided device layout."""

    def __init__(self, k, n, S, stripes, seed):
        self.k, self.n, self.m, self.S, self.stripes = k, n, n - k, S, stripes
        self.pitch = r16(S) + 32
        self.dss = k * self.pitch + 48
        self.pss = self.m * self.pitch + 16
        self.E = oracle.fec_matrix(k, n)
        rng = np.random.default_rng(seed)
        self.payload = rng.integers(0, 256, size=(stripes, k, S), dtype=np.uint8)
        self.ref = np.zeros((stripes, 0, S), dtype=np.uint8)
        if self.m:
            flat = np.ascontiguousarray(self.payload).reshape(-1)
            self.ref = oracle.encode_batch(self.E, k, n, flat, S, stripes).reshape(stripes, self.m, S)
        self.data = rng.integers(0, 256, size=stripes * self.dss, dtype=np.uint8)
        self.parity = rng.integers(0, 256, size=stripes * self.pss, dtype=np.uint8)
        for s in range(stripes):
            for i in range(n):
                buf, o = self.at(s, i)
                buf[o:o + S] = self.shard(s, i)
        for a in (self.payload, self.ref, self.data, self.parity):
            a.setflags(write=False)

    def at(self, s, i, data=None, parity=None):
        """(buffer, offset) of shard i of stripe s in the strided layout."""
        if i < self.k:
            return (self.data if data is None else data), s * self.dss + i * self.pitch
        return (self.parity if parity is None else parity), s * self.pss + (i - self.k) * self.pitch

    def shard(self, s, i):
        return self.payload[s, i] if i < self.k else self.ref[s, i - self.k]


_LAYOUTS = {}


def layout(code, S, stripes):
    key = (code, S, stripes)
    if key not in _LAYOUTS:
        k, n = CODES[code]
        _LAYOUTS[key] = Layout(k, n, S, stripes, seed=k * 1000003 + n * 10007 + S * 31 + stripes + 9)
    return _LAYOUTS[key]


_FECS = {}


def fec(code):
    if code not in _FECS:
        _FECS[code] = rsmi.FEC(*CODES[code], device=0)
    return _FECS[code]


def scribbled(L, er, rng, hd=None, hp=None):
    """Host copies of the strided buffers with the slots of the shards that er
    flags overwritten by fresh random bytes."""
    hd = (L.data if hd is None else hd).copy()
    hp = (L.parity if hp is None else hp).copy()
    for s, i in zip(*np.nonzero(er)):
        buf, o = L.at(int(s), int(i), hd, hp)
        buf[o:o + r16(L.S)] = rng.integers(0, 256, size=r16(L.S), dtype=np.uint8)
    return hd, hp


def run_read(f, L, er, wants, seed, hd=None, hp=None, expect=None, off=0, length=None):
    """One rs_read_stripes call: wants = [(stripe, shard)] in the order handed
    to the engine, er = flags [stripes][n], hd / hp = the strided buffers when
    they are not the pristine ones, expect = {(stripe, shard): bytes} where the
    answer is not the pristine shard.  Checks the outputs, the guards, the
    storage and the counters; returns {(stripe, shard): bytes read}."""
    S = L.S if length is None else length
    rng = np.random.default_rng(seed)
    hd, hp = scribbled(L, er, rng, hd, hp)
    dd, dp = torch.from_numpy(hd).cuda(), torch.from_numpy(hp).cuda()
    slot = r16(S) + 2 * GUARD
    out_h = rng.integers(0, 256, size=max(len(wants), 1) * slot, dtype=np.uint8)
    out = torch.from_numpy(out_h.copy()).cuda()
    reads = [(s, i, out.data_ptr() + q * slot + GUARD) for q, (s, i) in enumerate(wants)]
    regen0, copied0 = f.stat(f.STAT_READ_REGENERATED), f.stat(f.STAT_READ_COPIED)
    f.read_stripes(dd.data_ptr() + off, L.dss, dp.data_ptr() + off, L.pss, L.pitch, S, L.stripes, er.tobytes(), reads)
    f.sync()
    assert np.array_equal(dd.cpu().numpy(), hd), "the data region changed"
    assert np.array_equal(dp.cpu().numpy(), hp), "the parity region changed"
    got = out.cpu().numpy()
    res = {}
    for q, (s, i) in enumerate(wants):
        a = q * slot
        assert np.array_equal(got[a:a + GUARD], out_h[a:a + GUARD]), ("guard before", s, i)
        assert np.array_equal(got[a + GUARD + r16(S):a + slot], out_h[a + GUARD + r16(S):a + slot]), ("guard behind", s, i)
        want = expect[(s, i)] if expect and (s, i) in expect else L.shard(s, i)[off:off + S]
        res[(s, i)] = got[a + GUARD:a + GUARD + S].copy()
        bad = np.flatnonzero(res[(s, i)] != want)
        assert bad.size == 0, ("shard", s, i, bool(er[s, i]), bad[:8].tolist(), bad.size)
    missing = sum(1 for s, i in wants if er[s, i])
    assert f.stat(f.STAT_READ_REGENERATED) - regen0 == missing
    assert f.stat(f.STAT_READ_COPIED) - copied0 == len(wants) - missing
    return res


def random_flags(L, rng, lo=1, hi=None):
    """lo..hi (default m) erasures per stripe, anywhere."""
    er = np.zeros((L.stripes, L.n), dtype=np.uint8)
    hi = L.m if hi is None else hi
    for s in range(L.stripes):
        if hi:
            er[s, rng.choice(L.n, size=int(rng.integers(lo, hi + 1)), replace=False)] = 1
    return er


def repaired(f, L, er, seed):
    """The strided buffers after rs_reconstruct_stripes with the same flags."""
    hd, hp = scribbled(L, er, np.random.default_rng(seed))
    dd, dp = torch.from_numpy(hd).cuda(), torch.from_numpy(hp).cuda()
    f.reconstruct_stripes(dd.data_ptr(), L.dss, dp.data_ptr(), L.pss, L.pitch, L.S, L.stripes, er.tobytes())
    f.sync()
    return dd.cpu().numpy(), dp.cpu().numpy()


def check_reads(f, L):
    """Every list of one geometry."""
    k, n, m, stripes = L.k, L.n, L.m, L.stripes
    rng = np.random.default_rng(L.S * 7 + stripes + n)
    # one wanted shard: a missing data shard with e = 1, then a missing parity shard with e = m
    er = np.zeros((stripes, n), dtype=np.uint8)
    s0 = stripes // 2
    er[s0, k - 1] = 1
    run_read(f, L, er, [(s0, k - 1)], seed=1)
    er = np.zeros((stripes, n), dtype=np.uint8)
    er[stripes - 1, rng.choice(n - 1, size=m - 1, replace=False)] = 1
    er[stripes - 1, n - 1] = 1
    run_read(f, L, er, [(stripes - 1, n - 1)], seed=2)
    # all erased shards wanted, 1..m erasures per stripe, stripe 0 with m of
    # them (all row groups): equal to the pristine shards, and to the repair
    er = random_flags(L, rng)
    er[0] = 0
    er[0, rng.choice(n, size=m, replace=False)] = 1
    wants = [(int(s), int(i)) for s, i in zip(*np.nonzero(er))]
    got = run_read(f, L, er, wants, seed=3)
    rd, rp = repaired(f, L, er, seed=4)
    for s, i in wants:
        buf, o = L.at(s, i, rd, rp)
        assert np.array_equal(got[(s, i)], buf[o:o + L.S]), ("read and repair differ", s, i)
    # a mix per stripe, shuffled: missing data, missing parity, present data
    # and the lowest present parity, which Rebuild (data shares first, then
    # the highest-numbered parity) does not choose; odd stripes are not listed
    # and flagged fully erased
    er = np.zeros((stripes, n), dtype=np.uint8)
    wants = []
    for s in range(stripes):
        if s % 2 == 1:
            er[s] = 1
            continue
        gone_d = int(rng.integers(0, k))
        er[s, gone_d] = 1
        wants.append((s, gone_d))
        if m >= 3:  # a missing parity too, and still a parity to spare
            gone_p = k + int(rng.integers(1, m))
            er[s, gone_p] = 1
            wants.append((s, gone_p))
        present_d = (gone_d + 1 + int(rng.integers(0, k - 1))) % k
        wants.append((s, present_d))
        wants.append((s, k))  # present; Rebuild takes one parity here, the highest present one
    wants = [wants[i] for i in rng.permutation(len(wants))]
    run_read(f, L, er, wants, seed=5)
    # random lists over random flags: any shard of any stripe, some stripes twice or not at all
    er = random_flags(L, rng)
    pairs = [(s, i) for s in range(stripes) for i in range(n)]
    wants = [pairs[i] for i in rng.permutation(len(pairs))[:max(1, min(len(pairs) // 3, 80))]]
    run_read(f, L, er, wants, seed=6)


@pytest.mark.parametrize("code", list(VARIANT))
def test_read_variant_names(code):
    assert fec(code).kernel_name(4) == VARIANT[code]
    assert rsmi.FEC.STAT_READ_REGENERATED == 14 and rsmi.FEC.STAT_READ_COPIED == 15


@pytest.mark.parametrize("code,S,stripes", CASES)
def test_read(code, S, stripes):
    check_reads(fec(code), layout(code, S, stripes))


def test_read_six_erasures_all_wanted_take_two_row_groups():
    """RS(8,14), 6 erasures in every stripe, all 6 wanted: rows 4 and 5 are
    the second row group's."""
    L = layout("rs8_14", 4112, 3)
    rng = np.random.default_rng(86)
    er = random_flags(L, rng, lo=6, hi=6)
    run_read(fec("rs8_14"), L, er, [(int(s), int(i)) for s, i in zip(*np.nonzero(er))], seed=1)
    # 5 of the 6: the second group codes one row
    wants = [(int(s), int(i)) for s, i in zip(*np.nonzero(er))]
    run_read(fec("rs8_14"), L, er, [w for q, w in enumerate(wants) if q % 6 != 2], seed=2)


def test_read_without_parity_copies():
    """k = n = 6: every entry is a copy; a wanted erased shard cannot be served."""
    L = layout("rs6_6", 5000, 3)
    f = fec("rs6_6")
    er = np.zeros((3, 6), dtype=np.uint8)
    er[1, 2] = 1
    run_read(f, L, er, [(2, 5), (0, 0), (1, 3), (1, 0)], seed=1)
    out = torch.zeros(r16(L.S), dtype=torch.uint8, device="cuda:0")
    dd, dp = torch.from_numpy(L.data.copy()).cuda(), torch.from_numpy(L.parity.copy()).cuda()
    with pytest.raises(rsmi.NotEnoughShares):
        f.read_stripes(dd.data_ptr(), L.dss, dp.data_ptr(), L.pss, L.pitch, L.S, 3, er.tobytes(), [(1, 2, out.data_ptr())])
    assert not out.any()


def gathered(L, hd, hp):
    """Contiguous [stripes][k][S] and [stripes][m][S] copies of strided buffers."""
    d = np.zeros((L.stripes, L.k, L.S), dtype=np.uint8)
    p = np.zeros((L.stripes, L.m, L.S), dtype=np.uint8)
    for s in range(L.stripes):
        for i in range(L.n):
            buf, o = L.at(s, i, hd, hp)
            (d if i < L.k else p)[s, i if i < L.k else i - L.k] = buf[o:o + L.S]
    return d, p


def test_read_uses_the_survivors_rebuild_chooses():
    """RS(10,4), data 3 and parity 12 missing: Rebuild reads data 0..9 but 3
    and the highest present parity, 13.  A wrong byte in 13 or in data 6 shows
    in the regenerated shards exactly as in the oracle's Rebuild of the
    corrupted stripe; a wrong byte in parity 10 or 11 does not show at all."""
    L = layout("rs10_14", 5000, 3)
    f = fec("rs10_14")
    er = np.zeros((3, 14), dtype=np.uint8)
    er[:, 3] = 1
    er[:, 12] = 1
    wants = [(s, i) for s in range(3) for i in (3, 12)]
    for chosen in (13, 6):
        hd, hp = L.data.copy(), L.parity.copy()
        buf, o = L.at(1, chosen, hd, hp)
        buf[o + 4321] ^= 0xA5
        d, p = gathered(L, hd, hp)
        d[:, 3] = 0
        p[:, 2] = 0
        assert oracle.reconstruct_batch(L.E, 10, 14, d.reshape(-1), p.reshape(-1), L.S, 3, er) == 0
        expect = {(s, 3): d[s, 3] for s in range(3)}
        expect.update({(s, 12): p[s, 2] for s in range(3)})
        assert not np.array_equal(expect[(1, 3)], L.shard(1, 3)) and np.array_equal(expect[(0, 3)], L.shard(0, 3))
        run_read(f, L, er, wants, seed=chosen, hd=hd, hp=hp, expect=expect)
    for unchosen in (10, 11):
        hd, hp = L.data.copy(), L.parity.copy()
        buf, o = L.at(1, unchosen, hd, hp)
        buf[o + 77] ^= 0x3C
        run_read(f, L, er, wants, seed=unchosen, hd=hd, hp=hp)  # expected: the pristine shards


def check_slice(f, L):
    """Bytes [4688, 5688) of the shards -- an offset that is a multiple of 16
    but not of 4096: data / parity advanced by it, shard_len = 1000; pitch and
    strides stay."""
    rng = np.random.default_rng(L.n)
    er = random_flags(L, rng)
    wants = [(int(s), int(i)) for s, i in zip(*np.nonzero(er))] + [(0, int(np.flatnonzero(er[0] == 0)[0]))]
    run_read(f, L, er, wants, seed=12, off=4096 + 37 * 16, length=1000)


@pytest.mark.parametrize("code", ["rs10_14", "rs64_80"])
def test_read_slice(code):
    check_slice(fec(code), layout(code, SLICE_S, 3))


def test_read_refusals_leave_every_dst_alone():
    L = layout("rs10_14", 4112, 3)
    f = fec("rs10_14")
    k, n, S, stripes = L.k, L.n, L.S, L.stripes
    span = r16(S)
    rng = np.random.default_rng(5)
    dd, dp = torch.from_numpy(L.data.copy()).cuda(), torch.from_numpy(L.parity.copy()).cuda()
    out_h = rng.integers(0, 256, size=8 * span, dtype=np.uint8)  # guard-filled
    out = torch.from_numpy(out_h.copy()).cuda()
    op, d0, p0 = out.data_ptr(), dd.data_ptr(), dp.data_ptr()
    er = np.zeros((stripes, n), dtype=np.uint8)
    er[1, [2, 11]] = 1
    er[2, [0, 1, 2, 3, 4]] = 1  # five erasures
    lib = rsmi.load()
    regen0, copied0 = f.stat(f.STAT_READ_REGENERATED), f.stat(f.STAT_READ_COPIED)

    def call(entries, count=None, st=stripes, flags=er, data=d0, length=S):
        arr = None if entries is None else (rsmi.ShardRead * max(len(entries), 1))(*[rsmi.ShardRead(*e) for e in entries])
        buf = ctypes.c_char_p(flags.tobytes()) if flags is not None else None
        return lib.rs_read_stripes(f._h, data, L.dss, p0, L.pss, L.pitch, length, st,
                                   ctypes.cast(buf, ctypes.c_void_p) if buf is not None else None,
                                   arr, len(entries) if count is None else count, None)

    good = (1, 2, 0, op)
    assert call([good, (0, n, 0, op + span)]) == rsmi.RS_EBAD_SHARE_ID
    assert call([good, (stripes, 0, 0, op + span)]) == rsmi.RS_EINVAL
    assert call([good, (0, 1, 0, op + span), (1, 2, 0, op + 2 * span)]) == rsmi.RS_EINVAL  # duplicate
    assert call([good, (0, 1, 0, op + span + 8)]) == rsmi.RS_EINVAL                        # misaligned dst
    assert call([good, (0, 1, 0, 0)]) == rsmi.RS_EINVAL                                    # NULL dst
    assert call([good, (0, 1, 1, op + span)]) == rsmi.RS_EINVAL                            # reserved
    # dst inside the data region, inside the parity region, straddling the data region's end
    assert call([good, (0, 1, 0, d0 + 2 * L.pitch)]) == rsmi.RS_EINVAL
    assert call([good, (0, 1, 0, p0 + L.pss)]) == rsmi.RS_EINVAL
    data_end = d0 + (stripes - 1) * L.dss + (k - 1) * L.pitch + span
    assert call([good, (0, 1, 0, data_end - 16)]) == rsmi.RS_EINVAL
    # two dst ranges that intersect: equal, and one column shared
    assert call([good, (0, 1, 0, op)]) == rsmi.RS_EINVAL
    assert call([(0, 1, 0, op + 2 * span - 16), good, (0, 5, 0, op + span)]) == rsmi.RS_EINVAL
    # more than m erasures and one of them wanted; served when only present shards are
    assert call([good, (2, 4, 0, op + span)]) == rsmi.RS_ENOT_ENOUGH
    # a defect of the list is reported before the erasure count
    assert call([(2, 4, 0, op + span), good, (0, n, 0, op + 2 * span)]) == rsmi.RS_EBAD_SHARE_ID
    assert call([(2, 4, 0, op + span), good, (0, 1, 0, d0)]) == rsmi.RS_EINVAL
    assert call([good], flags=None) == rsmi.RS_EINVAL
    assert call(None, count=1) == rsmi.RS_EINVAL
    assert call([good], data=d0 + 8) == rsmi.RS_EINVAL
    f.sync()
    assert np.array_equal(out.cpu().numpy(), out_h), "a refused call wrote a dst"
    # 2^31 blocks: 4,096 jobs x 2^19 column chunks of 2 GiB shards, and the same as copies (refused
    # before anything is read: the strides are zero and the dsts bare aligned addresses 2 GiB apart)
    big = [(s, 0, 0, 16 + (s << 31)) for s in range(4096)]
    gone = np.zeros((4096, n), dtype=np.uint8)
    gone[:, 0] = 1
    arr = (rsmi.ShardRead * 4096)(*[rsmi.ShardRead(*e) for e in big])
    for flags in (gone, np.zeros((4096, n), dtype=np.uint8)):
        buf = ctypes.c_char_p(flags.tobytes())
        assert lib.rs_read_stripes(f._h, d0, 0, p0, 0, 1 << 31, 1 << 31, 4096, ctypes.cast(buf, ctypes.c_void_p),
                                   arr, 4096, None) == rsmi.RS_EINVAL
    # nothing to do: RS_OK whatever the entries hold
    assert call([(99, 99, 9, 1)], count=0) == rsmi.RS_OK
    assert call([good], st=0) == rsmi.RS_OK
    assert call([good], length=0) == rsmi.RS_OK
    f.sync()
    assert np.array_equal(out.cpu().numpy(), out_h)
    assert np.array_equal(dd.cpu().numpy(), L.data) and np.array_equal(dp.cpu().numpy(), L.parity)
    assert (f.stat(f.STAT_READ_REGENERATED), f.stat(f.STAT_READ_COPIED)) == (regen0, copied0)
    # the stripe with five erasures serves its present shards
    run_read(f, L, er, [(2, 9), (2, 13), (1, 11), (2, 5)], seed=3)


def test_read_shares_the_pattern_cache_with_the_repair():
    L = layout("rs10_14", 4112, 3)
    f = rsmi.FEC(10, 14, device=0)
    er = np.zeros((3, 14), dtype=np.uint8)
    er[0, [2, 7, 11]] = 1
    er[1, [2, 7, 11]] = 1  # not listed
    er[2, [5, 13]] = 1
    count0, tab0 = f.pattern_count(), f.stat(f.STAT_REC_STRIPES_TABLE)
    wants = [(0, 7), (2, 13), (0, 2), (2, 5), (0, 11)]
    got = run_read(f, L, er, wants, seed=1)
    assert f.pattern_count() == count0 + 2, "the read's patterns are not in the ctx's cache"
    rd, rp = repaired(f, L, er, seed=2)
    assert f.pattern_count() == count0 + 2, "the repair built the patterns again"
    assert f.stat(f.STAT_REC_STRIPES_TABLE) == tab0 + 3  # the repair's three stripes: the read is not counted as one
    for s, i in wants:
        buf, o = L.at(s, i, rd, rp)
        assert np.array_equal(got[(s, i)], buf[o:o + L.S]), (s, i)
    f.close()


def test_read_device_set_routes_the_call():
    L = layout("rs10_14", 5000, 3)
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert fs.kernel_name(4) == "read_K10_MG4_B256"
    er = random_flags(L, np.random.default_rng(31))
    wants = [(int(s), int(i)) for s, i in zip(*np.nonzero(er))] + [(1, int(np.flatnonzero(er[1] == 0)[0]))]
    run_read(fs, L, er, wants, seed=21)  # checks the counters summed over the members
    assert fs.stat(fs.STAT_READ_REGENERATED) == len(wants) - 1 and fs.stat(fs.STAT_READ_COPIED) == 1
    fs.close()


def test_read_four_threads_one_context():
    """Four threads share one fresh context; each reads its own erasure
    patterns, new to the cache in every round, so pattern builds, lookups and
    read launches of different callers interleave."""
    L = layout("rs10_14", 4112, 37)
    f = rsmi.FEC(10, 14, device=0)
    errors = []

    def work(t):
        try:
            rng = np.random.default_rng(700 + t)
            for r in range(4):
                er = random_flags(L, rng, lo=2, hi=4)
                wants = [(int(s), int(i)) for s, i in zip(*np.nonzero(er))]
                wants = [wants[i] for i in rng.permutation(len(wants))[:40]] + [(0, int(np.flatnonzero(er[0] == 0)[0]))]
                hd, hp = scribbled(L, er, rng)
                dd, dp = torch.from_numpy(hd).cuda(), torch.from_numpy(hp).cuda()
                span = r16(L.S)
                out = torch.zeros(len(wants) * span, dtype=torch.uint8, device="cuda:0")
                f.read_stripes(dd.data_ptr(), L.dss, dp.data_ptr(), L.pss, L.pitch, L.S, L.stripes, er.tobytes(),
                               [(s, i, out.data_ptr() + q * span) for q, (s, i) in enumerate(wants)])
                f.sync()
                got = out.cpu().numpy()
                for q, (s, i) in enumerate(wants):
                    assert np.array_equal(got[q * span:q * span + L.S], L.shard(s, i)), (t, r, s, i)
                assert np.array_equal(dd.cpu().numpy(), hd) and np.array_equal(dp.cpu().numpy(), hp), (t, r)
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert f.pattern_count() > 100
    f.close()


def test_read_multi_iteration_child():
    """RSMI_ITERS is read once per process: a child with RSMI_ITERS=2 runs the
    lists and the slice read of a several-chunk shape (two column chunks per
    block, the second one's loads issued from inside the loop)."""
    env = dict(os.environ, RSMI_ITERS="2")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "iters child ok" in run.stdout


if __name__ == "__main__":
    assert os.environ.get("RSMI_ITERS") == "2"
    for code in ("rs10_14", "rs8_14", "rs64_80", "rs17_49"):
        check_reads(fec(code), layout(code, SLICE_S, 3))
    check_slice(fec("rs10_14"), layout("rs10_14", SLICE_S, 3))
    check_slice(fec("rs64_80"), layout("rs64_80", SLICE_S, 3))
    print("iters child ok")

"""GPU: rs_update_degraded -- rs_update_stripes for stripes with missing
shards (rs_update_degraded_kernel, and the slow path over the read kernel).

The harness is test_gpu_update's: a shard pitch above round_up(shard_len, 16),
stripe strides with gaps, random bytes in padding and gaps, the expected
parity from the oracle only (oracle.encode_batch over the post-update payload)
and every comparison bit-exact.  Before a call the slots of erased shards are
overwritten with random bytes, so a kernel that reads one gives a wrong
answer, and after the call those slots must be byte-identical.  After a call
the present parity of listed stripes is the oracle's, present changed slots
hold the new bytes and everything else is unchanged; only the <= 15 padding
bytes behind shard_len of rewritten shards are exempt.  On a clone,
rs_reconstruct_stripes with the same flags then yields the oracle's full
stripe -- the new contents of erased changed shards included -- and
rs_verify_degraded finds the present shards on one codeword.
"""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

if __name__ == "__main__":  # the RSMI_ITERS child of test_update_degraded_multi_iteration_child
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "noise-erasurecode-plugin_amd"), os.path.join(_root, "tests")):
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from test_gpu_update import SLICE_S, Dev, fec, layout, r16  # noqa: E402

CLEAN = rsmi.RS_VERIFY_CLEAN
# m = 4: MG4 | m = 2 < MG | m = 6: MG8, partial last row step | m = 16: MG16 |
# m = 28 > 16: the slow path (regenerate, then pairs over two row groups)
VARIANT = {"rs10_14": "update_degraded_MG4_B256", "rs4_6": "update_degraded_MG4_B256",
           "rs8_14": "update_degraded_MG8_B256", "rs64_80": "update_degraded_MG16_B256",
           "rs12_40": "update_degraded_MG16_B256"}
# one column | exactly one 4 KiB block chunk | a chunk plus one column | not a multiple of 16
SHAPES = [16, 4096, 4112, 5000]
CASES = [(c, S, st) for c in VARIANT for S in (SHAPES if c != "rs64_80" else [4112, 5000]) for st in (1, 37)]
SITUATIONS = 8


def situation(L, which, rng):
    """(flags [n], changed shard ids) of one stripe, or (garbage flags, [])
    for a stripe that is not listed."""
    k, m, n = L.k, L.m, L.n
    fl = np.zeros(n, dtype=np.uint8)
    data = [int(i) for i in rng.permutation(k)]
    par = [k + int(r) for r in rng.permutation(m)]
    if which == 0:    # no erasure
        return fl, data[:1]
    if which == 1:    # a parity shard erased, the changed shard present
        fl[par[0]] = 1
        return fl, data[:1]
    if which == 2:    # the changed shard erased, e = 1
        fl[data[0]] = 1
        return fl, data[:1]
    if which == 3:    # the changed shard, another data shard and parity erased, e = m
        fl[data[:2]] = 1
        fl[par[:m - 2]] = 1
        return fl, data[:1]
    if which == 4:    # two changed shards, one present and one erased
        fl[data[0]] = 1
        if m > 2:
            fl[par[0]] = 1
        return fl, data[:2]
    if which == 5:    # all k data shards changed, some of them erased
        fl[data[:2]] = 1
        if m > 2:
            fl[par[0]] = 1
        return fl, data
    if which == 6:    # e = m + 1 > m, only present shards changed: no decode needed
        fl[data[:2]] = 1
        fl[par[:m - 1]] = 1
        return fl, data[2:4]
    fl[:] = 0xFF      # not listed: its flags are never looked at
    return fl, []


class DDev(Dev):
    """Dev with erasure flags: the slots of erased shards hold random bytes."""

    def __init__(self, L, flags, seed):
        super().__init__(L)
        self.flags = flags
        self.listed = np.zeros(L.stripes, dtype=bool)
        rng = np.random.default_rng(seed)
        for s in range(L.stripes):
            if flags[s].all():  # the unlisted stripe's garbage: nothing is missing there
                continue
            for i in np.flatnonzero(flags[s]):
                want, o = (self.want_d, s * L.dss + i * L.pitch) if i < L.k else \
                    (self.want_p, s * L.pss + (i - L.k) * L.pitch)
                want[o:o + r16(L.S)] = rng.integers(0, 256, size=r16(L.S), dtype=np.uint8)
        self.data = torch.from_numpy(self.want_d.copy()).cuda()
        self.parity = torch.from_numpy(self.want_p.copy()).cuda()

    def update(self, f, updates, seed, off=0, length=None):
        """Dev.update through rs_update_degraded.  off / length: a slice
        update of bytes [off, off + length) of the shards."""
        L = self.L
        ln = L.S if length is None else length
        slot = r16(ln) + 16
        rng = np.random.default_rng(seed)
        src_h = rng.integers(0, 256, size=max(len(updates), 1) * slot, dtype=np.uint8)
        src = torch.from_numpy(src_h.copy()).cuda()
        calls = [(s, i, src.data_ptr() + q * slot) for q, (s, i) in enumerate(updates)]
        f.update_degraded(self.data.data_ptr() + off, L.dss, self.parity.data_ptr() + off, L.pss, L.pitch, ln,
                          L.stripes, self.flags.tobytes(), calls)
        f.sync()
        assert np.array_equal(src.cpu().numpy(), src_h), "the src buffers changed"
        # A slice's coded bytes run to round_up(length, 16): inside the shard
        # for a slice, so the model takes them; padding for a whole shard.
        take = ln if length is None else r16(ln)
        for q, (s, i) in enumerate(updates):
            self.payload[s, i, off:off + take] = src_h[q * slot:q * slot + take]
            self.listed[s] = True
        touched = sorted({s for s, _ in updates})
        ref = L.encode(self.payload[touched])
        for s, i in updates:
            if self.flags[s, i]:
                continue  # absorbed: the slot is not written
            o = s * L.dss + i * L.pitch
            self.want_d[o:o + L.S] = self.payload[s, i]
            if length is None:
                self.loose_d[o + L.S:o + r16(L.S)] = True
        for t, s in enumerate(touched):
            for r in range(L.m):
                if self.flags[s, L.k + r]:
                    continue
                o = s * L.pss + r * L.pitch
                self.want_p[o:o + L.S] = ref[t, r]
                if length is None:
                    self.loose_p[o + L.S:o + r16(L.S)] = True

    def check_repair(self, f):
        """The stripes a repair can serve (at most m erasures, listed flags):
        rs_verify_degraded is clean on the device state as it is, and on a
        clone rs_reconstruct_stripes yields the oracle's full stripes."""
        L = self.L
        fl = (self.flags != 0).astype(np.uint8)
        ok = np.array([not self.flags[s].all() and fl[s].sum() <= L.m for s in range(L.stripes)])
        fl[~ok] = 0
        fb = torch.zeros(L.stripes, dtype=torch.int32, device="cuda:0")
        f.verify_degraded(*self.args(), fl.tobytes(), fb.data_ptr())
        f.sync()
        got = fb.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[ok], np.full(int(ok.sum()), CLEAN, dtype=np.uint32)), got.tolist()
        data, parity = self.data.clone(), self.parity.clone()
        f.reconstruct_stripes(data.data_ptr(), L.dss, parity.data_ptr(), L.pss, L.pitch, L.S, L.stripes, fl.tobytes())
        f.sync()
        hd, hp = data.cpu().numpy(), parity.cpu().numpy()
        ref = L.encode(self.payload)
        for s in np.flatnonzero(ok):
            gd = hd[s * L.dss:s * L.dss + L.k * L.pitch].reshape(L.k, L.pitch)[:, :L.S]
            gp = hp[s * L.pss:s * L.pss + L.m * L.pitch].reshape(L.m, L.pitch)[:, :L.S]
            assert np.array_equal(gd, self.payload[s]), ("reconstructed data", int(s))
            assert np.array_equal(gp, ref[s]), ("reconstructed parity", int(s))


def plan_call(L, base, seed):
    """Flags and the shuffled update list of one call: stripe s is in
    situation (s + base) % 8."""
    rng = np.random.default_rng(seed)
    flags = np.zeros((L.stripes, L.n), dtype=np.uint8)
    ups = []
    for s in range(L.stripes):
        flags[s], shards = situation(L, (s + base) % SITUATIONS, rng)
        ups += [(s, i) for i in shards]
    return flags, [ups[i] for i in rng.permutation(len(ups))]


def check_call(f, L, base, seed):
    flags, ups = plan_call(L, base, seed)
    d = DDev(L, flags, seed + 1)
    deg0, abs0, upd0 = (f.stat(x) for x in (f.STAT_UPDATE_DEGRADED, f.STAT_UPDATE_ABSORBED, f.STAT_UPDATE_STRIPES))
    if not ups:  # a single unlisted stripe: nothing to do
        return
    d.update(f, ups, seed + 2)
    d.check(f"base {base}")
    listed = {s for s, _ in ups}
    degraded = any(flags[s].any() for s in listed)
    assert f.stat(f.STAT_UPDATE_DEGRADED) - deg0 == (len(listed) if degraded else 0)
    assert f.stat(f.STAT_UPDATE_STRIPES) - upd0 == (0 if degraded else len(listed))
    assert f.stat(f.STAT_UPDATE_ABSORBED) - abs0 == sum(int(flags[s, i] != 0) for s, i in ups)
    d.check_repair(f)
    return d


@pytest.mark.parametrize("code", list(VARIANT))
def test_update_degraded_variant_names(code):
    assert fec(code).kernel_name(7) == VARIANT[code]


@pytest.mark.parametrize("code,S,stripes", CASES)
def test_update_degraded(code, S, stripes):
    L = layout(code, S, stripes)
    # one stripe: a call per situation; 37: every situation in one call, four or five times over
    for base in (range(SITUATIONS - 1) if stripes == 1 else [0]):
        check_call(fec(code), L, base, seed=S + 100 * base + stripes)


def test_update_degraded_without_flags_is_update_stripes():
    L = layout("rs10_14", 4112, 3)
    f = fec("rs10_14")
    flags = np.zeros((3, L.n), dtype=np.uint8)
    flags[1] = 0xFF  # not listed
    d = DDev(L, flags, 5)
    deg0, upd0 = f.stat(f.STAT_UPDATE_DEGRADED), f.stat(f.STAT_UPDATE_STRIPES)
    d.update(f, [(2, 9), (0, 0), (2, 1)], seed=6)
    d.check("no flags")
    assert f.stat(f.STAT_UPDATE_DEGRADED) == deg0 and f.stat(f.STAT_UPDATE_STRIPES) == upd0 + 2
    # rs_update_stripes' result: the same call through it gives the same bytes
    e = Dev(L)
    e.update(f, [(2, 9), (0, 0), (2, 1)], seed=6)
    assert torch.equal(d.data, e.data) and torch.equal(d.parity, e.parity)


def test_update_degraded_refusals_leave_memory_alone():
    L = layout("rs10_14", 4112, 3)
    f = fec("rs10_14")
    flags = np.zeros((3, L.n), dtype=np.uint8)
    flags[0, [1, 5, 11]] = 1             # e = 3
    flags[2, [0, 3, 10, 12, 13]] = 1     # e = 5 > m
    d = DDev(L, flags, 9)
    src = torch.zeros(4 * (r16(L.S) + 16), dtype=torch.uint8, device="cuda:0")
    sp = src.data_ptr()
    dp, dss, pp, pss, pitch, S, stripes = d.args()
    lib = rsmi.load()
    stats = (f.STAT_UPDATE_DEGRADED, f.STAT_UPDATE_ABSORBED, f.STAT_UPDATE_STRIPES)
    before = [f.stat(x) for x in stats]
    fbuf = flags.tobytes()

    def call(entries, count=None, st=stripes, fl=fbuf):
        arr = (rsmi.ShardUpdate * max(len(entries), 1))(*[rsmi.ShardUpdate(*e) for e in entries])
        return lib.rs_update_degraded(f._h, dp, dss, pp, pss, pitch, S, st, fl, arr,
                                      len(entries) if count is None else count, None)

    good = (0, 1, 0, sp)        # an erased changed shard of a repairable stripe
    many = (2, 3, 0, sp + 8192)  # an erased changed shard of the stripe with e > m
    assert call([good, many]) == rsmi.RS_ENOT_ENOUGH
    assert call([many]) == rsmi.RS_ENOT_ENOUGH
    assert call([good], fl=None) == rsmi.RS_EINVAL  # NULL erased
    # the inherited refusals, each ahead of the stripe with too many erasures
    assert call([good, many, (1, L.k, 0, sp + 16384)]) == rsmi.RS_EBAD_SHARE_ID
    assert call([good, many, (stripes, 0, 0, sp + 16384)]) == rsmi.RS_EINVAL
    assert call([good, many, (0, 1, 0, sp + 16384)]) == rsmi.RS_EINVAL       # duplicate
    assert call([good, many, (1, 1, 0, sp + 8)]) == rsmi.RS_EINVAL           # misaligned src
    assert call([good, many, (1, 1, 0, 0)]) == rsmi.RS_EINVAL                # NULL src
    assert call([good, many, (1, 1, 1, sp + 16384)]) == rsmi.RS_EINVAL       # reserved
    assert call([good, many, (1, 1, 0, dp + 2 * pitch)]) == rsmi.RS_EINVAL   # src in the data region
    assert call([good, many, (1, 1, 0, pp + pss)]) == rsmi.RS_EINVAL         # ... in the parity region
    assert lib.rs_update_degraded(f._h, dp, dss, pp, pss, pitch, S, stripes, fbuf, None, 1, None) == rsmi.RS_EINVAL
    assert lib.rs_update_degraded(f._h, dp + 8, dss, pp, pss, pitch, S, stripes, fbuf,
                                  (rsmi.ShardUpdate * 1)(rsmi.ShardUpdate(*good)), 1, None) == rsmi.RS_EINVAL
    # 2^31 blocks (refused before anything is read: strides zero, src a bare aligned address)
    big = (rsmi.ShardUpdate * 4096)(*[rsmi.ShardUpdate(s, 0, 0, 16) for s in range(4096)])
    bigf = bytes([0] * 13 + [1]) * 4096
    assert lib.rs_update_degraded(f._h, dp, 0, pp, 0, 1 << 31, 1 << 31, 4096, bigf, big, 4096, None) == rsmi.RS_EINVAL
    # nothing to do: RS_OK whatever the entries and the flags hold
    assert call([(99, 99, 9, 1)], count=0) == rsmi.RS_OK
    assert call([good], st=0) == rsmi.RS_OK
    assert lib.rs_update_degraded(f._h, dp, dss, pp, pss, pitch, 0, stripes, fbuf,
                                  (rsmi.ShardUpdate * 1)(rsmi.ShardUpdate(*good)), 1, None) == rsmi.RS_OK
    f.sync()
    d.check("refusals")  # byte-identical: nothing is loose
    assert [f.stat(x) for x in stats] == before


def test_update_degraded_without_parity():
    """RS(4,4), m = 0: present changed shards are overwritten, an erased one
    cannot be absorbed anywhere."""
    k, S, stripes = 4, 5000, 3
    pitch, dss = r16(S) + 32, 4 * (r16(S) + 32) + 48
    f = rsmi.FEC(k, k, device=0)
    rng = np.random.default_rng(45)
    host = rng.integers(0, 256, size=stripes * dss, dtype=np.uint8)
    src_h = rng.integers(0, 256, size=2 * pitch, dtype=np.uint8)
    data, src = torch.from_numpy(host.copy()).cuda(), torch.from_numpy(src_h.copy()).cuda()
    flags = np.zeros((stripes, k), dtype=np.uint8)
    flags[2, 0] = 1
    with pytest.raises(rsmi.RSError) as ei:
        f.update_degraded(data.data_ptr(), dss, 0, 0, pitch, S, stripes, flags.tobytes(), [(2, 0, src.data_ptr())])
    assert ei.value.code == rsmi.RS_ENOT_ENOUGH
    ups = [(2, 3, src.data_ptr()), (0, 1, src.data_ptr() + pitch)]
    f.update_degraded(data.data_ptr(), dss, 0, 0, pitch, S, stripes, flags.tobytes(), ups)
    f.sync()
    want = host.copy()
    for q, (s, i, _) in enumerate(ups):
        o = s * dss + i * pitch
        want[o:o + r16(S)] = src_h[q * pitch:q * pitch + r16(S)]
    assert np.array_equal(data.cpu().numpy(), want)
    f.close()


def test_update_degraded_keeps_a_wrong_parity_byte_wrong_by_the_same_difference():
    """The stored parity is trusted: an XOR mask in a present parity shard
    that is not one of the survivors is the exact difference from the oracle
    afterwards, and nothing else differs."""
    L = layout("rs10_14", 5000, 3)
    f = fec("rs10_14")
    flags = np.zeros((3, L.n), dtype=np.uint8)
    flags[1, 4] = 1  # survivors: the nine other data shards and parity row 3 (the highest id)
    assert f.pattern_survivors(bytes(flags[1])) == [0, 1, 2, 3, 13, 5, 6, 7, 8, 9]
    d = DDev(L, flags, 12)
    at = 1 * L.pss + 1 * L.pitch + 1234
    mask = np.frombuffer(bytes([0x5A, 0x01, 0xFF, 0x80]), dtype=np.uint8)
    d.parity[at:at + 4] ^= torch.from_numpy(mask.copy()).cuda()
    d.update(f, [(1, 4), (1, 7), (2, 0)], seed=3)
    d.want_p[at:at + 4] ^= mask
    d.check("trusted parity")


def test_update_degraded_slice():
    """Bytes [4096, 5096) of the shards: data / parity advanced by 4096,
    shard_len = 1000; pitch and strides stay."""
    for code in ("rs10_14", "rs12_40"):
        L = layout(code, SLICE_S, 3)
        f = fec(code)
        flags = np.zeros((3, L.n), dtype=np.uint8)
        flags[1, [3, L.k + 1]] = 1
        flags[2, [0, 2]] = 1
        d = DDev(L, flags, 31)
        d.update(f, [(1, 3), (2, 0), (1, L.k - 1), (2, 1)], seed=77, off=4096, length=1000)
        d.check(f"slice {code}")  # no loose bytes: nothing outside [4096, 4096 + 1008) of rewritten shards may change
        d.check_repair(f)


def test_update_degraded_wide_jobs_cross_the_lds_threshold():
    """RS(200,216): the tables of k + j sources pass the LDS for every j, so a
    call with an erased changed shard takes the slow path; one without stays
    on the kernel's pair form however wide."""
    L = layout("rs200_216", 4112, 2)
    f = fec("rs200_216")
    assert f.kernel_name(7) == "update_degraded_MG16_B256"
    rng = np.random.default_rng(8)
    flags = np.zeros((2, L.n), dtype=np.uint8)
    flags[0, [7, 100, 203]] = 1
    flags[1, [0, 199, 201, 215]] = 1
    d = DDev(L, flags, 4)
    wide = [int(i) for i in rng.permutation(200)[:150] if i not in (7, 100)]
    d.update(f, [(0, i) for i in wide] + [(0, 7), (0, 100), (1, 199)], seed=1)
    d.check("slow path, wide job")
    d.update(f, [(1, int(i)) for i in range(1, 199)], seed=2)  # j = 198, all present
    d.check("pair form, j = 198")
    d.check_repair(f)


def test_update_degraded_device_set_routes_the_call():
    L = layout("rs10_14", 5000, 3)
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert fs.kernel_name(7) == "update_degraded_MG4_B256"
    flags = np.zeros((3, L.n), dtype=np.uint8)
    flags[0, [2, 12]] = 1
    flags[2, 9] = 1
    d = DDev(L, flags, 21)
    d.update(fs, [(2, 9), (0, 0), (2, 1), (0, 2)], seed=22)
    d.check("device set")
    assert fs.stat(fs.STAT_UPDATE_DEGRADED) == 2 and fs.stat(fs.STAT_UPDATE_ABSORBED) == 2
    d.check_repair(fs)
    fs.close()


def test_update_degraded_four_threads_one_context():
    """Four threads share one context; each patches its own degraded layout
    six times over.  An absorbed shard stays erased, so the next round
    regenerates the previous round's new contents as its old ones."""
    L = layout("rs10_14", 4112, 37)
    f = fec("rs10_14")
    devs, lists = [], []
    for t in range(4):
        flags, ups = plan_call(L, t, seed=500 + t)
        devs.append(DDev(L, flags, 600 + t))
        lists.append(ups)
    errors = []

    def work(t):
        try:
            for r in range(6):
                devs[t].update(f, lists[t], seed=1000 + 10 * t + r)
                devs[t].check(f"thread {t} round {r}")
            devs[t].check_repair(f)
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_update_degraded_multi_iteration_child():
    """RSMI_ITERS is read once per process: a child with RSMI_ITERS=2 runs the
    situations at a several-chunk shape (two column chunks per block: the
    second one's loads are issued from inside the loop, next to the in-place
    stores of the first)."""
    env = dict(os.environ, RSMI_ITERS="2")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "iters child ok" in run.stdout


if __name__ == "__main__":
    assert os.environ.get("RSMI_ITERS") == "2"
    for _code in ("rs10_14", "rs8_14", "rs64_80", "rs12_40"):
        check_call(fec(_code), layout(_code, SLICE_S, 9), 0, seed=17)
    print("iters child ok")

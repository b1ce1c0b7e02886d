"""GPU: rs_update_stripes -- overwrite data shards of device-resident stripes
and patch the stored parity in place from old ^ new (rs_update_kernel).

Stripes are laid out with a shard pitch above round_up(shard_len, 16) and
stripe strides with gaps; padding and gaps hold random bytes.  The expected
parity always comes from the oracle (oracle.encode_batch over the post-update
payload), never from the engine, and every comparison is bit-exact: after a
call the updated shards hold the new bytes, the parity of updated stripes is
the oracle's, and everything else -- untouched stripes and shards, pitch and
stride gaps -- is byte-identical to before; only the <= 15 padding bytes behind
shard_len of rewritten shards are exempt.
"""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

if __name__ == "__main__":  # the RSMI_ITERS child of test_update_multi_iteration_child
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "noise-erasurecode-plugin_amd"), os.path.join(_root, "tests")):
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from oracle import oracle  # noqa: E402

CLEAN = rsmi.RS_VERIFY_CLEAN
# m = 4: MG4 | m = 2 < MG | m = 6: MG8, partial last row step | m = 28: two row
# groups of 16, so the copy commit | m = 16: MG16
CODES = {"rs10_14": (10, 14), "rs4_6": (4, 6), "rs8_14": (8, 14), "rs12_40": (12, 40), "rs64_80": (64, 80)}
VARIANT = {"rs10_14": "update_MG4_B256", "rs4_6": "update_MG4_B256", "rs8_14": "update_MG8_B256",
           "rs12_40": "update_MG16_B256", "rs64_80": "update_MG16_B256"}
COPY_COMMIT = {"rs12_40"}
# one column | exactly one 4 KiB block chunk | a chunk plus one column (the
# second block is all tail lanes but one) | not a multiple of 16
SHAPES = [16, 4096, 4112, 5000]
CASES = [(c, S, st) for c in list(CODES) for S in (SHAPES if c != "rs64_80" else [4112, 5000]) for st in (1, 3, 37)]
# The widest jobs: 195 changed shards are the most whose tables fit the LDS
# with row groups of 16 (195 * 336 = 65,520 bytes); 196 and more take row
# groups of 8, two per stripe for m = 16, and so the copy commit.
CODES["rs200_216"] = (200, 216)
SLICE_S = 3 * 4096 + 40


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
        ref = self.encode(self.payload)
        self.data = rng.integers(0, 256, size=stripes * self.dss, dtype=np.uint8)
        self.parity = rng.integers(0, 256, size=stripes * self.pss, dtype=np.uint8)
        for s in range(stripes):
            for i in range(k):
                o = s * self.dss + i * self.pitch
                self.data[o:o + S] = self.payload[s, i]
            for i in range(self.m):
                o = s * self.pss + i * self.pitch
                self.parity[o:o + S] = ref[s, i]
        for a in (self.payload, self.data, self.parity):
            a.setflags(write=False)

    def encode(self, payload):
        """The oracle's parity [stripes][m][S] of payload [stripes][k][S]."""
        st, _, S = payload.shape
        flat = np.ascontiguousarray(payload).reshape(-1)
        return oracle.encode_batch(self.E, self.k, self.n, flat, S, st).reshape(st, self.m, S)


_LAYOUTS = {}


def layout(code, S, stripes):
    key = (code, S, stripes)
    if key not in _LAYOUTS:
        k, n = CODES[code]
        _LAYOUTS[key] = Layout(k, n, S, stripes, seed=k * 1000003 + n * 10007 + S * 31 + stripes + 5)
    return _LAYOUTS[key]


_FECS = {}


def fec(code):
    if code not in _FECS:
        _FECS[code] = rsmi.FEC(*CODES[code], device=0)
    return _FECS[code]


class Dev:
    """Device clones of a layout, a host model of what they must hold, and the
    update call."""

    def __init__(self, L):
        self.L = L
        self.data = torch.from_numpy(L.data.copy()).cuda()
        self.parity = torch.from_numpy(L.parity.copy()).cuda()
        self.want_d, self.want_p = L.data.copy(), L.parity.copy()  # expected device bytes
        self.payload = L.payload.copy()                            # expected shard bytes [0, S)
        self.loose_d = np.zeros(len(self.want_d), dtype=bool)      # padding bytes behind shard_len of
        self.loose_p = np.zeros(len(self.want_p), dtype=bool)      # rewritten shards: not compared

    def args(self):
        L = self.L
        return (self.data.data_ptr(), L.dss, self.parity.data_ptr(), L.pss, L.pitch, L.S, L.stripes)

    def update(self, f, updates, seed):
        """updates = [(stripe, shard)] in the order handed to the engine; the
        new contents are random, each src a 16-byte aligned slot of one device
        buffer with random bytes around and behind the shard_len bytes."""
        L = self.L
        slot = r16(L.S) + 16
        rng = np.random.default_rng(seed)
        src_h = rng.integers(0, 256, size=max(len(updates), 1) * slot, dtype=np.uint8)
        src = torch.from_numpy(src_h.copy()).cuda()
        calls = [(s, i, src.data_ptr() + q * slot) for q, (s, i) in enumerate(updates)]
        f.update_stripes(*self.args(), calls)
        f.sync()
        assert np.array_equal(src.cpu().numpy(), src_h), "the src buffers changed"
        for q, (s, i) in enumerate(updates):
            self.payload[s, i] = src_h[q * slot:q * slot + L.S]
        touched = sorted({s for s, _ in updates})
        ref = L.encode(self.payload[touched])
        for s, i in updates:
            o = s * L.dss + i * L.pitch
            self.want_d[o:o + L.S] = self.payload[s, i]
            self.loose_d[o + L.S:o + r16(L.S)] = True
        for t, s in enumerate(touched):
            for r in range(L.m):
                o = s * L.pss + r * L.pitch
                self.want_p[o:o + L.S] = ref[t, r]
                self.loose_p[o + L.S:o + r16(L.S)] = True
        return src_h, slot

    def check(self, what=""):
        for got_t, want, loose, name in ((self.data, self.want_d, self.loose_d, "data"),
                                         (self.parity, self.want_p, self.loose_p, "parity")):
            got = got_t.cpu().numpy()
            bad = np.flatnonzero((got != want) & ~loose)
            assert bad.size == 0, (what, name, bad[:8].tolist(), bad.size)

    def verify(self, f):
        fb = torch.zeros(self.L.stripes, dtype=torch.int32, device="cuda:0")
        f.verify_stripes(*self.args(), fb.data_ptr())
        f.sync()
        return fb.cpu().numpy().view(np.uint32)


def check_updates(f, L, copy_commit):
    """Every update set of one geometry, applied one after another to the same
    device clones (each call starts from clean stripes: the previous result)."""
    k, stripes = L.k, L.stripes
    d = Dev(L)
    rng = np.random.default_rng(L.S * 7 + stripes)
    patched0, copies0 = f.stat(f.STAT_UPDATE_STRIPES), f.stat(f.STAT_UPDATE_COPY_COMMITS)
    calls = patched = 0

    def run(updates, what):
        nonlocal calls, patched
        d.update(f, updates, seed=calls + 11)
        d.check(what)
        calls += 1
        patched += len({s for s, _ in updates})

    # one shard in one stripe: first, last and a middle id
    for j, shard in enumerate((0, k - 1, k // 2)):
        run([((stripes - 1) * (j + 1) // 3, shard)], f"one shard {shard}")
    # one shard in every stripe
    run([(s, int(rng.integers(0, k))) for s in range(stripes)], "every stripe")
    # j = 2 and j = k in the same call, shuffled, interleaved with other stripes' entries
    ups = [(0, int(i)) for i in range(k)]
    if stripes > 1:
        ups += [(1, int(i)) for i in rng.choice(k, size=min(2, k), replace=False)]
        ups += [(s, int(rng.integers(0, k))) for s in range(2, stripes, 5)]
    else:
        run([(0, int(i)) for i in rng.choice(k, size=2, replace=False)], "j = 2")
    run([ups[i] for i in rng.permutation(len(ups))], "j = 2 and j = k")
    # j = k replaced the whole payload of stripe 0: its parity is a fresh encode
    # (d.check compared it with the oracle's encode of exactly those k shards)
    assert np.array_equal(d.verify(f), np.full(stripes, CLEAN, dtype=np.uint32)), "updated stripes do not verify"
    # an update and its inverse restore the parity bytes [0, S)
    before_p, before_payload = d.want_p.copy(), d.payload.copy()
    inv = [(stripes // 2, k - 1)] + ([(0, 0), (0, 1)] if k > 1 else [])
    src_h, slot = d.update(f, inv, seed=99)
    d.check("forward")
    assert not np.array_equal(d.want_p, before_p)
    old = torch.from_numpy(np.concatenate([np.concatenate([before_payload[s, i], np.zeros(slot - L.S, dtype=np.uint8)])
                                           for s, i in inv])).cuda()
    f.update_stripes(*d.args(), [(s, i, old.data_ptr() + q * slot) for q, (s, i) in enumerate(inv)])
    f.sync()
    calls, patched = calls + 2, patched + 2 * len({s for s, _ in inv})
    d.payload, d.want_p = before_payload, before_p
    for s, i in inv:
        o = s * L.dss + i * L.pitch
        d.want_d[o:o + L.S] = before_payload[s, i]
    d.check("inverse")
    assert f.stat(f.STAT_UPDATE_STRIPES) - patched0 == patched
    assert f.stat(f.STAT_UPDATE_COPY_COMMITS) - copies0 == (calls if copy_commit else 0)


@pytest.mark.parametrize("code", list(VARIANT))
def test_update_variant_names(code):
    assert fec(code).kernel_name(3) == VARIANT[code]
    assert fec(code).kernel_name(3).startswith("update_")


@pytest.mark.parametrize("code,S,stripes", CASES)
def test_update(code, S, stripes):
    check_updates(fec(code), layout(code, S, stripes), code in COPY_COMMIT)


def test_update_widest_jobs_cross_the_lds_threshold():
    L = layout("rs200_216", 4112, 2)
    f, d = fec("rs200_216"), Dev(L)
    assert f.kernel_name(3) == "update_MG16_B256"
    rng = np.random.default_rng(8)
    copies0 = f.stat(f.STAT_UPDATE_COPY_COMMITS)
    d.update(f, [(1, int(i)) for i in rng.permutation(200)[:195]] + [(0, 7)], seed=1)
    d.check("j = 195")
    assert f.stat(f.STAT_UPDATE_COPY_COMMITS) == copies0
    d.update(f, [(0, int(i)) for i in rng.permutation(200)[:196]] + [(1, 199)], seed=2)
    d.check("j = 196")
    assert f.stat(f.STAT_UPDATE_COPY_COMMITS) == copies0 + 1
    d.update(f, [(1, int(i)) for i in rng.permutation(200)], seed=3)
    d.check("j = k = 200")
    assert f.stat(f.STAT_UPDATE_COPY_COMMITS) == copies0 + 2
    assert np.array_equal(d.verify(f), np.full(2, CLEAN, dtype=np.uint32))


def check_slice(f, L):
    """Bytes [4096, 5096) of two shards: data / parity advanced by 4096,
    shard_len = 1000; pitch and strides stay."""
    d = Dev(L)
    o, l = 4096, 1000
    ups = [(1, 3), (L.stripes - 1, 0), (1, L.k - 1)]
    rng = np.random.default_rng(77)
    slot = r16(l) + 16
    src_h = rng.integers(0, 256, size=len(ups) * slot, dtype=np.uint8)
    src = torch.from_numpy(src_h.copy()).cuda()
    f.update_stripes(d.data.data_ptr() + o, L.dss, d.parity.data_ptr() + o, L.pss, L.pitch, l, L.stripes,
                     [(s, i, src.data_ptr() + q * slot) for q, (s, i) in enumerate(ups)])
    f.sync()
    assert np.array_equal(src.cpu().numpy(), src_h)
    # The 8 bytes behind the slice are coded and committed too (round_up(1000,
    # 16)): they lie inside the shard here, so the model takes them as well
    # and the whole stripe must still match the oracle.
    for q, (s, i) in enumerate(ups):
        d.payload[s, i, o:o + r16(l)] = src_h[q * slot:q * slot + r16(l)]
    touched = sorted({s for s, _ in ups})
    ref = L.encode(d.payload[touched])
    for s, i in ups:
        at = s * L.dss + i * L.pitch
        d.want_d[at:at + L.S] = d.payload[s, i]
    for t, s in enumerate(touched):
        for r in range(L.m):
            at = s * L.pss + r * L.pitch
            d.want_p[at:at + L.S] = ref[t, r]
    d.check("slice")  # no loose bytes: nothing outside [o, o + 1008) of the listed shards and their parity may change
    got_p = d.parity.cpu().numpy()
    for s in touched:
        for r in range(L.m):
            at = s * L.pss + r * L.pitch
            assert np.array_equal(got_p[at:at + o], L.parity[at:at + o]) and \
                np.array_equal(got_p[at + o + r16(l):at + L.pitch], L.parity[at + o + r16(l):at + L.pitch])
    assert np.array_equal(d.verify(f), np.full(L.stripes, CLEAN, dtype=np.uint32))


@pytest.mark.parametrize("code", ["rs10_14", "rs12_40"])
def test_update_slice(code):
    check_slice(fec(code), layout(code, SLICE_S, 3))


def test_update_refusals_leave_memory_alone():
    L = layout("rs10_14", 4112, 3)
    f, d = fec("rs10_14"), Dev(L)
    src = torch.zeros(4 * (r16(L.S) + 16), dtype=torch.uint8, device="cuda:0")
    sp = src.data_ptr()
    dp, dss, pp, pss, pitch, S, stripes = d.args()
    lib = rsmi.load()
    patched0 = f.stat(f.STAT_UPDATE_STRIPES)

    def call(entries, count=None, st=stripes):
        arr = (rsmi.ShardUpdate * max(len(entries), 1))(*[rsmi.ShardUpdate(*e) for e in entries])
        return lib.rs_update_stripes(f._h, dp, dss, pp, pss, pitch, S, st, arr, len(entries) if count is None else count,
                                     None)

    good = (1, 2, 0, sp)
    assert call([good, (0, L.k, 0, sp + 8192)]) == rsmi.RS_EBAD_SHARE_ID
    assert call([good, (stripes, 0, 0, sp + 8192)]) == rsmi.RS_EINVAL
    assert call([good, (0, 1, 0, sp + 8192), (1, 2, 0, sp + 8192)]) == rsmi.RS_EINVAL  # duplicate
    assert call([good, (0, 1, 0, sp + 8)]) == rsmi.RS_EINVAL                            # misaligned src
    assert call([good, (0, 1, 0, 0)]) == rsmi.RS_EINVAL                                 # NULL src
    assert call([good, (0, 1, 1, sp + 8192)]) == rsmi.RS_EINVAL                         # reserved
    # src inside the data region, inside the parity region, and straddling the data region's end
    assert call([good, (0, 1, 0, dp + 2 * pitch)]) == rsmi.RS_EINVAL
    assert call([good, (0, 1, 0, pp + pss)]) == rsmi.RS_EINVAL
    data_end = dp + (stripes - 1) * dss + (L.k - 1) * pitch + r16(S)
    assert call([good, (0, 1, 0, data_end - 16)]) == rsmi.RS_EINVAL
    assert lib.rs_update_stripes(f._h, dp, dss, pp, pss, pitch, S, stripes, None, 1, None) == rsmi.RS_EINVAL
    assert lib.rs_update_stripes(f._h, dp + 8, dss, pp, pss, pitch, S, stripes,
                                 (rsmi.ShardUpdate * 1)(rsmi.ShardUpdate(*good)), 1, None) == rsmi.RS_EINVAL
    # 2^31 blocks: 4,096 jobs x 2^19 column chunks of 2 GiB shards (refused before anything is read:
    # the strides are zero and src is a bare aligned address outside every region)
    big = (rsmi.ShardUpdate * 4096)(*[rsmi.ShardUpdate(s, 0, 0, 16) for s in range(4096)])
    assert lib.rs_update_stripes(f._h, dp, 0, pp, 0, 1 << 31, 1 << 31, 4096, big, 4096, None) == rsmi.RS_EINVAL
    # nothing to do: RS_OK whatever the entries hold
    assert call([(99, 99, 9, 1)], count=0) == rsmi.RS_OK
    assert call([good], st=0) == rsmi.RS_OK
    assert lib.rs_update_stripes(f._h, dp, dss, pp, pss, pitch, 0, stripes,
                                 (rsmi.ShardUpdate * 1)(rsmi.ShardUpdate(*good)), 1, None) == rsmi.RS_OK
    f.sync()
    d.check("refusals")  # byte-identical: nothing is loose
    assert f.stat(f.STAT_UPDATE_STRIPES) == patched0


def test_update_leaves_an_inconsistent_stripe_inconsistent_by_the_same_difference():
    """The stored parity is trusted: a wrong parity byte stays wrong by the
    same XOR, at the same place, and nowhere else."""
    L = layout("rs10_14", 5000, 3)
    f, d = fec("rs10_14"), Dev(L)
    at = 1 * L.pss + 2 * L.pitch + 1234
    d.parity[at] ^= 0x5A
    d.update(f, [(1, 4), (2, 0)], seed=3)
    d.want_p[at] ^= 0x5A
    d.check("trusted parity")
    want = np.full(3, CLEAN, dtype=np.uint32)
    want[1] = 1234
    assert np.array_equal(d.verify(f), want)


def test_update_without_parity_only_commits():
    """RS(4,4), m = 0: the listed shards take the new contents, nothing else
    changes, and the commit is the copy pass."""
    k, S, stripes = 4, 5000, 3
    pitch, dss = r16(S) + 32, 4 * (r16(S) + 32) + 48
    f = rsmi.FEC(k, k, device=0)
    rng = np.random.default_rng(44)
    host = rng.integers(0, 256, size=stripes * dss, dtype=np.uint8)
    src_h = rng.integers(0, 256, size=2 * pitch, dtype=np.uint8)
    data, src = torch.from_numpy(host.copy()).cuda(), torch.from_numpy(src_h.copy()).cuda()
    ups = [(2, 3, src.data_ptr()), (0, 1, src.data_ptr() + pitch)]
    f.update_stripes(data.data_ptr(), dss, 0, 0, pitch, S, stripes, ups)
    f.sync()
    want = host.copy()
    for q, (s, i, _) in enumerate(ups):
        o = s * dss + i * pitch
        want[o:o + r16(S)] = src_h[q * pitch:q * pitch + r16(S)]  # round_up(shard_len, 16) bytes are committed
    assert np.array_equal(data.cpu().numpy(), want)
    assert np.array_equal(src.cpu().numpy(), src_h)
    assert f.stat(f.STAT_UPDATE_STRIPES) == 2 and f.stat(f.STAT_UPDATE_COPY_COMMITS) == 1
    f.close()


def test_update_device_set_routes_the_call():
    L = layout("rs10_14", 5000, 3)
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert fs.kernel_name(3) == "update_MG4_B256"
    d = Dev(L)
    d.update(fs, [(2, 9), (0, 0), (2, 1)], seed=21)
    d.check("device set")
    assert fs.stat(fs.STAT_UPDATE_STRIPES) == 2 and fs.stat(fs.STAT_UPDATE_COPY_COMMITS) == 0
    assert np.array_equal(d.verify(fs), np.full(3, CLEAN, dtype=np.uint32))
    fs.close()


def test_update_four_threads_one_context():
    """Four threads share one context; each patches its own layout ten times
    with alternating contents (two src sets: the second is the inverse of the
    first, so the expected bytes alternate between two oracle results)."""
    L = layout("rs10_14", 4112, 37)
    f = fec("rs10_14")
    devs = [Dev(L) for _ in range(4)]
    errors = []

    def work(t):
        try:
            d = devs[t]
            ups = [(s, (s + t) % L.k) for s in range(0, 37, 2)] + [(36, (36 + t + 1) % L.k)]
            for r in range(10):
                if r % 2 == 0:
                    d.update(f, ups, seed=1000 + t)
                else:  # back to the pristine shards
                    slot = r16(L.S) + 16
                    old = np.zeros(len(ups) * slot, dtype=np.uint8)
                    for q, (s, i) in enumerate(ups):
                        old[q * slot:q * slot + L.S] = L.payload[s, i]
                    src = torch.from_numpy(old).cuda()
                    f.update_stripes(*d.args(), [(s, i, src.data_ptr() + q * slot) for q, (s, i) in enumerate(ups)])
                    f.sync()
                    d.payload = L.payload.copy()
                    d.want_d, d.want_p = L.data.copy(), L.parity.copy()
                d.check(f"thread {t} round {r}")
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_update_multi_iteration_child():
    """RSMI_ITERS is read once per process: a child with RSMI_ITERS=2 runs the
    update sets and the slice update of a several-chunk shape (two column
    chunks per block, the second one's loads issued from inside the loop)."""
    env = dict(os.environ, RSMI_ITERS="2")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "iters child ok" in run.stdout


if __name__ == "__main__":
    assert os.environ.get("RSMI_ITERS") == "2"
    check_updates(fec("rs10_14"), layout("rs10_14", SLICE_S, 3), False)
    check_updates(fec("rs12_40"), layout("rs12_40", SLICE_S, 3), True)
    check_updates(fec("rs64_80"), layout("rs64_80", SLICE_S, 3), False)
    check_slice(fec("rs10_14"), layout("rs10_14", SLICE_S, 3))
    print("iters child ok")

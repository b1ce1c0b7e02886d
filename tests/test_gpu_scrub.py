"""GPU: the scrub of device-resident stripes -- rs_verify_stripes (the verify
twin of the split-table encode kernel) and rs_correct_stripes (verify, locate
by Berlekamp-Welch on one gathered column, batched reconstruct, verify again).

Stripes are laid out with a shard pitch above round_up(shard_len, 16) and
stripe strides with gaps; padding and gaps hold random bytes.  The expected
parity comes from the oracle (oracle.encode_batch), never from the engine; it
is computed once per geometry and every test works on clones of it.
"""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

if __name__ == "__main__":  # the RSMI_ITERS child of test_verify_multi_iteration_child
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
CODES = {"rs10_14": (10, 14), "rs4_6": (4, 6), "rs8_14": (8, 14), "rs12_40": (12, 40), "rs64_80": (64, 80)}
VARIANT = {"rs10_14": "verify_K10_MG4_B256", "rs4_6": "verify_K4_MG4_B256", "rs8_14": "verify_K8_MG6_B256",
           "rs12_40": "verify_K0_MG8_B256", "rs64_80": "verify_K64_MG16_B256"}
# one column | exactly one 4 KiB block chunk | a chunk plus one column | not a
# multiple of 16 | several chunks
SHAPES = [16, 4096, 4112, 5000, 3 * 4096 + 40]
VERIFY_CASES = [(c, S, st) for c in CODES for S in (SHAPES if c != "rs64_80" else [4112, 5000]) for st in (1, 3, 37)]


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
        rng = np.random.default_rng(seed)
        payload = rng.integers(0, 256, size=(stripes, k, S), dtype=np.uint8)
        E = oracle.fec_matrix(k, n)
        ref = oracle.encode_batch(E, k, n, np.ascontiguousarray(payload).reshape(-1), S, stripes).reshape(stripes, self.m, S)
        self.data = rng.integers(0, 256, size=stripes * self.dss, dtype=np.uint8)
        self.parity = rng.integers(0, 256, size=stripes * self.pss, dtype=np.uint8)
        for s in range(stripes):
            for i in range(k):
                o = s * self.dss + i * self.pitch
                self.data[o:o + S] = payload[s, i]
            for i in range(self.m):
                o = s * self.pss + i * self.pitch
                self.parity[o:o + S] = ref[s, i]
        self.data.setflags(write=False)
        self.parity.setflags(write=False)

    def offset(self, s, shard, byte=0):
        """(is_parity, offset into the data or parity buffer)"""
        if shard < self.k:
            return False, s * self.dss + shard * self.pitch + byte
        return True, s * self.pss + (shard - self.k) * self.pitch + byte

    def device(self):
        return torch.from_numpy(self.data.copy()).cuda(), torch.from_numpy(self.parity.copy()).cuda()


_LAYOUTS = {}


def layout(code, S, stripes):
    key = (code, S, stripes)
    if key not in _LAYOUTS:
        k, n = CODES[code] if isinstance(code, str) else code
        _LAYOUTS[key] = Layout(k, n, S, stripes, seed=k * 1000003 + n * 10007 + S * 31 + stripes)
    return _LAYOUTS[key]


_FECS = {}


def fec(code):
    if code not in _FECS:
        k, n = CODES[code] if isinstance(code, str) else code
        _FECS[code] = rsmi.FEC(k, n, device=0)
    return _FECS[code]


class Dev:
    """Device clones of a layout plus helpers to corrupt and to call the engine."""

    def __init__(self, L):
        self.L = L
        self.data, self.parity = L.device()
        self.d0, self.p0 = self.data.clone(), self.parity.clone()

    def buf(self, shard):
        return self.parity if shard >= self.L.k else self.data

    def flip(self, s, shard, byte, mask=0x40):
        _, o = self.L.offset(s, shard, byte)
        self.buf(shard)[o] ^= mask

    def garbage(self, s, shard, seed):
        """Whole-shard garbage: every byte of [0, shard_len) changes."""
        _, o = self.L.offset(s, shard)
        g = torch.from_numpy(np.random.default_rng(seed).integers(1, 256, size=self.L.S, dtype=np.uint8)).cuda()
        self.buf(shard)[o:o + self.L.S] ^= g

    def restore(self):
        self.data.copy_(self.d0)
        self.parity.copy_(self.p0)

    def args(self):
        L = self.L
        return (self.data.data_ptr(), L.dss, self.parity.data_ptr(), L.pss, L.pitch, L.S, L.stripes)

    def verify(self, f):
        fb = torch.zeros(self.L.stripes, dtype=torch.int32, device="cuda:0")  # zeros: the engine must initialise it
        f.verify_stripes(*self.args(), fb.data_ptr())
        f.sync()
        return fb.cpu().numpy().view(np.uint32)

    def correct(self, f):
        st, rw = f.correct_stripes(*self.args())
        return st, np.frombuffer(rw, dtype=np.uint8).reshape(self.L.stripes, self.L.n)

    def unchanged(self):
        return torch.equal(self.data, self.d0) and torch.equal(self.parity, self.p0)

    def assert_restored(self, rewritten):
        """Shard bytes [0, shard_len) equal the pristine ones everywhere;
        everything but the 16-byte padding of a rewritten shard (which the
        reconstruct codes, as rs_encode_stripes does) is byte-identical."""
        L = self.L
        hd, hp = self.data.cpu().numpy(), self.parity.cpu().numpy()
        ed, ep = L.data.copy(), L.parity.copy()
        for s in range(L.stripes):
            for i in np.flatnonzero(rewritten[s]):
                par, o = L.offset(s, int(i))
                (ep if par else ed)[o + L.S:o + r16(L.S)] = (hp if par else hd)[o + L.S:o + r16(L.S)]
        assert np.array_equal(hd, ed), np.flatnonzero(hd != ed)[:8]
        assert np.array_equal(hp, ep), np.flatnonzero(hp != ep)[:8]


def expect(stripes, **bad):
    e = np.full(stripes, CLEAN, dtype=np.uint32)
    for s, off in bad.items():
        e[int(s[1:])] = off
    return e


@pytest.mark.parametrize("code", list(CODES))
def test_verify_variant_names(code):
    assert fec(code).kernel_name(2) == VARIANT[code]


def check_verify(f, L):
    """Every verify case of one geometry."""
    k, n, S, stripes = L.k, L.n, L.S, L.stripes
    d = Dev(L)
    assert np.array_equal(d.verify(f), expect(stripes)), "clean"
    assert d.unchanged(), "verify wrote to the stripes"
    flips = [(0, 0), (k, S - 1), (k - 1, S // 2), (n - 1, 0), (n - 1, S - 1), (1, S - 1)]
    flips += [(sh, off) for sh in (0, k + 1) for off in (4095, 4096) if off < S]
    for j, (shard, off) in enumerate(flips):
        s = j % stripes
        d.flip(s, shard, off, mask=1 << (j % 8))
        got = d.verify(f)
        assert np.array_equal(got, expect(stripes, **{f"s{s}": off})), (shard, off, got)
        d.restore()
    # bytes the code does not cover: 16-byte padding, pitch gap, stripe gap
    s = stripes - 1
    for shard in (0, n - 1):
        if S % 16:
            d.flip(s, shard, S)
            d.flip(s, shard, r16(S) - 1)
        d.flip(s, shard, r16(S))
        d.flip(s, shard, L.pitch - 1)
    d.data[s * L.dss + k * L.pitch] ^= 0xFF
    d.parity[s * L.pss + L.m * L.pitch] ^= 0xFF
    assert np.array_equal(d.verify(f), expect(stripes)), "padding and gaps are not compared"
    d.restore()
    # two corruptions in one stripe: the smaller offset wins, whichever shard
    if S > 16:
        lo, hi = S // 3, S - 2
        for a, b in ((0, n - 1), (n - 1, 0), (k, k - 1)):
            d.flip(s, a, lo)
            d.flip(s, b, hi)
            assert np.array_equal(d.verify(f), expect(stripes, **{f"s{s}": lo})), (a, b)
            d.restore()


@pytest.mark.parametrize("code,S,stripes", VERIFY_CASES)
def test_verify(code, S, stripes):
    check_verify(fec(code), layout(code, S, stripes))


def test_verify_row_groups_report_the_minimum():
    """RS(12,40): 28 parity rows in four row groups of 8, whose blocks contend
    on one word.  Parity rows 1 and 18 (shards 13 and 30) and the last row
    sit in different groups."""
    L = layout("rs12_40", 5000, 3)
    f, d = fec("rs12_40"), Dev(L)
    for (ra, oa), (rb, ob) in (((1, 4500), (18, 77)), ((1, 77), (18, 4500)), ((27, 4999), (9, 4998))):
        d.flip(1, L.k + ra, oa)
        d.flip(1, L.k + rb, ob)
        assert np.array_equal(d.verify(f), expect(3, s1=min(oa, ob)))
        d.restore()


def test_verify_device_set_matches_single_device():
    L = layout("rs10_14", 5000, 3)
    d = Dev(L)
    d.flip(2, 4, 1234)
    d.flip(0, 12, 4999)
    one = d.verify(fec("rs10_14"))
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert np.array_equal(d.verify(fs), one)
    assert np.array_equal(one, expect(3, s0=4999, s2=1234))
    fs.close()


def test_verify_rejects_bad_arguments():
    L = layout("rs10_14", 4112, 3)
    f, d = fec("rs10_14"), Dev(L)
    fb = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    dp, dss, pp, pss, pitch, S, stripes = d.args()
    lib = rsmi.load()
    call = lambda *a: lib.rs_verify_stripes(f._h, *a, None)  # noqa: E731
    assert call(dp, dss, pp, pss, pitch, S, stripes, fb.data_ptr()) == rsmi.RS_OK
    assert call(dp, dss, pp, pss, pitch + 8, S, stripes, fb.data_ptr()) == rsmi.RS_EINVAL
    assert call(dp, dss, pp, pss, r16(S) - 16, S, stripes, fb.data_ptr()) == rsmi.RS_EINVAL
    assert call(dp, dss, pp, pss, pitch, S, stripes, fb.data_ptr() + 2) == rsmi.RS_EINVAL
    assert call(dp, dss, pp, pss, pitch, S, stripes, None) == rsmi.RS_EINVAL
    assert call(dp + 8, dss, pp, pss, pitch, S, stripes, fb.data_ptr()) == rsmi.RS_EINVAL
    assert call(dp, dss, pp, pss, pitch, S, 0, None) == rsmi.RS_OK
    st = (ctypes.c_int * 3)()
    assert lib.rs_correct_stripes(f._h, dp, dss, pp, pss, pitch + 8, S, stripes, st, None, None) == rsmi.RS_EINVAL
    f.sync()
    assert d.unchanged()


def test_verify_multi_iteration_child():
    """RSMI_ITERS is read once per process: a child with RSMI_ITERS=2 runs the
    verify cases of a several-chunk shape (two column chunks per block, the
    second one's loads issued from inside the loop) and one repair."""
    env = dict(os.environ, RSMI_ITERS="2")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "iters child ok" in run.stdout


# ---------------------------------------------------------------- correct --
def check_repair(f, L, corrupt, want_rewritten):
    """corrupt(d) damages clones of L; the scrub must restore them and report
    exactly want_rewritten = {stripe: set of shards}."""
    d = Dev(L)
    corrupt(d)
    assert not d.unchanged()
    st, rw = d.correct(f)
    assert st == [rsmi.RS_OK] * L.stripes
    want = np.zeros((L.stripes, L.n), dtype=bool)
    for s, shards in want_rewritten.items():
        want[s, sorted(shards)] = True
    assert np.array_equal(rw != 0, want), [np.flatnonzero(r).tolist() for r in rw]
    d.assert_restored(rw)
    assert np.array_equal(d.verify(f), expect(L.stripes))


@pytest.mark.parametrize("code", ["rs10_14", "rs4_6", "rs8_14", "rs12_40"])
def test_correct_one_shard(code):
    L = layout(code, 5000, 3)
    f = fec(code)
    check_repair(f, L, lambda d: d.garbage(1, 2, seed=5), {1: {2}})            # a data shard, whole-shard garbage
    check_repair(f, L, lambda d: d.garbage(2, L.n - 1, seed=6), {2: {L.n - 1}})  # a parity shard

    def three_bytes(d):
        for off in (3, 2500, 4999):
            d.flip(0, L.k - 1, off, mask=0x81)
    check_repair(f, L, three_bytes, {0: {L.k - 1}})


def test_correct_two_shards_same_column():
    L = layout("rs10_14", 5000, 3)

    def corrupt(d):
        d.flip(1, 2, 777)
        d.flip(1, 11, 777, mask=0x13)
    check_repair(fec("rs10_14"), L, corrupt, {1: {2, 11}})


def test_correct_second_round_erases_both():
    """Shard 3 is wrong only at offset 5 and shard 7 only at offset 900.
    Shard 7 is one of Rebuild's survivors for shard 3, so the first repair of
    shard 3 comes out wrong at offset 900; the second round locates shard 7
    there and regenerates both."""
    L = layout("rs10_14", 5000, 3)

    def corrupt(d):
        d.flip(1, 3, 5)
        d.flip(1, 7, 900)
    check_repair(fec("rs10_14"), L, corrupt, {1: {3, 7}})


def test_correct_rs64_80_eight_shards():
    L = layout("rs64_80", 4112, 3)
    shards = [0, 9, 31, 63, 64, 70, 75, 79]  # floor(16 / 2), over data and parity

    def corrupt(d):
        for j, sh in enumerate(shards):
            if j % 2:
                d.garbage(1, sh, seed=40 + j)
            else:
                d.flip(1, sh, 1 + 500 * j, mask=0xFF)
    check_repair(fec("rs64_80"), L, corrupt, {1: set(shards)})


def test_correct_batch_of_37():
    L = layout("rs10_14", 4112, 37)

    def corrupt(d):
        d.garbage(0, 13, seed=1)
        d.flip(5, 0, 0)
        d.flip(5, 12, 4111)
        d.garbage(36, 9, seed=2)
        d.flip(36, 4, 4096, mask=0x02)
    check_repair(fec("rs10_14"), L, corrupt, {0: {13}, 5: {0, 12}, 36: {4, 9}})


def test_correct_radius_zero_reports_too_many_errors():
    """RS(4,5), m = 1: an error can be seen but not located."""
    L = layout((4, 5), 4112, 3)
    f, d = fec((4, 5)), Dev(L)
    assert f.kernel_name(2) == "verify_K4_MG4_B256"
    d.flip(1, 2, 100)
    assert np.array_equal(d.verify(f), expect(3, s1=100))
    before_d, before_p = d.data.clone(), d.parity.clone()
    st = (ctypes.c_int * 3)()
    rw = ctypes.create_string_buffer(3 * 5)
    rc = rsmi.load().rs_correct_stripes(f._h, *d.args(), st, ctypes.cast(rw, ctypes.c_void_p), None)
    assert rc == rsmi.RS_ETOO_MANY_ERRORS
    assert list(st) == [rsmi.RS_OK, rsmi.RS_ETOO_MANY_ERRORS, rsmi.RS_OK]
    assert rw.raw == bytes(15)
    assert torch.equal(d.data, before_d) and torch.equal(d.parity, before_p)
    st2, rw2 = d.correct(f)  # the binding reports it through the status list
    assert st2 == list(st) and not rw2.any()


# Three corrupt shards at one column of RS(10,14) are past the radius of 2.
# The seed below was chosen on the CPU so that the oracle's Berlekamp-Welch
# (oracle.decode_correct on that column with all 14 shares) finds no codeword
# within the radius: its verdict is ORACLE_VERDICT, the oracle's TooManyErrors
# code (seed 1: shards 5, 6 and 10 at offset 1246).
THREE_ERRORS_SEED = 1
ORACLE_VERDICT = -7  # ORC_ETOO_MANY (oracle/rs_oracle.h)
ORACLE_TO_ENGINE = {0: rsmi.RS_OK, -7: rsmi.RS_ETOO_MANY_ERRORS}


def three_errors(L, seed):
    rng = np.random.default_rng(seed)
    shards = sorted(int(x) for x in rng.choice(L.n, size=3, replace=False))
    masks = [int(x) for x in rng.integers(1, 256, size=3)]
    return shards, masks, int(rng.integers(0, L.S))


def test_correct_three_errors_matches_the_oracle():
    L = layout("rs10_14", 5000, 3)
    f, d = fec("rs10_14"), Dev(L)
    shards, masks, off = three_errors(L, THREE_ERRORS_SEED)
    for sh, mk in zip(shards, masks):
        d.flip(1, sh, off, mask=mk)
    col = []
    for i in range(L.n):
        par, o = L.offset(1, i, off)
        col.append(int((d.parity if par else d.data)[o]))
    rc, _ = oracle.decode_correct(oracle.fec_matrix(10, 14), 10, 14, [(i, bytes([col[i]])) for i in range(14)])
    assert (shards, off) == ([5, 6, 10], 1246)
    assert rc == ORACLE_VERDICT
    before_d, before_p = d.data.clone(), d.parity.clone()
    st, rw = d.correct(f)
    assert st == [rsmi.RS_OK, ORACLE_TO_ENGINE[rc], rsmi.RS_OK]
    assert not rw.any()
    assert torch.equal(d.data, before_d) and torch.equal(d.parity, before_p)  # nothing located, nothing rewritten


def test_correct_clean_batch_runs_no_reconstruct():
    L = layout("rs10_14", 4112, 37)
    f, d = fec("rs10_14"), Dev(L)
    patterns = f.stat(f.STAT_PATTERNS)
    st, rw = d.correct(f)
    assert st == [rsmi.RS_OK] * 37 and not rw.any()
    assert f.stat(f.STAT_PATTERNS) == patterns
    assert d.unchanged()


def test_correct_two_threads_one_context():
    L = layout("rs10_14", 5000, 3)
    f = fec("rs10_14")
    devs = [Dev(L), Dev(L)]
    errors = []

    def work(t):
        try:
            d = devs[t]
            for r in range(5):
                shard = (3 * t + 2 * r) % L.n
                d.garbage(r % 3, shard, seed=100 * t + r)
                st, rw = d.correct(f)
                assert st == [rsmi.RS_OK] * 3
                assert np.flatnonzero(rw.reshape(-1)).tolist() == [(r % 3) * L.n + shard]
                d.assert_restored(rw)
                d.restore()
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def test_correct_device_set():
    L = layout("rs10_14", 5000, 3)
    fs = rsmi.FEC(10, 14, devices=[0, 0])

    def corrupt(d):
        d.garbage(0, 6, seed=9)
        d.flip(2, 10, 4999)
    check_repair(fs, L, corrupt, {0: {6}, 2: {10}})
    fs.close()


if __name__ == "__main__":
    assert os.environ.get("RSMI_ITERS") == "2"
    _L = layout("rs10_14", 3 * 4096 + 40, 3)
    check_verify(fec("rs10_14"), _L)
    check_verify(fec("rs12_40"), layout("rs12_40", 3 * 4096 + 40, 3))
    check_repair(fec("rs10_14"), _L, lambda d: (d.flip(1, 3, 5), d.flip(1, 7, 9000)), {1: {3, 7}})
    print("iters child ok")

"""GPU: rs_reconstruct_checked and rs_reconstruct_checked_ptrs -- the repair
that verifies its survivors in the same pass.

Every case works on a whole image (strided_image.Layout for the strided
layout, strided_image.Pool for the pointer placement): nothing is dense, the
slots of the erased shards are pre-filled with random bytes over their whole
pitch (in pointer mode they are the shards' own rows, distinct valid rows the
table names), and after every call the ENTIRE buffer -- and in pointer mode
the table -- is compared with the expected image, byte for byte, the pad
between shard_len and the next multiple of 16 included.

Expected bytes and verdicts never come from the engine.  The codeword of a
stripe is the oracle's: Decode of the k survivors Rebuild chooses (written the
long way here) as the image holds them, damage included, then Encode.  The
erased slots must hold that codeword's shards over round_up(shard_len, 16)
bytes, and first_bad is the lowest offset below shard_len at which a present
shard outside the survivors differs from it.  The byte columns of a stripe are
codewords of their own, so the oracle runs over the 16-byte blocks that hold a
damaged survivor byte or the random pad; everywhere else the codeword is the
pristine one (payload seeded, parity from the oracle).
"""
import ctypes
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from oracle import oracle  # noqa: E402
from strided_image import Layout, Pool, r16  # noqa: E402

CLEAN = rsmi.RS_VERIFY_CLEAN
SENTINEL = 0x7A7A7A7A
# K4 | K10, one full group | K8, m = 6: a full and a partial group | runtime K,
# m = 16: four groups | LDS pointers, both routes | m = 1: intact or saturated |
# r up to 256
CODES = {"rs4_6": (4, 6), "rs10_14": (10, 14), "rs8_14": (8, 14), "rs3_19": (3, 19), "rs64_80": (64, 80),
         "rs4_5": (4, 5), "rs240_256": (240, 256)}
REPAIR_NAME = {"rs4_6": "repair_K4_MG4_B256", "rs10_14": "repair_K10_MG4_B256", "rs8_14": "repair_K8_MG4_B256",
               "rs3_19": "repair_K0_MG4_B256", "rs64_80": "repair_K64_MG4_B256", "rs4_5": "repair_K4_MG4_B256",
               "rs240_256": "repair_K0_MG4_B256"}
# one column | exactly one 4 KiB block chunk | a chunk plus one column | not a
# multiple of 16 | several chunks
SHAPES = [16, 4096, 4112, 5000, 3 * 4096 + 40]
STRIPES = [1, 3, 37]
# route: None = the context's default (the repair kernel); "fused" / "split"
# force the repair kernel / the check and reconstruct launches (RS(64,16): both)
CASES = ([(c, None, S, st) for c in ("rs4_6", "rs10_14", "rs8_14", "rs3_19", "rs4_5") for S in SHAPES for st in STRIPES] +
         [("rs64_80", r, S, st) for r in ("fused", "split") for S in SHAPES for st in STRIPES] +
         [("rs240_256", None, S, st) for S in (16, 4112) for st in STRIPES])
PLACEMENTS = ("strided", "ptrs")

_STORES = {}
_FECS = {}
_MATRIX = {}


def fec(code, route=None):
    """One context per (code, route).  RSMI_REPAIR_FUSED is read when a
    context is created."""
    key = (code, route)
    if key not in _FECS:
        old = os.environ.pop("RSMI_REPAIR_FUSED", None)
        try:
            if route is not None:
                os.environ["RSMI_REPAIR_FUSED"] = "1" if route == "fused" else "0"
            _FECS[key] = rsmi.FEC(*CODES[code], device=0)
        finally:
            os.environ.pop("RSMI_REPAIR_FUSED", None)
            if old is not None:
                os.environ["RSMI_REPAIR_FUSED"] = old
    return _FECS[key]


def matrix(k, n):
    if (k, n) not in _MATRIX:
        _MATRIX[(k, n)] = oracle.fec_matrix(k, n)
    return _MATRIX[(k, n)]


def rebuild_choice(k, n, er_row):
    """Rebuild's survivors: every present data share, then the highest present parity."""
    c = [i for i in range(k) if not er_row[i]]
    for i in range(n - 1, k - 1, -1):
        if len(c) < k and not er_row[i]:
            c.append(i)
    return sorted(c)


def oracle_codeword(k, n, shares):
    """The n shards of the codeword through k shares [(id, bytes)]: the
    oracle's Decode, then its Encode."""
    E = matrix(k, n)
    rc, data = oracle.decode(E, k, n, shares)
    assert rc == 0, rc
    L = len(shares[0][1])
    par = oracle.encode(E, k, n, data)
    rows = [data[i * L:(i + 1) * L] for i in range(k)] + [par[i * L:(i + 1) * L] for i in range(n - k)]
    return [np.frombuffer(r, dtype=np.uint8) for r in rows]


class Strided:
    """A Layout as a store of shards: buffers, slots, the call."""
    placement = "strided"

    def __init__(self, code, S, stripes):
        k, n = CODES[code]
        self.G = Layout(k, n, S, stripes, seed=k * 1000003 + n * 10007 + S * 31 + stripes,
                        mode="joined" if S % 32 == 16 else "split")
        self.k, self.n, self.m, self.S, self.stripes = k, n, n - k, S, stripes
        self.slot_bytes = self.G.pitch
        self.pristine = self.G.pristine

    def at(self, s, i):
        return self.G.shard_at(s, i)

    def shard(self, s, i):
        return self.G.shard(s, i)


class Pointer:
    """A Pool as a store of shards; every table entry names its shard's row,
    erased or not."""
    placement = "ptrs"

    def __init__(self, code, S, stripes):
        k, n = CODES[code]
        self.G = Pool(k, n, S, stripes, seed=k * 1000003 + n * 10007 + S * 31 + stripes + 1)
        self.k, self.n, self.m, self.S, self.stripes = k, n, n - k, S, stripes
        self.slot_bytes = self.G.row_bytes
        self.pristine = self.G.pristine

    def at(self, s, i):
        return 0, self.G.row_at(self.G.rows[s, i])

    def shard(self, s, i):
        return self.G.payload[s, i] if i < self.k else self.G.ref[s, i - self.k]


def store(placement, code, S, stripes):
    key = (placement, code, S, stripes)
    if key not in _STORES:
        while len(_STORES) >= 6:
            del _STORES[next(iter(_STORES))]
        _STORES[key] = (Strided if placement == "strided" else Pointer)(code, S, stripes)
    return _STORES[key]


class Run:
    """The host model of one call on a store: `cur` is what the buffers hold
    before the call, `want` what they must hold afterwards, `fb` the verdicts."""

    def __init__(self, T, er, seed=0):
        self.T = T
        self.er = np.asarray(er, dtype=np.uint8).reshape(T.stripes, T.n)
        self.cur = [b.copy() for b in T.pristine]
        self.flips = {}  # (stripe, shard) -> offsets
        rng = np.random.default_rng(4000 + seed)
        for s, i in zip(*np.nonzero(self.er)):
            b, o = T.at(s, i)
            self.cur[b][o:o + T.slot_bytes] = rng.integers(0, 256, size=T.slot_bytes, dtype=np.uint8)
        self.dev = self.table = self.host_table = None
        self.want = self.fb = None

    def present(self, s):
        return [i for i in range(self.T.n) if not self.er[s, i]]

    def survivors(self, s):
        return rebuild_choice(self.T.k, self.T.n, self.er[s])

    def compared(self, s):
        c = set(self.survivors(s))
        return [i for i in self.present(s) if i not in c]

    def flip(self, s, i, off, mask):
        """XORs mask into byte off of the slot of present shard i of stripe s."""
        assert mask and not self.er[s, i] and 0 <= off < self.T.slot_bytes
        b, o = self.T.at(s, i)
        self.cur[b][o + off] ^= mask
        self.flips.setdefault((int(s), int(i)), []).append(off)

    def slot(self, bufs, s, i, lo, hi):
        b, o = self.T.at(s, i)
        return bufs[b][o + lo:o + hi]

    def expect(self):
        """want and fb from the oracle and the image before the call."""
        T = self.T
        S, R = T.S, r16(T.S)
        self.want = [b.copy() for b in self.cur]
        self.fb = np.full(T.stripes, CLEAN, dtype=np.uint32)
        for s in range(T.stripes):
            C, U = self.survivors(s), self.compared(s)
            X = [i for i in range(T.n) if self.er[s, i]]
            # The byte columns of a stripe are codewords of their own.  The
            # stripe's codeword through its survivors is the pristine one but
            # in the 16-byte blocks where a survivor is damaged and, for what
            # is written, in the pad behind shard_len, which holds random bytes:
            # the oracle runs over those blocks only.
            blocks = {off // 16 for i in C for off in self.flips.get((s, i), []) if off < R}
            if X and R > S:
                blocks.add(S // 16)
            words = {b: oracle_codeword(T.k, T.n, [(i, self.slot(self.cur, s, i, 16 * b, 16 * b + 16).tobytes())
                                                   for i in C]) for b in sorted(blocks)}
            for i in X:
                self.slot(self.want, s, i, 0, S)[:] = T.shard(s, i)
                for b, word in words.items():
                    self.slot(self.want, s, i, 16 * b, 16 * b + 16)[:] = word[i]
            for i in U:
                if not words and (s, i) not in self.flips:
                    continue  # stored as coded, and the codeword is the pristine one
                w = np.zeros(R, dtype=np.uint8)
                w[:S] = T.shard(s, i)
                for b, word in words.items():
                    w[16 * b:16 * b + 16] = word[i]
                bad = np.flatnonzero(self.slot(self.cur, s, i, 0, S) != w[:S])
                if bad.size:
                    self.fb[s] = min(int(self.fb[s]), int(bad[0]))
        return self

    def upload(self, within=None):
        """within: a device buffer and a 16-byte-aligned offset in it at which
        the (single) buffer of a pointer store goes."""
        if within is None:
            self.dev = [torch.from_numpy(b).cuda() for b in self.cur]
        else:
            assert len(self.cur) == 1
            self.dev = [within[0][within[1]:within[1] + len(self.cur[0])]]
            self.dev[0].copy_(torch.from_numpy(self.cur[0]))
        if self.T.placement == "ptrs":
            self.host_table = self.T.G.table(self.dev[0].data_ptr()).reshape(-1)
            assert (self.host_table % 16 == 0).all()
            self.table = torch.from_numpy(self.host_table.copy()).cuda()
        self.first_bad = torch.full((self.T.stripes,), SENTINEL, dtype=torch.int32, device="cuda:0")
        return self

    def args(self):
        if self.T.placement == "ptrs":
            return (self.table.data_ptr(), self.T.S, self.T.stripes)
        return self.T.G.args([d.data_ptr() for d in self.dev])

    def call(self, f, upload=True):
        """The checked repair over the image as it is now; returns first_bad."""
        if upload:
            self.upload()
        if self.T.placement == "ptrs":
            f.reconstruct_checked_ptrs(*self.args(), self.er.tobytes(), self.first_bad.data_ptr())
        else:
            f.reconstruct_checked(*self.args(), self.er.tobytes(), self.first_bad.data_ptr())
        f.sync()
        return self.verdicts()

    def two_calls(self, f):
        """rs_verify_degraded / rs_verify_ptrs, then rs_reconstruct_stripes / rs_reconstruct_ptrs."""
        self.upload()
        er = self.er.tobytes()
        if self.T.placement == "ptrs":
            f.verify_ptrs(*self.args(), self.first_bad.data_ptr(), erased=er)
            f.reconstruct_ptrs(*self.args(), er)
        else:
            f.verify_degraded(*self.args(), er, self.first_bad.data_ptr())
            f.reconstruct_stripes(*self.args(), er)
        f.sync()
        return self.verdicts()

    def verdicts(self):
        return self.first_bad.cpu().numpy().view(np.uint32)

    def image(self):
        return [d.cpu().numpy() for d in self.dev]

    def check(self, what="", want=None):
        want = self.want if want is None else want
        for name, g, w in zip(self.T.G.names if self.T.placement == "strided" else ["pool"], self.image(), want):
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, f"{what} {name}: {bad.size} bytes differ, first offsets {bad[:8].tolist()}"
        if self.table is not None:
            assert np.array_equal(self.table.cpu().numpy(), self.host_table), f"{what}: the table changed"

    def run(self, f, what=""):
        """expect, call, compare everything."""
        self.expect()
        got = self.call(f)
        assert np.array_equal(got, self.fb), (what, got.tolist(), self.fb.tolist())
        self.check(what)
        return got


def mandatory(k, n):
    """The erasure sets every geometry is run with: nothing | all parity (e =
    m) | erasures in the data only, as many as the code allows (e = m where k
    >= m) | one data shard | a data shard and a middle parity shard: the groups
    of X' then mix stored and compared rows | the highest parity shard."""
    m = n - k
    sets = [[], list(range(k, n)), list(range(min(m, k))), [k // 2]]
    if m >= 2:
        sets += [[0, k + m // 2], [n - 1]]
    return sets


def erasure_rounds(k, n, stripes, seed):
    """Flag arrays [stripes][n], as many as it takes to run every mandatory set
    at this stripe count; the other stripes get 0 .. m random erasures."""
    m = n - k
    rng = np.random.default_rng(seed)
    sets = mandatory(k, n)
    rounds = []
    for r0 in range(0, len(sets), stripes):
        er = np.zeros((stripes, n), dtype=np.uint8)
        for s in range(stripes):
            if r0 + s < len(sets):
                ids = sets[r0 + s]
            else:
                ids = rng.choice(n, size=int(rng.integers(0, m + 1)), replace=False)
            er[s, ids] = 1
        if stripes >= len(sets):
            er = er[rng.permutation(stripes)]
        rounds.append(er)
    return rounds


def count_stats(f):
    return f.stat(f.STAT_REPAIR_CHECKED), f.stat(f.STAT_CHECK_STRIPES)


def assert_stats(f, before, er, m, is_fused, what=""):
    e = er.sum(axis=1)
    repaired, checked = (a - b for a, b in zip(count_stats(f), before))
    if is_fused:  # every stripe with an erasure is the repair kernel's; intact ones are not counted
        assert (repaired, checked) == (int((e > 0).sum()), 0), (what, repaired, checked)
    else:  # the check kernel takes the degraded stripes that have something to compare
        assert (repaired, checked) == (0, int(((e > 0) & (e < m)).sum())), (what, repaired, checked)


# ------------------------------------------------------------ 1. clean ----
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("code,route,S,stripes", CASES)
def test_clean_stripes(code, route, S, stripes, placement):
    """Slots filled as the oracle says, every first_bad clean, nothing else changed."""
    T, f = store(placement, code, S, stripes), fec(code, route)
    for r, er in enumerate(erasure_rounds(T.k, T.n, stripes, seed=S + stripes)):
        before = count_stats(f)
        run = Run(T, er, seed=r)
        got = run.run(f, f"{code} S={S} x{stripes} round {r}")
        assert (got == CLEAN).all()
        assert_stats(f, before, er, T.m, route != "split", f"round {r}")


# ----------------------------------------------------------- 2. damage ----
DAMAGE = [("rs10_14", None), ("rs8_14", None), ("rs3_19", None), ("rs4_6", None), ("rs64_80", "fused"),
          ("rs64_80", "split")]


def special_offsets(S):
    """0, 15, 16, both sides of the first chunk edge, the last byte."""
    return [o for o in dict.fromkeys([0, 15, 16, 4095, 4096, S - 1]) if 0 <= o < S]


def degraded_flags(T, seed):
    """1 .. m - 1 erasures in every stripe (something is left to compare),
    stripe 0 with a data and a parity shard gone where m allows."""
    rng = np.random.default_rng(seed)
    er = np.zeros((T.stripes, T.n), dtype=np.uint8)
    for s in range(T.stripes):
        e = 1 + (s % (T.m - 1)) if T.m > 1 else 0
        er[s, rng.choice(T.n, size=e, replace=False)] = 1
    if T.m > 2:
        er[0] = 0
        er[0, [1, T.k + 1]] = 1
    return er


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("code,route", DAMAGE)
def test_one_wrong_byte_in_a_compared_shard(code, route, placement):
    """first_bad is that offset; the filled slots are the pristine shards."""
    S = 3 * 4096 + 40
    T, f = store(placement, code, S, 3), fec(code, route)
    er = degraded_flags(T, 5)
    rng = np.random.default_rng(S)
    for c, off in enumerate(special_offsets(S)):
        run = Run(T, er, seed=c)
        s = c % 3
        U = run.compared(s)
        run.flip(s, U[c % len(U)], off, int(rng.integers(1, 256)))
        got = run.run(f, f"compared shard, offset {off}")
        assert got.tolist() == [off if x == s else CLEAN for x in range(3)]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("code,route", DAMAGE)
def test_one_wrong_byte_in_a_survivor(code, route, placement):
    """first_bad is that offset, and the filled slots equal the oracle's
    rebuild from the damaged survivors: wrong at that column, and only there."""
    S = 4112 + 9
    T, f = store(placement, code, S, 3), fec(code, route)
    er = degraded_flags(T, 6)
    rng = np.random.default_rng(S)
    for c, off in enumerate(special_offsets(S)):
        run = Run(T, er, seed=c)
        s = c % 3
        C = run.survivors(s)
        run.flip(s, C[(5 * c) % len(C)], off, int(rng.integers(1, 256)))
        got = run.run(f, f"survivor, offset {off}")
        assert got.tolist() == [off if x == s else CLEAN for x in range(3)]
        for i in np.flatnonzero(er[s]):  # the damage went into every regenerated shard
            assert run.slot(run.want, s, i, off, off + 1)[0] != T.shard(s, i)[off]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("code,route,S", [("rs10_14", None, 5000), ("rs64_80", "fused", 4112 - 7),
                                          ("rs64_80", "split", 4112 - 7), ("rs3_19", None, 3 * 4096 + 40)])
def test_wrong_bytes_beyond_shard_len_are_clean(code, route, S, placement):
    """Flips in [shard_len, round_up 16) of compared shards and of survivors
    are not reported (the survivors' pads still go into the coded pad), nor are
    flips in the pitch gap, which nothing reads."""
    T, f = store(placement, code, S, 3), fec(code, route)
    run = Run(T, degraded_flags(T, 7))
    for s in range(3):
        for i in (run.compared(s)[0], run.survivors(s)[0], run.survivors(s)[-1]):
            for off in list(range(S, r16(S))) + [r16(S), T.slot_bytes - 1]:
                run.flip(s, i, off, 0xA5)
    assert (run.run(f, "pad") == CLEAN).all()
    run = Run(T, degraded_flags(T, 7))
    run.flip(2, run.compared(2)[-1], S, 0x11)
    run.flip(2, run.compared(2)[-1], S - 1, 0x80)
    assert run.run(f, "pad and last byte").tolist() == [CLEAN, CLEAN, S - 1]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("code,route", DAMAGE)
def test_damage_in_two_stripes_of_37(code, route, placement):
    """The others are clean, and first_bad is the lowest offset when several
    bytes are wrong: in one compared shard, in two, in a survivor and a
    compared shard."""
    S = 5000
    T, f = store(placement, code, S, 37), fec(code, route)
    er = degraded_flags(T, 8)
    run = Run(T, er)
    a, b = 5, 36
    Ua, Ub = run.compared(a), run.compared(b)
    run.flip(a, Ua[0], 4097, 0x01)
    run.flip(a, Ua[0], 300, 0x80)
    run.flip(a, Ua[-1], 299 if len(Ua) > 1 else 4999, 0x10)
    run.flip(b, run.survivors(b)[3 % T.k], 4096, 0x04)
    run.flip(b, Ub[0], 4999, 0x40)
    before = count_stats(f)
    got = run.run(f, "two of 37")
    want = [CLEAN] * 37
    want[a], want[b] = (299 if len(Ua) > 1 else 300), 4096
    assert got.tolist() == want
    assert_stats(f, before, er, T.m, route != "split")


# ------------------------------------ 3. agrees with the two calls it fuses ----
def damaged_run(T, seed):
    """Mixed 0 .. m erasures and, in two stripes of three, one or two wrong
    bytes anywhere in the present shards."""
    rng = np.random.default_rng(seed)
    er = erasure_rounds(T.k, T.n, T.stripes, seed)[0]
    run = Run(T, er, seed=seed)
    for s in range(T.stripes):
        for _ in range(s % 3):
            i = run.present(s)[int(rng.integers(len(run.present(s))))]
            off = int(rng.integers(r16(T.S)))
            if off not in run.flips.get((s, i), []):
                run.flip(s, i, off, int(rng.integers(1, 256)))
    return run


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("code,route,S,stripes", [c for c in CASES if c[3] == 37])
def test_agrees_with_verify_then_reconstruct(code, route, S, stripes, placement):
    """Two copies of one damaged image: the new call's first_bad equals
    rs_verify_degraded's (rs_verify_ptrs') and its image equals
    rs_reconstruct_stripes' (rs_reconstruct_ptrs'), pad bytes included."""
    T, f = store(placement, code, S, stripes), fec(code, route)
    one, two = damaged_run(T, S + 1), damaged_run(T, S + 1)
    assert all(np.array_equal(a, b) for a, b in zip(one.cur, two.cur))
    got = one.call(f)
    ref = two.two_calls(f)
    assert np.array_equal(got, ref), (got.tolist(), ref.tolist())
    assert (got != CLEAN).any() and (got == CLEAN).any()
    one.check("against the two calls", want=two.image())
    one.expect()  # and both are what the oracle says
    assert np.array_equal(got, one.fb)
    one.check("against the oracle")


# ------------------------------------------- addresses around bit 31 ----
@pytest.mark.parametrize("code,route", [("rs10_14", None), ("rs64_80", "fused"), ("rs64_80", "split")])
def test_addresses_across_a_2gib_boundary(code, route):
    """The pool lies across an address whose low 32 bits are 0x80000000, so the
    shards' addresses -- survivors, compared shards and destinations -- have
    bit 31 of their low word clear (rows below it) and set (rows above it):
    the kernel has to carry them as unsigned 64-bit values through its scalar
    registers and the LDS."""
    span = (4 << 30) + (16 << 20)
    free, _ = torch.cuda.mem_get_info()
    if free < span + (1 << 30):
        pytest.skip(f"needs {(span >> 30) + 2} GiB free on the device, {free >> 30} GiB are")
    T, f = store("ptrs", code, 4112, 3), fec(code, route)
    er = degraded_flags(T, 9)
    er[0] = 0  # stripe 0 loses the shards in its lowest and its highest row: destinations on both sides
    er[0, [int(np.argmin(T.G.rows[0])), int(np.argmax(T.G.rows[0]))]] = 1
    run = Run(T, er, seed=6)
    run.flip(1, run.compared(1)[0], 4100, 0x20)
    run.flip(2, run.survivors(2)[0], 17, 0x02)
    run.expect()
    big = torch.empty(span, dtype=torch.uint8, device="cuda:0")  # only the pool's bytes are ever touched
    half = len(run.cur[0]) // 2 // 16 * 16
    off = ((2 << 30) - half - big.data_ptr()) % (4 << 30)
    run.upload((big, off))
    low = run.host_table & 0xFFFFFFFF
    assert (low < (1 << 31)).any() and (low >= (1 << 31)).any()
    dst = low.reshape(3, T.n)[er != 0]
    assert (dst < (1 << 31)).any() and (dst >= (1 << 31)).any()
    got = run.call(f, upload=False)
    assert got.tolist() == [CLEAN, 4100, 17]
    run.check("across 2 GiB")
    del run.dev, big
    torch.cuda.empty_cache()


# ----------------------------------------------------------- refusals ----
@pytest.mark.parametrize("route", [None, "split"])
def test_refusals_write_nothing(route):
    lib = rsmi.load()
    code = "rs10_14"
    f = fec(code, route)
    for placement in PLACEMENTS:
        T = store(placement, code, 4112, 3)
        er = np.zeros((3, T.n), dtype=np.uint8)
        er[1, [0, 5, 10, 13]] = 1
        er[2, 3] = 1
        run = Run(T, er)
        run.flip(0, 3, 7, 0x10)
        run.upload()
        fbp = run.first_bad.data_ptr()

        def call(args=None, flags=er, fb=fbp, h=f._h):
            buf = ctypes.c_char_p(flags.tobytes()) if flags is not None else None
            a = list(run.args() if args is None else args)
            fn = lib.rs_reconstruct_checked_ptrs if placement == "ptrs" else lib.rs_reconstruct_checked
            return fn(h, *a, ctypes.cast(buf, ctypes.c_void_p), fb, None)

        too_many = er.copy()
        too_many[1, 7] = 1  # m + 1 erasures, behind a stripe that could be repaired
        assert call(flags=too_many) == rsmi.RS_ENOT_ENOUGH
        with pytest.raises(rsmi.NotEnoughShares):
            if placement == "ptrs":
                f.reconstruct_checked_ptrs(*run.args(), too_many.tobytes(), fbp)
            else:
                f.reconstruct_checked(*run.args(), too_many.tobytes(), fbp)
        assert call(h=None) == rsmi.RS_EINVAL
        assert call(flags=None) == rsmi.RS_EINVAL
        assert call(fb=None) == rsmi.RS_EINVAL
        assert call(fb=fbp + 2) == rsmi.RS_EINVAL
        a = list(run.args())
        if placement == "ptrs":
            assert call(args=[None] + a[1:]) == rsmi.RS_EINVAL          # a NULL table
            assert call(args=[a[0] + 4] + a[1:]) == rsmi.RS_EINVAL      # a misaligned one
            assert call(args=[a[0], 1 << 32, a[2]]) == rsmi.RS_EINVAL   # the column limit
            assert call(args=[a[0], a[1], 1 << 32]) == rsmi.RS_EINVAL   # 2^32 stripes
            assert call(args=[a[0], a[1], 0], flags=None, fb=None) == rsmi.RS_OK
            assert call(args=[a[0], 0, a[2]], flags=None, fb=None) == rsmi.RS_OK
        else:
            assert call(args=[None] + a[1:]) == rsmi.RS_EINVAL          # NULL data
            assert call(args=[a[0] + 4] + a[1:]) == rsmi.RS_EINVAL      # misaligned data
            assert call(args=a[:4] + [r16(a[5]) - 16] + a[5:]) == rsmi.RS_EINVAL  # pitch below the coded span
            assert call(args=a[:4] + [a[4] + 8] + a[5:]) == rsmi.RS_EINVAL        # misaligned pitch
            assert call(args=a[:4] + [1 << 33, 1 << 32, a[6]]) == rsmi.RS_EINVAL  # the column limit
            assert call(args=a[:6] + [1 << 32]) == rsmi.RS_EINVAL                 # 2^32 stripes
            assert call(args=a[:6] + [0], flags=None, fb=None) == rsmi.RS_OK
            assert call(args=a[:5] + [0, a[6]], flags=None, fb=None) == rsmi.RS_OK
        f.sync()
        run.check(f"refused calls, {placement}", want=run.cur)
        assert run.verdicts().tolist() == [SENTINEL] * 3


def test_no_parity_is_clean():
    """An RS(4,4) context: no flag can be set, and every stripe is clean."""
    f = rsmi.FEC(4, 4, device=0)
    S, stripes = 4112, 3
    host = np.random.default_rng(3).integers(0, 256, size=stripes * 4 * r16(S), dtype=np.uint8)
    buf = torch.from_numpy(host.copy()).cuda()
    table = torch.from_numpy(buf.data_ptr() + np.arange(stripes * 4, dtype=np.int64) * r16(S)).cuda()
    for ptrs in (False, True):
        fb = torch.full((stripes,), SENTINEL, dtype=torch.int32, device="cuda:0")
        if ptrs:
            f.reconstruct_checked_ptrs(table.data_ptr(), S, stripes, bytes(stripes * 4), fb.data_ptr())
        else:
            f.reconstruct_checked(buf.data_ptr(), 4 * r16(S), 0, 0, r16(S), S, stripes, bytes(stripes * 4), fb.data_ptr())
        f.sync()
        assert fb.cpu().numpy().view(np.uint32).tolist() == [CLEAN] * 3
        one = bytearray(stripes * 4)
        one[5] = 1
        with pytest.raises(rsmi.NotEnoughShares):
            if ptrs:
                f.reconstruct_checked_ptrs(table.data_ptr(), S, stripes, bytes(one), fb.data_ptr())
            else:
                f.reconstruct_checked(buf.data_ptr(), 4 * r16(S), 0, 0, r16(S), S, stripes, bytes(one), fb.data_ptr())
    assert np.array_equal(buf.cpu().numpy(), host)
    f.close()


# ------------------------------------------- kernel names, the counter ----
@pytest.mark.parametrize("code", sorted(REPAIR_NAME))
def test_kernel_names(code):
    f = fec(code)
    assert f.kernel_name(12) == REPAIR_NAME[code]
    assert f.kernel_name(13) == REPAIR_NAME[code] + "_ptrs"
    assert f.kernel_name(5) == REPAIR_NAME[code].replace("repair", "check")


def test_intact_stripes_are_not_counted():
    """No flag set at all: the call is rs_verify_stripes, whatever the route."""
    for route in (None, "split"):
        f = fec("rs10_14", route)
        for placement in PLACEMENTS:
            T = store(placement, "rs10_14", 4112, 3)
            before = count_stats(f)
            run = Run(T, np.zeros((3, T.n), dtype=np.uint8))
            run.flip(1, 12, 4111, 0x08)
            run.flip(2, 4, 16, 0x08)
            assert run.run(f, "no flags").tolist() == [CLEAN, 4111, 16]
            assert count_stats(f) == before


# ------------------------------------------ device set, threads, caches ----
def test_device_set():
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert fs.kernel_name(12) == "repair_K10_MG4_B256" and fs.kernel_name(13) == "repair_K10_MG4_B256_ptrs"
    for placement in PLACEMENTS:
        T = store(placement, "rs10_14", 5000, 3)
        before = fs.stat(fs.STAT_REPAIR_CHECKED)
        run = Run(T, degraded_flags(T, 10))
        run.flip(1, run.survivors(1)[2], 4096, 0x33)
        assert run.run(fs, f"device set, {placement}").tolist() == [CLEAN, 4096, CLEAN]
        assert fs.stat(fs.STAT_REPAIR_CHECKED) - before == 3  # summed over the members
    fs.close()


def test_two_threads_one_context():
    f = fec("rs10_14")
    stores = [Strided("rs10_14", 5000, 3), Pointer("rs10_14", 5000, 3)]  # built ahead of the threads
    runs = []
    for t, T in enumerate(stores):
        mine = []
        for rep in range(4):
            run = Run(T, erasure_rounds(T.k, T.n, 3, seed=10 * t + rep)[rep % 2], seed=rep)
            s = rep % 3
            if run.compared(s):
                run.flip(s, run.compared(s)[0], 1000 + rep, 0x01)
            mine.append(run.expect())
        runs.append(mine)
    errors = []

    def work(t):
        try:
            for rep, run in enumerate(runs[t]):
                got = run.call(f)
                assert np.array_equal(got, run.fb), (got.tolist(), run.fb.tolist())
                run.check(f"thread {t} rep {rep}")
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_pattern_cache_is_shared(placement):
    """A second call with the same patterns builds none; rs_reconstruct_stripes
    with the same flags on the same context then finds the saturated stripes'
    patterns (X' = X) in the cache the checked repair filled."""
    f = rsmi.FEC(10, 14, device=0)
    T = store(placement, "rs10_14", 4112, 3)
    er = np.zeros((3, T.n), dtype=np.uint8)
    er[0, [0, 1, 2, 3]] = 1     # saturated
    er[1, [10, 11, 12, 13]] = 1  # saturated, all parity
    er[2, [4, 12]] = 1          # X' = {4, 10, 11, 12}
    run = Run(T, er)
    run.flip(2, 11, 5, 0x01)
    assert run.run(f, "first").tolist() == [CLEAN, CLEAN, 5]
    built = f.pattern_count()
    assert built == 3
    again = Run(T, er, seed=1)
    again.flip(2, 10, 6, 0x01)
    assert again.run(f, "cache hit").tolist() == [CLEAN, CLEAN, 6]
    assert f.pattern_count() == built
    # the plain reconstruct: stripes 0 and 1 hit, stripe 2 (X = {4, 12}) is new
    plain = Run(T, er, seed=2).expect().upload()
    if placement == "ptrs":
        f.reconstruct_ptrs(*plain.args(), er.tobytes())
    else:
        f.reconstruct_stripes(*plain.args(), er.tobytes())
    f.sync()
    plain.check("reconstruct on the shared cache")
    assert f.pattern_count() == built + 1
    f.close()

"""GPU: rs_verify_ptrs and rs_correct_columns_ptrs -- the scrub of the pointer
placement (shard i of stripe s at shard_ptrs[s * n + i], anywhere in device
memory).

Every case works on a strided_image.Pool: the shards at random rows of one
buffer, row padding behind round_up(S, 16), decoy rows that no present shard
lives in, guard bands around the buffer, all random bytes.  The table entries
of erased shards point at DECOY rows (valid memory, so a mistake shows as a
wrong byte or a changed decoy, never as a fault), and the erased shards' own
rows are overwritten with random bytes no table entry names.  After every call
the WHOLE pool buffer and the device table are compared with the expected
image.  Expected bytes never come from the engine: they are the pristine pool
(payload seeded, parity from the oracle) and, for columns beyond the radius,
oracle.decode_correct on that one column re-encoded with the oracle.
"""
import ctypes
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from oracle import oracle  # noqa: E402
from strided_image import GUARD, Layout, Pool, r16  # noqa: E402

CLEAN = rsmi.RS_VERIFY_CLEAN
OK, TOO_MANY = rsmi.RS_OK, rsmi.RS_ETOO_MANY_ERRORS
# register pointers, MG4 | MG8 | MG16, r > k + 8 | LDS pointer path, two rounds
# of 32 column sources | r up to 256
CODES = {"rs4_6": (4, 6), "rs10_14": (10, 14), "rs8_14": (8, 14), "rs3_19": (3, 19), "rs64_80": (64, 80),
         "rs240_256": (240, 256), "rs4_5": (4, 5), "rs12_40": (12, 40)}
CHECK_NAME = {"rs4_6": "check_K4_MG4_B256", "rs10_14": "check_K10_MG4_B256", "rs8_14": "check_K8_MG4_B256",
              "rs3_19": "check_K0_MG4_B256", "rs64_80": "check_K64_MG4_B256", "rs240_256": "check_K0_MG4_B256"}
COLUMN_NAME = {"rs4_6": "columns_MG4_B256", "rs10_14": "columns_MG4_B256", "rs8_14": "columns_MG8_B256",
               "rs3_19": "columns_MG16_B256", "rs64_80": "columns_MG16_B256", "rs240_256": "columns_MG16_B256"}
# one column | exactly one 4 KiB block chunk | a chunk plus one column | not a
# multiple of 16 | several chunks
SHAPES = [16, 4096, 4112, 5000, 3 * 4096 + 40]
STRIPES = [1, 3, 37]
CASES = ([(c, S, st) for c in ("rs4_6", "rs10_14", "rs8_14", "rs3_19", "rs64_80") for S in SHAPES for st in STRIPES] +
         [("rs240_256", S, st) for S in (16, 4112) for st in STRIPES])

_POOLS = {}
_FECS = {}
_MATRIX = {}


def pool(code, S, stripes):
    key = (code, S, stripes)
    if key not in _POOLS:
        while len(_POOLS) >= 6:
            del _POOLS[next(iter(_POOLS))]
        k, n = CODES[code]
        _POOLS[key] = Pool(k, n, S, stripes, seed=k * 1000003 + n * 10007 + S * 31 + stripes)
    return _POOLS[key]


def fec(code):
    if code not in _FECS:
        _FECS[code] = rsmi.FEC(*CODES[code], device=0)
    return _FECS[code]


def matrix(k, n):
    if (k, n) not in _MATRIX:
        _MATRIX[(k, n)] = oracle.fec_matrix(k, n)
    return _MATRIX[(k, n)]


def oracle_column(k, n, shares):
    """The oracle's Correct on one byte column: shares = [(number, byte)].
    (status, the n bytes of the codeword it found, or None)."""
    E = matrix(k, n)
    rc, data = oracle.decode_correct(E, k, n, [(i, bytes([b])) for i, b in shares])
    if rc != 0:
        return rc, None
    return rc, list(data) + list(oracle.encode(E, k, n, data))


def rebuild_choice(k, n, er_row):
    """Rebuild's survivors: every present data share, then the highest present parity."""
    c = [i for i in range(k) if not er_row[i]]
    for i in range(n - 1, k - 1, -1):
        if len(c) < k and not er_row[i]:
            c.append(i)
    return sorted(c)


class Run:
    """The host model of calls on one pool: `cur` is what the pool buffer holds
    before a call, `want` what it must hold afterwards (the pristine pool but
    for the erased shards' rows, unless a test says otherwise), `counts` the
    per-shard bytes a correcting call must report, `er` the erasure flags."""

    def __init__(self, P, gone=None, seed=0):
        self.P = P
        self.cur = P.pristine[0].copy()
        self.want = P.pristine[0].copy()
        self.counts = np.zeros((P.stripes, P.n), dtype=np.int64)
        self.er = np.zeros((P.stripes, P.n), dtype=np.uint8)
        self.entry_row = P.rows.copy()  # the row each table entry names
        rng = np.random.default_rng(900 + seed)
        for s, shards in (gone or {}).items():
            for i in shards:
                self.er[s, i] = 1
                o = P.row_at(P.rows[s, i])
                g = rng.integers(0, 256, size=P.row_bytes, dtype=np.uint8)
                self.cur[o:o + P.row_bytes] = g  # the lost shard: nothing names this row any more
                self.want[o:o + P.row_bytes] = g
                self.entry_row[s, i] = P.decoys[int(rng.integers(len(P.decoys)))]
        self.dev = self.table = self.host_table = None

    def flags(self):
        return self.er.tobytes() if self.er.any() else None

    def present(self, s):
        return [i for i in range(self.P.n) if not self.er[s, i]]

    def at(self, s, i):
        return self.P.row_at(self.P.rows[s, i])

    def pristine_byte(self, s, i, off):
        return int(self.P.pristine[0][self.at(s, i) + off])

    def flip(self, s, i, off, mask, counted=True):
        """XORs mask into byte off of present shard i of stripe s (once per byte)."""
        o = self.at(s, i) + off
        assert mask and not self.er[s, i] and self.cur[o] == self.P.pristine[0][o]
        self.cur[o] ^= mask
        if counted:
            self.counts[s, i] += 1

    def column(self, s, off):
        return [(i, int(self.cur[self.at(s, i) + off])) for i in self.present(s)]

    def keep_column(self, s, off):
        """The call must leave column off of stripe s as it is now."""
        for i in self.present(s):
            o = self.at(s, i) + off
            self.want[o] = self.cur[o]
            self.counts[s, i] -= int(self.cur[o] != self.P.pristine[0][o])

    def expect_column(self, s, off, word):
        """The call must turn column off of stripe s into `word` (n bytes)."""
        for i in self.present(s):
            o = self.at(s, i) + off
            self.counts[s, i] += int(word[i] != self.cur[o]) - int(self.cur[o] != self.P.pristine[0][o])
            self.want[o] = word[i]

    def upload(self, within=None):
        """within: a device buffer and a 16-byte-aligned offset in it at which the pool goes."""
        if within is None:
            self.dev = torch.from_numpy(self.cur).cuda()
        else:
            self.dev = within[0][within[1]:within[1] + len(self.cur)]
            self.dev.copy_(torch.from_numpy(self.cur))
        self.host_table = self.dev.data_ptr() + GUARD + self.entry_row.astype(np.int64) * self.P.row_bytes
        assert (self.host_table % 16 == 0).all()
        self.table = torch.from_numpy(self.host_table.reshape(-1).copy()).cuda()
        return self.table.data_ptr()

    def verify(self, f, upload=True, flags="own"):
        """first_bad of rs_verify_ptrs over the pool as it is now."""
        if upload:
            self.upload()
        fb = torch.zeros(self.P.stripes, dtype=torch.int32, device="cuda:0")
        f.verify_ptrs(self.table.data_ptr(), self.P.S, self.P.stripes, fb.data_ptr(),
                      erased=self.flags() if flags == "own" else flags)
        f.sync()
        return fb.cpu().numpy().view(np.uint32)

    def correct(self, f, within=None):
        tp = self.upload(within)
        st, cnt = f.correct_columns_ptrs(tp, self.P.S, self.P.stripes, erased=self.flags())
        return st, np.asarray(cnt, dtype=np.int64).reshape(self.P.stripes, self.P.n)

    def check(self, what="", want=None):
        want = self.want if want is None else want
        g = self.dev.cpu().numpy()
        bad = np.flatnonzero(g != want)
        assert bad.size == 0, f"{what} pool: {bad.size} bytes differ, first offsets {bad[:8].tolist()}"
        assert np.array_equal(self.table.cpu().numpy(), self.host_table.reshape(-1)), f"{what}: the table changed"


def mask_of(rng):
    return int(rng.integers(1, 256))


def erasures(P, e, seed, stripes=None):
    """e erasures in each of the listed stripes (default: all): one in the
    data, one in the parity where e allows, the rest anywhere."""
    rng = np.random.default_rng(seed)
    gone = {}
    for s in range(P.stripes) if stripes is None else stripes:
        if e == 0:
            continue
        ids = [int(rng.integers(P.k))]
        if e > 1:
            ids.append(int(P.k + rng.integers(P.m)))
        while len(ids) < e:
            i = int(rng.integers(P.n))
            if i not in ids:
                ids.append(i)
        gone[s] = sorted(ids)
    return gone


def special_offsets(S):
    """The first and the last byte and both sides of every 4096 boundary."""
    offs = [0, S - 1]
    for b in range(4096, S, 4096):
        offs += [b - 1, b]
    return list(dict.fromkeys(o for o in offs if 0 <= o < S))


def scatter(run, s, rng, extra=6):
    """Damage of stripe s within the radius floor((r - k) / 2): at the special
    offsets and a few random ones, 1 .. radius flips in distinct present
    shards of the column (the first column exactly at the radius), the shards
    rotating from column to column."""
    P = run.P
    present = run.present(s)
    radius = (len(present) - P.k) // 2
    if radius == 0:
        return
    special = special_offsets(P.S)
    rest = [int(o) for o in rng.permutation(P.S)[:extra + len(special)] if int(o) not in special][:extra]
    at = int(rng.integers(len(present)))
    for c, off in enumerate(special + rest):
        w = radius if c == 0 else int(rng.integers(1, radius + 1))
        for j in range(w):
            run.flip(s, present[(at + j) % len(present)], off, mask_of(rng))
        at += w


def check_corrected(f, run, what):
    P = run.P
    columns = f.stat(f.STAT_COLUMN_STRIPES)
    corrected = f.stat(f.STAT_COLUMN_BYTES)
    st, cnt = run.correct(f)
    assert st == [OK] * P.stripes, what
    run.check(what)
    assert np.array_equal(cnt, run.counts), (what, np.argwhere(cnt != run.counts)[:8].tolist())
    assert f.stat(f.STAT_COLUMN_STRIPES) - columns == int((run.counts.sum(axis=1) > 0).sum())
    assert f.stat(f.STAT_COLUMN_BYTES) - corrected == int(run.counts.sum())
    assert np.array_equal(run.verify(f, upload=False), np.full(P.stripes, CLEAN, dtype=np.uint32)), what
    run.check(what + ", verified")


# ------------------------------------------------------ 1. verify, clean ----
@pytest.mark.parametrize("code,S,stripes", CASES)
def test_verify_clean(code, S, stripes):
    P, f = pool(code, S, stripes), fec(code)
    clean = np.full(stripes, CLEAN, dtype=np.uint32)
    run = Run(P)
    assert np.array_equal(run.verify(f), clean)
    assert np.array_equal(run.verify(f, upload=False, flags=bytes(stripes * P.n)), clean)
    run.check("no flags")
    # e = 1 .. m - 1 erasures, and the last stripe with exactly m: its present shards may hold anything
    gone = {s: erasures(P, 1 + (s % max(P.m - 1, 1)), 40 + s, [s])[s] for s in range(stripes) if P.m > 1}
    gone[stripes - 1] = erasures(P, P.m, 7, [stripes - 1])[stripes - 1]
    run = Run(P, gone, seed=1)
    for i in run.present(stripes - 1)[:3]:
        o = run.at(stripes - 1, i)
        run.cur[o] ^= 0x5A
        run.want[o] ^= 0x5A
    checked = f.stat(f.STAT_CHECK_STRIPES)
    assert np.array_equal(run.verify(f), clean)
    run.check("flags")
    assert f.stat(f.STAT_CHECK_STRIPES) - checked == sum(1 for s in gone if len(gone[s]) < P.m)


# ---------------------------------------------------- 2. verify, damaged ----
def damage_targets(P, er_row):
    """A data shard, a parity shard Rebuild uses and one it does not use (where
    the erasure set leaves such shards)."""
    chosen = rebuild_choice(P.k, P.n, er_row)
    data = [i for i in chosen if i < P.k]
    used = [i for i in chosen if i >= P.k]
    unused = [i for i in range(P.k, P.n) if not er_row[i] and i not in chosen]
    return [t[len(t) // 2] for t in (data, used, unused) if t]


@pytest.mark.parametrize("code,S,stripes", CASES)
def test_verify_damaged(code, S, stripes):
    P, f = pool(code, S, stripes), fec(code)
    offsets = [o for o in (0, S - 1, 4095, 4096) if o < S]
    for e in sorted({0, 1, P.m - 1}):
        run = Run(P, erasures(P, e, 11 * e + S), seed=e)
        rng = np.random.default_rng(e + S + stripes)
        want = np.full(stripes, CLEAN, dtype=np.uint32)
        # every other stripe damaged (all of one or three), each at one target and one or two offsets
        for s in range(0, stripes, 2):
            targets = damage_targets(P, run.er[s])
            assert e == P.m or targets
            i = targets[(s // 2) % len(targets)]
            offs = [offsets[(s // 2) % len(offsets)], offsets[(s // 2 + 1) % len(offsets)]][:1 + (s // 2) % 2]
            for off in set(offs):
                run.flip(s, i, off, mask_of(rng))
            want[s] = min(offs)
        if stripes == 1:  # the one stripe: every target and every offset in turn
            for i in damage_targets(P, run.er[0]):
                for off in offsets:
                    one = Run(P, {0: [x for x in range(P.n) if run.er[0, x]]}, seed=e)
                    one.flip(0, i, off, mask_of(rng))
                    assert one.verify(f).tolist() == [off], (e, i, off)
        run.want = run.cur.copy()
        got = run.verify(f)
        assert np.array_equal(got, want), (e, got.tolist(), want.tolist())
        run.check(f"damaged e={e}")


@pytest.mark.parametrize("code,S", [("rs10_14", 5000), ("rs64_80", 4112 - 7), ("rs4_6", 3 * 4096 + 40)])
def test_verify_ignores_the_pad(code, S):
    """Flips inside [S, round_up(S, 16)) and in the row padding are not reported."""
    P, f = pool(code, S, 3), fec(code)
    for gone in (None, {1: [0, P.n - 1]}):
        run = Run(P, gone)
        for s in range(3):
            for i in run.present(s)[::3]:
                for off in list(range(S, r16(S))) + [r16(S), P.row_bytes - 1]:
                    run.cur[run.at(s, i) + off] ^= 0xA5
        run.want = run.cur.copy()
        assert run.verify(f).tolist() == [CLEAN] * 3
        run.flip(2, run.present(2)[-1], S - 1, 0x80)
        run.want = run.cur.copy()
        assert run.verify(f).tolist() == [CLEAN, CLEAN, S - 1]
        run.check("pad")


# ------------------------------------ 3. verify agrees with the strided call ----
@pytest.mark.parametrize("code,S,stripes", [(c, S, 37) for c in ("rs10_14", "rs8_14", "rs3_19", "rs64_80")
                                            for S in (4112, 5000)] + [("rs4_6", 3 * 4096 + 40, 3),
                                                                      ("rs240_256", 4112, 3)])
def test_verify_agrees_with_strided(code, S, stripes):
    """The same stripes with the same damage in a Layout and in a Pool:
    rs_verify_ptrs equals rs_verify_stripes / rs_verify_degraded word for word."""
    k, n = CODES[code]
    P, f = pool(code, S, stripes), fec(code)
    L = Layout(k, n, S, stripes, seed=5, mode="split")
    assert np.array_equal(L.payload, P.payload) and np.array_equal(L.ref, P.ref)
    for e in (0, 1, P.m - 1):
        gone = erasures(P, e, 3 * e + 1, [s for s in range(stripes) if s % 3 != 1])
        run = Run(P, gone, seed=e)
        bufs = [b.copy() for b in L.pristine]
        rng = np.random.default_rng(S + e)
        for s in range(stripes):
            for _ in range(s % 3):  # 0, 1 or 2 flips: a third of the stripes stays clean
                i = run.present(s)[int(rng.integers(len(run.present(s))))]
                off = int(rng.integers(S))
                if run.cur[run.at(s, i) + off] != run.pristine_byte(s, i, off):
                    continue
                mk = mask_of(rng)
                run.flip(s, i, off, mk)
                b, o = L.shard_at(s, i)
                bufs[b][o + off] ^= mk
        run.want = run.cur.copy()
        got = run.verify(f)
        dev = [torch.from_numpy(b).cuda() for b in bufs]
        fb = torch.zeros(stripes, dtype=torch.int32, device="cuda:0")
        args = L.args([d.data_ptr() for d in dev])
        if e == 0:
            f.verify_stripes(*args, fb.data_ptr())
        else:
            f.verify_degraded(*args, run.er.tobytes(), fb.data_ptr())
        f.sync()
        strided = fb.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, strided), (e, got.tolist(), strided.tolist())
        assert (got != CLEAN).any() and (got == CLEAN).any() or stripes < 3
        run.check(f"agree e={e}")


# ----------------------------- 4. correct, scattered damage in the radius ----
@pytest.mark.parametrize("code,S,stripes", CASES)
def test_correct_scattered(code, S, stripes):
    P, f = pool(code, S, stripes), fec(code)
    for degraded in (False, True):
        gone = None
        if degraded:  # 1 .. m - 2 erasures (a radius of at least 1 stays), every third stripe whole
            gone = {s: erasures(P, 1 + (s % (P.m - 2)) if P.m > 2 else 0, 60 + s, [s]).get(s, [])
                    for s in range(stripes) if s % 3 != 2}
        run = Run(P, gone, seed=2)
        rng = np.random.default_rng(S + stripes + degraded)
        # the first and the last stripe and every fifth one between them; the others stay clean
        for s in sorted({0, stripes - 1} | set(range(2, stripes, 5))):
            scatter(run, s, rng)
        assert run.counts.sum() > 0
        check_corrected(f, run, f"{code} S={S} x{stripes} degraded={degraded}")
        assert not run.counts[run.er != 0].any()


# --------------------------------------------- 5. a wholly wrong shard ----
@pytest.mark.parametrize("code,S,stripes,gone", [("rs10_14", 5000, 3, None), ("rs10_14", 4112, 3, {2: [3]}),
                                                 ("rs64_80", 4112, 2, {1: [0, 70]}), ("rs3_19", 4096, 1, None),
                                                 ("rs8_14", 3 * 4096 + 40, 1, None)])
def test_correct_whole_shard(code, S, stripes, gone):
    """floor((r - k) / 2) shards of the last stripe wrong at (nearly) every
    byte: the counts are the differing bytes."""
    P, f = pool(code, S, stripes), fec(code)
    run, rng = Run(P, gone), np.random.default_rng(S)
    s = stripes - 1
    present = run.present(s)
    shards = [present[0], present[-1], present[len(present) // 2]][:(len(present) - P.k) // 2]
    for i in shards:
        o = run.at(s, i)
        mk = rng.integers(0, 256, size=S, dtype=np.uint8)  # a zero mask leaves a byte right
        run.cur[o:o + S] ^= mk
        run.counts[s, i] = int((mk != 0).sum())
    check_corrected(f, run, f"whole shard {code}")


# ------------------------------------------- addresses around bit 31 ----
@pytest.mark.parametrize("code,gone", [("rs10_14", {1: [3]}), ("rs64_80", {0: [0, 70]}), ("rs3_19", None)])
def test_addresses_across_a_2gib_boundary(code, gone):
    """The pool lies across an address whose low 32 bits are 0x80000000, so the
    shards' addresses have bit 31 of their low word clear (rows below it) and
    set (rows above it): every kernel has to carry the table's addresses as
    unsigned 64-bit values through its scalar registers and the LDS."""
    span = (4 << 30) + (16 << 20)
    free, _ = torch.cuda.mem_get_info()
    if free < span + (1 << 30):
        pytest.skip(f"needs {(span >> 30) + 2} GiB free on the device, {free >> 30} GiB are")
    P, f = pool(code, 4112, 3), fec(code)
    run, rng = Run(P, gone, seed=6), np.random.default_rng(31)
    for s in range(3):
        scatter(run, s, rng)
    big = torch.empty(span, dtype=torch.uint8, device="cuda:0")  # only the pool's bytes are ever touched
    half = len(run.cur) // 2 // 16 * 16
    off = ((2 << 30) - half - big.data_ptr()) % (4 << 30)
    within = (big, off)
    run.upload(within)
    low = run.host_table & 0xFFFFFFFF
    assert (low < (1 << 31)).any() and (low >= (1 << 31)).any()
    fb = run.verify(f, upload=False)
    assert (fb != CLEAN).all()
    st, cnt = run.correct(f, within)
    assert st == [OK] * 3
    run.check("across 2 GiB")
    assert np.array_equal(cnt, run.counts)
    assert run.verify(f, upload=False).tolist() == [CLEAN] * 3
    del run.dev, big
    torch.cuda.empty_cache()


# ---------------------------------------------------- 6. beyond radius ----
def find_column(run, s, seed, taken):
    """(offset, {shard: mask}): a column of radius + 1 errors of stripe s."""
    P = run.P
    rng = np.random.default_rng(seed)
    present = run.present(s)
    weight = (len(present) - P.k) // 2 + 1
    off = next(int(o) for o in rng.permutation(P.S) if int(o) not in taken)
    taken.add(off)
    return off, {int(i): mask_of(rng) for i in rng.choice(present, size=weight, replace=False)}


@pytest.mark.parametrize("code,gone", [("rs10_14", None), ("rs4_6", None), ("rs10_14", {1: [2], 2: [0, 13]}),
                                       ("rs64_80", {1: [5, 77]})])
def test_correct_beyond_radius(code, gone):
    """Stripes 1 and 2 hold columns of floor((r - k) / 2) + 1 errors among
    correctable ones.  What the oracle's Correct does with such a column is
    what the engine must do: leave it alone (the stripe ends
    RS_ETOO_MANY_ERRORS) or write the other codeword it finds.  Every other
    damaged column of those stripes is repaired."""
    P, f = pool(code, 5000, 3), fec(code)
    run, rng = Run(P, gone, seed=4), np.random.default_rng(77)
    taken, far = set(), []
    for s, seed in ((1, 11), (1, 12), (2, 13), (2, 14)):
        off, masks = find_column(run, s, seed, taken)
        for i, mk in masks.items():
            run.flip(s, i, off, mk)
        far.append((s, off))
    for s in range(3):  # correctable columns around them, next to the first one too
        near = [far[0][1] - 1, far[0][1] + 1] if s == 1 else []
        for off in [int(o) for o in rng.choice(P.S, size=10, replace=False)] + near:
            if 0 <= off < P.S and off not in taken:
                taken.add(off)
                run.flip(s, run.present(s)[int(rng.integers(len(run.present(s))))], off, mask_of(rng))
    want_st = [OK, OK, OK]
    want_fb = np.full(3, CLEAN, dtype=np.uint32)
    for s, off in far:
        rc, word = oracle_column(P.k, P.n, run.column(s, off))
        if rc != 0:
            run.keep_column(s, off)
            want_st[s] = TOO_MANY
            want_fb[s] = min(int(want_fb[s]), off)
        else:
            run.expect_column(s, off, word)
    st, cnt = run.correct(f)
    assert st == want_st
    run.check(f"beyond radius {code}")
    assert np.array_equal(cnt, run.counts), np.argwhere(cnt != run.counts)[:8].tolist()
    assert np.array_equal(run.verify(f, upload=False), want_fb)
    # the return value, through the C ABI, with NULL status and corrected
    tp = run.upload()
    er = run.flags()
    buf = ctypes.c_char_p(er) if er else None
    rc = rsmi.load().rs_correct_columns_ptrs(f._h, tp, P.S, 3, ctypes.cast(buf, ctypes.c_void_p), None, None, None)
    assert rc == (TOO_MANY if TOO_MANY in want_st else OK)
    run.check(f"beyond radius {code}, NULL status and corrected")


@pytest.mark.parametrize("code,gone", [("rs4_5", None), ("rs10_14", {1: [1, 2, 11]})])
def test_correct_radius_zero_is_unwritten(code, gone):
    """r - k < 2: an error can be seen but not located."""
    P, f = pool(code, 4112, 3), fec(code)
    run = Run(P, gone)
    run.flip(1, run.present(1)[2], 100, 0x40, counted=False)
    run.flip(0, 0, 4111, 0x01, counted=P.m >= 2)  # a whole stripe next to it: repaired where the code can
    run.want = run.cur.copy()
    if P.m >= 2:
        o = run.at(0, 0) + 4111
        run.want[o] = P.pristine[0][o]
    st, cnt = run.correct(f)
    assert st == [OK if P.m >= 2 else TOO_MANY, TOO_MANY, OK]
    assert np.array_equal(cnt, run.counts)
    run.check("radius 0")


# ------------------------------------------------------- 8. refusals ----
def test_refusals():
    P, f = pool("rs10_14", 4112, 3), fec("rs10_14")
    run = Run(P, {1: [0, 5, 10, 13]})
    run.flip(0, 3, 7, 0x10, counted=False)  # repairable, but a refused call writes nothing
    run.want = run.cur.copy()
    tp = run.upload()
    lib = rsmi.load()
    fb = torch.full((3,), 0x7A7A7A7A, dtype=torch.int32, device="cuda:0")
    st = (ctypes.c_int * 3)(9, 9, 9)
    er = run.er.copy()
    er[1, 7] = 1  # m + 1 erasures
    buf = ctypes.c_char_p(er.tobytes())
    erp = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.rs_verify_ptrs(f._h, tp, P.S, 3, erp, fb.data_ptr(), None) == rsmi.RS_ENOT_ENOUGH
    assert lib.rs_correct_columns_ptrs(f._h, tp, P.S, 3, erp, st, None, None) == rsmi.RS_ENOT_ENOUGH
    with pytest.raises(rsmi.NotEnoughShares):
        f.correct_columns_ptrs(tp, P.S, 3, erased=er.tobytes())
    # a misaligned table, a misaligned or NULL first_bad, a NULL table
    assert lib.rs_verify_ptrs(f._h, tp + 4, P.S, 3, None, fb.data_ptr(), None) == rsmi.RS_EINVAL
    assert lib.rs_verify_ptrs(f._h, tp, P.S, 3, None, fb.data_ptr() + 2, None) == rsmi.RS_EINVAL
    assert lib.rs_verify_ptrs(f._h, tp, P.S, 3, None, None, None) == rsmi.RS_EINVAL
    assert lib.rs_verify_ptrs(f._h, None, P.S, 3, None, fb.data_ptr(), None) == rsmi.RS_EINVAL
    assert lib.rs_correct_columns_ptrs(f._h, tp + 4, P.S, 3, None, st, None, None) == rsmi.RS_EINVAL
    assert lib.rs_correct_columns_ptrs(f._h, None, P.S, 3, None, st, None, None) == rsmi.RS_EINVAL
    # too long a shard, too many stripes
    assert lib.rs_verify_ptrs(f._h, tp, 1 << 32, 3, None, fb.data_ptr(), None) == rsmi.RS_EINVAL
    assert lib.rs_verify_ptrs(f._h, tp, P.S, 1 << 32, None, fb.data_ptr(), None) == rsmi.RS_EINVAL
    assert lib.rs_correct_columns_ptrs(f._h, tp, 1 << 32, 3, None, st, None, None) == rsmi.RS_EINVAL
    assert lib.rs_correct_columns_ptrs(f._h, tp, P.S, 1 << 32, None, None, None, None) == rsmi.RS_EINVAL
    # m = 28 > 16: the correcting call is not served
    wide = fec("rs12_40")
    assert wide.kernel_name(11) == "none"
    assert lib.rs_correct_columns_ptrs(wide._h, tp, P.S, 1, None, st, None, None) == rsmi.RS_EINVAL
    # nothing to do
    assert lib.rs_verify_ptrs(f._h, tp, P.S, 0, None, None, None) == rsmi.RS_OK
    assert lib.rs_verify_ptrs(f._h, tp, 0, 3, None, None, None) == rsmi.RS_OK
    assert lib.rs_correct_columns_ptrs(f._h, tp, 0, 3, None, None, None, None) == rsmi.RS_OK
    f.sync()
    run.check("refused calls")
    assert fb.cpu().numpy().view(np.uint32).tolist() == [0x7A7A7A7A] * 3
    assert list(st) == [9, 9, 9]


def test_no_parity_is_ok():
    """An RS(4,4) context: every stripe is a codeword."""
    f = rsmi.FEC(4, 4, device=0)
    S, stripes = 4112, 3
    host = np.random.default_rng(3).integers(0, 256, size=stripes * 4 * r16(S), dtype=np.uint8)
    buf = torch.from_numpy(host.copy()).cuda()
    table = torch.from_numpy(buf.data_ptr() + np.arange(stripes * 4, dtype=np.int64) * r16(S)).cuda()
    fb = torch.zeros(stripes, dtype=torch.int32, device="cuda:0")
    f.verify_ptrs(table.data_ptr(), S, stripes, fb.data_ptr())
    f.sync()
    assert fb.cpu().numpy().view(np.uint32).tolist() == [CLEAN] * 3
    st, cnt = f.correct_columns_ptrs(table.data_ptr(), S, stripes)
    assert st == [OK] * 3 and not cnt.any()
    assert np.array_equal(buf.cpu().numpy(), host)
    f.close()


# --------------------------------------------------- 9. kernel names ----
@pytest.mark.parametrize("code", sorted(CHECK_NAME))
def test_kernel_names(code):
    f = fec(code)
    assert f.kernel_name(10) == CHECK_NAME[code] + "_ptrs"
    assert f.kernel_name(11) == COLUMN_NAME[code] + "_ptrs"
    assert f.kernel_name(5) == CHECK_NAME[code]
    assert f.kernel_name(8) == COLUMN_NAME[code]


# ------------------------------------- 10. device set, 11. two threads ----
def scattered_run(code, S, stripes, seed, gone=None):
    run = Run(pool(code, S, stripes), gone, seed=seed)
    rng = np.random.default_rng(1000 * seed + S)
    for s in sorted({0, stripes - 1}):
        scatter(run, s, rng)
    return run


def test_device_set():
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert fs.kernel_name(10) == "check_K10_MG4_B256_ptrs" and fs.kernel_name(11) == "columns_MG4_B256_ptrs"
    single = scattered_run("rs10_14", 5000, 3, 1, {1: [4], 2: [0, 12]})
    check_corrected(fec("rs10_14"), single, "single")
    for seed, gone in ((1, {1: [4], 2: [0, 12]}), (2, None)):
        run = scattered_run("rs10_14", 5000, 3, seed, gone)
        run.flip(1, 7, 4096, 0x33)
        fb = run.verify(fs)
        assert fb[1] == 4096 and fb[0] != CLEAN
        check_corrected(fs, run, "device set")
        if seed == 1:  # the same bytes as through the single-device context
            assert np.array_equal(run.dev.cpu().numpy(), single.dev.cpu().numpy())
    fs.close()


def test_two_threads_one_context():
    f = fec("rs10_14")
    pools = [Pool(10, 14, 5000, 3, seed=70 + t) for t in range(2)]  # disjoint pools, built ahead of the threads
    errors = []

    def work(t):
        try:
            for rep in range(4):
                run = Run(pools[t], {1: [rep]} if rep % 2 else None, seed=rep)
                rng = np.random.default_rng(10 * t + rep)
                for s in range(3):
                    scatter(run, s, rng)
                st, cnt = run.correct(f)
                assert st == [OK] * 3
                assert np.array_equal(cnt, run.counts)
                run.check(f"thread {t} rep {rep}")
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors

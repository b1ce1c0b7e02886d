"""GPU: rs_correct_columns -- the column scrub of device-resident stripes
(verify, one per-column decode launch over the inconsistent stripes, verify of
those stripes again).

Every case works on a strided_image.Layout: shard pitch above
round_up(S, 16), gapped stripe strides, guard bands around every buffer, and
random bytes in padding, gaps and guards.  After every call the WHOLE device
image is compared with the expected one.  Expected bytes never come from the
engine: they are the pristine layout (payload seeded, parity from the oracle)
and, for columns beyond the radius, oracle.decode_correct on that one column
(share length 1) re-encoded with the oracle.
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
from strided_image import Layout, r16  # noqa: E402

CLEAN = rsmi.RS_VERIFY_CLEAN
OK, TOO_MANY = rsmi.RS_OK, rsmi.RS_ETOO_MANY_ERRORS
CODES = {"rs4_6": (4, 6), "rs10_14": (10, 14), "rs8_14": (8, 14), "rs3_19": (3, 19), "rs64_80": (64, 80),
         "rs240_256": (240, 256), "rs4_5": (4, 5), "rs12_40": (12, 40)}
VARIANT = {"rs4_6": "columns_MG4_B256", "rs10_14": "columns_MG4_B256", "rs8_14": "columns_MG8_B256",
           "rs3_19": "columns_MG16_B256", "rs64_80": "columns_MG16_B256", "rs240_256": "columns_MG16_B256",
           "rs4_5": "columns_MG4_B256"}
# one column | exactly one 4 KiB block chunk | a chunk plus one column | not a
# multiple of 16 | several chunks
SHAPES = [16, 4096, 4112, 5000, 3 * 4096 + 40]
SCATTER_CASES = ([(c, S, st) for c in ("rs4_6", "rs10_14", "rs8_14", "rs3_19") for S in SHAPES for st in (1, 3, 37)] +
                 [("rs64_80", S, st) for S in SHAPES for st in (1, 2)] +
                 [("rs240_256", S, st) for S in (16, 4112) for st in (1, 2)])

_LAYOUTS = {}
_FECS = {}
_MATRIX = {}


def layout(code, S, stripes):
    """Joined (one buffer of whole stripes) for three stripes, split otherwise."""
    key = (code, S, stripes)
    if key not in _LAYOUTS:
        k, n = CODES[code]
        _LAYOUTS[key] = Layout(k, n, S, stripes, seed=k * 1000003 + n * 10007 + S * 31 + stripes,
                               mode="joined" if stripes == 3 else "split")
    return _LAYOUTS[key]


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


class Run:
    """The host model of one call: `cur` is what the device buffers hold
    before it, `want` what they must hold afterwards (the pristine image
    unless a test says otherwise), `counts` the per-shard bytes the call must
    report as corrected."""

    def __init__(self, L):
        self.L = L
        self.cur = [b.copy() for b in L.pristine]
        self.want = [b.copy() for b in L.pristine]
        self.counts = np.zeros((L.stripes, L.n), dtype=np.int64)
        self.dev = None

    def flip(self, s, i, off, mask, counted=True):
        """XORs mask into byte off of shard i of stripe s (once per byte)."""
        b, o = self.L.shard_at(s, i)
        assert mask and self.cur[b][o + off] == self.L.pristine[b][o + off]
        self.cur[b][o + off] ^= mask
        if counted:
            self.counts[s, i] += 1

    def garbage_slot(self, s, i, seed):
        """An erased shard's slot: random bytes over its whole pitch, which
        must come back untouched."""
        b, o = self.L.shard_at(s, i)
        g = np.random.default_rng(seed).integers(0, 256, size=self.L.pitch, dtype=np.uint8)
        self.cur[b][o:o + self.L.pitch] = g
        self.want[b][o:o + self.L.pitch] = g

    def column(self, s, off, present=None):
        out = []
        for i in range(self.L.n) if present is None else present:
            b, o = self.L.shard_at(s, i)
            out.append((i, int(self.cur[b][o + off])))
        return out

    def pristine_column(self, s, off):
        return all(self.cur[b][o + off] == self.L.pristine[b][o + off]
                   for b, o in (self.L.shard_at(s, i) for i in range(self.L.n)))

    def keep_column(self, s, off, present=None):
        """The call must leave column off of stripe s as it is now."""
        for i in range(self.L.n) if present is None else present:
            b, o = self.L.shard_at(s, i)
            self.want[b][o + off] = self.cur[b][o + off]
            self.counts[s, i] -= int(self.cur[b][o + off] != self.L.pristine[b][o + off])

    def expect_column(self, s, off, word, present=None):
        """The call must turn column off of stripe s into `word` (n bytes)."""
        for i in range(self.L.n) if present is None else present:
            b, o = self.L.shard_at(s, i)
            self.counts[s, i] += int(word[i] != self.cur[b][o + off]) - int(self.cur[b][o + off] != self.L.pristine[b][o + off])
            self.want[b][o + off] = word[i]

    def upload(self):
        self.dev = [torch.from_numpy(b).cuda() for b in self.cur]
        return self.L.args([d.data_ptr() for d in self.dev])

    def call(self, f, erased=None):
        args = self.upload()
        st, cnt = f.correct_columns(*args, erased=None if erased is None else erased.tobytes())
        return st, np.array(cnt, dtype=np.int64).reshape(self.L.stripes, self.L.n)

    def check(self, what=""):
        for name, d, w in zip(self.L.names, self.dev, self.want):
            g = d.cpu().numpy()
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, f"{what} {name}: {bad.size} bytes differ, first offsets {bad[:8].tolist()}"

    def verify(self, f, erased=None):
        fb = torch.zeros(self.L.stripes, dtype=torch.int32, device="cuda:0")
        args = self.L.args([d.data_ptr() for d in self.dev])
        if erased is None:
            f.verify_stripes(*args, fb.data_ptr())
        else:
            f.verify_degraded(*args, erased.tobytes(), fb.data_ptr())
        f.sync()
        return fb.cpu().numpy().view(np.uint32)


def mask_of(rng):
    return int(rng.integers(1, 256))


def special_offsets(S):
    """Offset 0, the last byte (in the last, possibly partial, 16-byte
    column), both sides of the first 16-byte column's end and of the first
    4 KiB chunk's end."""
    return list(dict.fromkeys(o for o in (0, S - 1, 15, 16, 4095, 4096) if o < S))


def scatter(run, s, rng, present=None, radius=None):
    """Damage of stripe s that only a per-column decoder repairs: EVERY present
    shard is wrong somewhere (as far as S has columns for it: RS(240,256) at
    S = 16 has 16 columns of at most 8 errors), every column holds at most
    `radius` errors.  Column 0 holds one error, on the lowest present shard
    (shard 0 alone); the columns after it take the shards in order, `radius`
    to a column -- exactly at the radius, shard 0 together with others in the
    first of them and shard n - 1 in the last.  The special offsets come
    first; one left over gets a single error."""
    L = run.L
    present = list(range(L.n)) if present is None else present
    radius = L.m // 2 if radius is None else radius
    special = special_offsets(L.S)
    need = 1 + -(-len(present) // radius)
    rest = [int(o) for o in rng.permutation(L.S) if int(o) not in special]
    cols = (special + rest)[:max(need, len(special))]
    run.flip(s, present[0], cols[0], mask_of(rng))
    at = 0
    for off in cols[1:]:
        if at >= len(present):
            run.flip(s, present[int(rng.integers(len(present)))], off, mask_of(rng))
            continue
        for i in present[at:at + radius]:
            run.flip(s, i, off, mask_of(rng))
        at += radius


def sprinkle(run, s, rng, count):
    """`count` single errors in different columns of stripe s."""
    L = run.L
    for off in rng.choice(L.S, size=min(count, L.S), replace=False):
        run.flip(s, int(rng.integers(L.n)), int(off), mask_of(rng))


def scattered_run(code, S, stripes, seed=0):
    """Stripes 0 and stripes - 1 scattered; of the others every fifth gets a
    few single errors and the rest stay clean."""
    L = layout(code, S, stripes)
    run, rng = Run(L), np.random.default_rng(1000 * seed + S + stripes)
    for s in sorted({0, stripes - 1}):
        scatter(run, s, rng)
    for s in range(1, stripes - 1):
        if s % 5 == 2:
            sprinkle(run, s, rng, 1 + s % 3)
    return run


def check_scattered(f, run, what):
    L = run.L
    columns = f.stat(f.STAT_COLUMN_STRIPES)
    corrected = f.stat(f.STAT_COLUMN_BYTES)
    st, cnt = run.call(f)
    assert st == [OK] * L.stripes, what
    run.check(what)
    assert np.array_equal(cnt, run.counts), (what, np.argwhere(cnt != run.counts)[:8].tolist())
    dirty = int((run.counts.sum(axis=1) > 0).sum())
    assert f.stat(f.STAT_COLUMN_STRIPES) - columns == dirty
    assert f.stat(f.STAT_COLUMN_BYTES) - corrected == int(run.counts.sum())
    assert np.array_equal(run.verify(f), np.full(L.stripes, CLEAN, dtype=np.uint32))


# ---------------------------------------------------------------- clean ----
def test_clean_stripes_launch_nothing_new():
    L = layout("rs10_14", 4112, 37)
    f, run = fec("rs10_14"), Run(L)
    handed = f.stat(f.STAT_COLUMN_STRIPES)
    st, cnt = run.call(f)
    assert st == [OK] * 37 and not cnt.any()
    assert f.stat(f.STAT_COLUMN_STRIPES) == handed
    run.check("clean")


@pytest.mark.parametrize("code", sorted(VARIANT))
def test_variant_names(code):
    assert fec(code).kernel_name(8) == VARIANT[code]
    assert fec(code).kernel_name(8).startswith("columns_")


# ------------------------------------------------- scattered, in radius ----
@pytest.mark.parametrize("code,S,stripes", SCATTER_CASES)
def test_scattered_within_radius(code, S, stripes):
    run = scattered_run(code, S, stripes)
    L = run.L
    # the damage is what the case says: every shard of stripe 0 wrong wherever S has the columns for it
    if 1 + -(-L.n // (L.m // 2)) <= S:
        assert (run.counts[0] > 0).all()
    check_scattered(fec(code), run, f"{code} S={S} x{stripes}")


def test_scattered_three_sectors_rs10_14():
    """The issue's example: three bad 4 KiB sectors on three devices at three
    offsets of an RS(10,4) stripe -- one error per column."""
    L = layout("rs10_14", 3 * 4096 + 40, 3)
    run, rng = Run(L), np.random.default_rng(5)
    for shard, start in ((0, 0), (7, 4096), (13, 8192)):
        for off in range(start, start + 4096):
            run.flip(1, shard, off, mask_of(rng))
    check_scattered(fec("rs10_14"), run, "three sectors")
    assert run.counts[1].tolist() == [4096] + [0] * 6 + [4096] + [0] * 5 + [4096]


@pytest.mark.parametrize("code,S,stripes", [("rs10_14", 5000, 3), ("rs64_80", 4112, 2), ("rs3_19", 4096, 1)])
def test_whole_shard_garbage(code, S, stripes):
    """floor(m / 2) shards of a stripe wrong at every byte: what
    rs_correct_stripes repairs, this call repairs too."""
    L = layout(code, S, stripes)
    run, rng = Run(L), np.random.default_rng(S)
    s = stripes - 1
    shards = sorted({0, L.n - 1} | set(int(x) for x in rng.choice(L.n, size=L.m // 2, replace=False)))[:L.m // 2]
    for i in shards:
        for off, mk in enumerate(rng.integers(1, 256, size=S)):
            run.flip(s, i, off, int(mk))
    check_scattered(fec(code), run, f"garbage {code}")
    assert run.counts[s, shards].tolist() == [S] * len(shards)


# -------------------------------------------------------- beyond radius ----
def find_columns(L, s, seed, weight, want_fail, count, taken):
    """`count` columns (offset, {shard: mask}) of `weight` errors on stripe s
    of the pristine layout on which the oracle fails (want_fail) or lands on
    another codeword, at offsets not in `taken`."""
    rng = np.random.default_rng(seed)
    found = []
    for _ in range(40000):
        if len(found) == count:
            break
        off = int(rng.integers(L.S))
        if off in taken:
            continue
        shards = [int(x) for x in rng.choice(L.n, size=weight, replace=False)]
        masks = {i: mask_of(rng) for i in shards}
        col = [(i, int(L.shard(s, i)[off]) ^ masks.get(i, 0)) for i in range(L.n)]
        rc, _ = oracle_column(L.k, L.n, col)
        if (rc != 0) == want_fail:
            found.append((off, masks))
            taken.add(off)
    assert len(found) == count, (len(found), count)
    return found


@pytest.mark.parametrize("code", ["rs10_14", "rs4_6"])
def test_beyond_radius(code):
    """Stripe 1: hopeless columns (floor(m / 2) + 1 errors, seeded so that the
    oracle FAILS on them) among correctable ones -- RS_ETOO_MANY_ERRORS, the
    correctable columns restored, the hopeless ones byte-identical, and the
    lowest of them is what rs_verify_stripes reports afterwards.  Stripe 2:
    columns of floor(m / 2) + 1 errors on which the oracle lands on ANOTHER
    codeword -- the engine writes the oracle's bytes, and the stripe is
    consistent (RS_OK).  Stripe 0: correctable damage only."""
    L = layout(code, 5000, 3)
    f, run, rng = fec(code), Run(L), np.random.default_rng(77)
    weight = L.m // 2 + 1
    taken = set()
    hopeless = find_columns(L, 1, 11, weight, True, 2, taken)
    elsewhere = find_columns(L, 2, 12, weight, False, 2, taken)
    for s, cols in ((1, hopeless), (2, elsewhere)):
        for off, masks in cols:
            for i, mk in masks.items():
                run.flip(s, i, off, mk)
    # correctable columns around them, in all three stripes, next to the hopeless ones too
    for s in range(3):
        for off in rng.choice(L.S, size=12, replace=False):
            if int(off) not in taken:
                run.flip(s, int(rng.integers(L.n)), int(off), mask_of(rng))
    off0 = hopeless[0][0]
    for near in (off0 - 1, off0 + 1):
        if 0 <= near < L.S and run.pristine_column(1, near):
            run.flip(1, 0, near, 0x5A)
    for off, _ in hopeless:
        rc, _ = oracle_column(L.k, L.n, run.column(1, off))
        assert rc != 0  # the oracle fails: nothing to write
        run.keep_column(1, off)
    for off, _ in elsewhere:
        rc, word = oracle_column(L.k, L.n, run.column(2, off))
        assert rc == 0 and any(word[i] != int(L.shard(2, i)[off]) for i in range(L.n))  # another codeword
        run.expect_column(2, off, word)
    st, cnt = run.call(f)
    assert st == [OK, TOO_MANY, OK]
    run.check(f"beyond radius {code}")
    assert np.array_equal(cnt, run.counts), np.argwhere(cnt != run.counts)[:8].tolist()
    want_fb = np.full(3, CLEAN, dtype=np.uint32)
    want_fb[1] = min(off for off, _ in hopeless)
    assert np.array_equal(run.verify(f), want_fb)
    # the return value, through the C ABI
    args = run.upload()
    rc = rsmi.load().rs_correct_columns(f._h, *args, None, None, None, None)
    assert rc == TOO_MANY
    run.check(f"beyond radius {code}, NULL status and corrected")


# --------------------------------------------- radius 0, nothing to check ----
def test_radius_zero_reports_too_many_errors_unwritten():
    """RS(4,5), m = 1: an error can be seen but not located."""
    L = layout("rs4_5", 4112, 3)
    f, run = fec("rs4_5"), Run(L)
    run.flip(1, 2, 100, 0x40, counted=False)
    run.want = [b.copy() for b in run.cur]
    handed = f.stat(f.STAT_COLUMN_STRIPES)
    st, cnt = run.call(f)
    assert st == [OK, TOO_MANY, OK] and not cnt.any()
    assert f.stat(f.STAT_COLUMN_STRIPES) == handed
    run.check("RS(4,5)")
    st3 = (ctypes.c_int * 3)()
    assert rsmi.load().rs_correct_columns(f._h, *run.upload(), None, st3, None, None) == TOO_MANY
    assert list(st3) == [OK, TOO_MANY, OK]
    run.check("RS(4,5) again")


def test_no_parity_is_ok():
    """k == n: every stripe is a codeword."""
    f = rsmi.FEC(6, 6, device=0)
    S, stripes = 4112, 3
    pitch = r16(S) + 32
    host = np.random.default_rng(3).integers(0, 256, size=stripes * 6 * pitch, dtype=np.uint8)
    buf = torch.from_numpy(host.copy()).cuda()
    st, cnt = f.correct_columns(buf.data_ptr(), 6 * pitch, buf.data_ptr(), 0, pitch, S, stripes)
    assert st == [OK] * 3 and not any(cnt)
    assert np.array_equal(buf.cpu().numpy(), host)
    assert f.kernel_name(8) == "none"
    f.close()


# ------------------------------------------------------------- degraded ----
def erased_flags(L, gone):
    er = np.zeros((L.stripes, L.n), dtype=np.uint8)
    for s, shards in gone.items():
        er[s, shards] = 1
    return er


def degraded_run(code, S, stripes, gone, garbage_seed):
    """Errors exactly at the degraded radius in every column that has any, on
    stripes with missing shards (gone = {stripe: shards}); stripes without
    erasures are scattered at the full radius."""
    L = layout(code, S, stripes)
    run, rng = Run(L), np.random.default_rng(S + stripes)
    for s in range(stripes):
        lost = gone.get(s, [])
        present = [i for i in range(L.n) if i not in lost]
        scatter(run, s, rng, present, (L.m - len(lost)) // 2)
        for i in lost:
            run.garbage_slot(s, i, garbage_seed * 1000 + s * 256 + i)
    return run, erased_flags(L, gone)


@pytest.mark.parametrize("code,S,stripes,gone", [
    ("rs10_14", 5000, 3, {0: [0], 1: [3, 13]}),            # e = 1 and e = 2: radius 1; stripe 2 whole: radius 2
    ("rs10_14", 4112, 37, {0: [13], 5: [0, 12], 36: [9]}),
    ("rs64_80", 4112, 2, {0: [0, 31, 64, 79]}),            # e = 4: radius 6
    ("rs240_256", 4112, 1, {0: [0, 255]}),                 # r = 254, radius 7
])
def test_degraded(code, S, stripes, gone):
    f = fec(code)
    images = []
    for garbage_seed in (1, 2):
        run, er = degraded_run(code, S, stripes, gone, garbage_seed)
        checked = f.stat(f.STAT_CHECK_STRIPES)
        st, cnt = run.call(f, er)
        assert st == [OK] * stripes
        run.check(f"degraded {code} garbage {garbage_seed}")  # the slots keep their garbage
        assert np.array_equal(cnt, run.counts), np.argwhere(cnt != run.counts)[:8].tolist()
        assert not cnt[er != 0].any()
        assert f.stat(f.STAT_CHECK_STRIPES) > checked  # the degraded verify served the missing shards
        assert np.array_equal(run.verify(f, er), np.full(stripes, CLEAN, dtype=np.uint32))
        images.append([d.cpu().numpy() for d in run.dev])
    # the same image whatever the slots hold, but for the slots themselves
    L = run.L
    for s, shards in gone.items():
        for i in shards:
            buf, o = L.shard_at(s, i)
            assert not np.array_equal(images[0][buf][o:o + L.pitch], images[1][buf][o:o + L.pitch])
            for img in images:
                img[buf][o:o + L.pitch] = 0
    for a, b in zip(*images):
        assert np.array_equal(a, b)


def test_degraded_saturated_and_too_many():
    """e == m: no redundancy left, RS_OK with nothing touched, whatever the
    stripe holds.  e == m + 1: RS_ENOT_ENOUGH and nothing written, also when
    other stripes could be repaired."""
    L = layout("rs10_14", 5000, 3)
    f, run, rng = fec("rs10_14"), Run(L), np.random.default_rng(8)
    gone = {1: [0, 5, 10, 13]}
    for i in gone[1]:
        run.garbage_slot(1, i, 50 + i)
    run.flip(1, 2, 77, 0x11, counted=False)  # indistinguishable from data
    run.want = [b.copy() for b in run.cur]
    st, cnt = run.call(f, erased_flags(L, gone))
    assert st == [OK] * 3 and not cnt.any()
    run.check("e == m")
    sprinkle(run, 0, rng, 3)  # repairable, but the call must refuse as a whole
    run.want = [b.copy() for b in run.cur]
    er = erased_flags(L, {1: [0, 5, 10, 13, 7]})
    args = run.upload()
    st3 = (ctypes.c_int * 3)(9, 9, 9)
    buf = ctypes.c_char_p(er.tobytes())
    rc = rsmi.load().rs_correct_columns(f._h, *args, ctypes.cast(buf, ctypes.c_void_p), st3, None, None)
    assert rc == rsmi.RS_ENOT_ENOUGH
    f.sync()
    run.check("e == m + 1")
    with pytest.raises(rsmi.NotEnoughShares):
        f.correct_columns(*args, erased=er.tobytes())


def test_degraded_radius_zero_and_beyond():
    """RS(10,14) with three shards missing has r - k = 1: an inconsistent
    stripe ends RS_ETOO_MANY_ERRORS unwritten.  With two missing, two errors in
    a column are past the radius of 1: the oracle decides what happens."""
    L = layout("rs10_14", 5000, 3)
    f, run = fec("rs10_14"), Run(L)
    gone = {0: [1, 2, 11], 2: [0, 13]}
    er = erased_flags(L, gone)
    for s, shards in gone.items():
        for i in shards:
            run.garbage_slot(s, i, 7 * s + i)
    run.flip(0, 5, 4999, 0x01)
    run.keep_column(0, 4999, [i for i in range(L.n) if i not in gone[0]])
    run.flip(1, 0, 0, 0x80)  # no erasures: repaired
    present = [i for i in range(L.n) if i not in gone[2]]
    run.flip(2, 4, 16, 0x21)
    run.flip(2, 12, 16, 0x07)
    run.flip(2, 1, 4096, 0xFF)  # within the radius, same stripe
    rc, word = oracle_column(L.k, L.n, run.column(2, 16, present))
    if rc != 0:
        run.keep_column(2, 16, present)
    else:
        run.expect_column(2, 16, word, present)
    st, cnt = run.call(f, er)
    assert st == [TOO_MANY, OK, TOO_MANY if rc != 0 else OK]
    run.check("degraded, radius 0 and beyond")
    assert np.array_equal(cnt, run.counts), np.argwhere(cnt != run.counts)[:8].tolist()
    want_fb = np.array([4999, CLEAN, 16 if rc != 0 else CLEAN], dtype=np.uint32)
    assert np.array_equal(run.verify(f, er), want_fb)


def test_zero_flags_behave_as_null():
    run = scattered_run("rs10_14", 5000, 3, seed=3)
    f = fec("rs10_14")
    checked = f.stat(f.STAT_CHECK_STRIPES)
    st, cnt = run.call(f, np.zeros((3, 14), dtype=np.uint8))
    assert st == [OK] * 3 and np.array_equal(cnt, run.counts)
    run.check("zero flags")
    assert f.stat(f.STAT_CHECK_STRIPES) == checked  # the plain verify, not the degraded one


# -------------------------------------------------------------- padding ----
@pytest.mark.parametrize("code,S", [("rs10_14", 5000), ("rs10_14", 16), ("rs64_80", 4112 - 7)])
def test_padding_and_gaps_are_not_errors(code, S):
    """Flips inside [S, round_up(S, 16)), in the pitch gap behind it, in the
    stride gaps and in the guards: RS_OK, nothing changed, nothing counted."""
    L = layout(code, S, 2)
    f, run = fec(code), Run(L)
    for s in range(2):
        for i in (0, L.k - 1, L.k, L.n - 1):
            b, o = L.shard_at(s, i)
            for off in list(range(S, r16(S))) + [r16(S), L.pitch - 1]:
                run.cur[b][o + off] ^= 0xA5
    for b in range(len(run.cur)):
        run.cur[b][0] ^= 1
        run.cur[b][-1] ^= 1
    b, o = L.shard_at(0, L.k - 1)
    run.cur[b][o + L.pitch + 3] ^= 0x33  # the stride gap behind stripe 0's data (split) or its parity's predecessor
    run.want = [x.copy() for x in run.cur]
    handed = f.stat(f.STAT_COLUMN_STRIPES)
    st, cnt = run.call(f)
    assert st == [OK] * 2 and not cnt.any()
    assert f.stat(f.STAT_COLUMN_STRIPES) == handed
    run.check("padding")
    # and a real error next to the padding is still repaired, the padding left alone
    run.flip(1, L.n - 1, S - 1, 0x80)
    st, cnt = run.call(f)
    assert st == [OK] * 2 and int(cnt.sum()) == 1 and cnt[1, L.n - 1] == 1
    run.check("padding, one error")


# ------------------------------------------------------------ arguments ----
def test_rejects_bad_arguments():
    L = layout("rs10_14", 4112, 3)
    f, run = fec("rs10_14"), Run(L)
    sprinkle(run, 1, np.random.default_rng(2), 2)
    dp, dss, pp, pss, pitch, S, stripes = run.upload()
    run.want = [b.copy() for b in run.cur]
    lib = rsmi.load()
    st = (ctypes.c_int * 3)()
    call = lambda *a: lib.rs_correct_columns(f._h, *a, None, st, None, None)  # noqa: E731
    assert call(dp, dss, pp, pss, pitch + 8, S, stripes) == rsmi.RS_EINVAL
    assert call(dp, dss, pp, pss, r16(S) - 16, S, stripes) == rsmi.RS_EINVAL
    assert call(dp + 8, dss, pp, pss, pitch, S, stripes) == rsmi.RS_EINVAL
    assert call(dp, dss, pp + 4, pss, pitch, S, stripes) == rsmi.RS_EINVAL
    assert call(dp, dss + 8, pp, pss, pitch, S, stripes) == rsmi.RS_EINVAL
    assert call(None, dss, pp, pss, pitch, S, stripes) == rsmi.RS_EINVAL
    assert call(dp, dss, pp, pss, pitch, S, 0) == rsmi.RS_OK
    assert call(dp, dss, pp, pss, pitch, 0, stripes) == rsmi.RS_OK
    assert lib.rs_correct_columns(None, dp, dss, pp, pss, pitch, S, stripes, None, st, None, None) == rsmi.RS_EINVAL
    f.sync()
    run.check("refused calls")
    # m = 28 > 16: not served
    wide = fec("rs12_40")
    assert wide.kernel_name(8) == "none"
    assert lib.rs_correct_columns(wide._h, dp, dss, pp, pss, pitch, S, 1, None, st, None, None) == rsmi.RS_EINVAL
    run.check("m > 16")
    # NULL status and NULL corrected
    run.want = [b.copy() for b in L.pristine]
    assert lib.rs_correct_columns(f._h, dp, dss, pp, pss, pitch, S, stripes, None, None, None, None) == rsmi.RS_OK
    run.check("NULL outputs")


# ----------------------------------------------- device set, two threads ----
def test_device_set():
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert fs.kernel_name(8) == "columns_MG4_B256"
    check_scattered(fs, scattered_run("rs10_14", 5000, 3, seed=1), "device set")
    check_scattered(fs, scattered_run("rs10_14", 4112, 37, seed=1), "device set x37")
    fs.close()


def test_two_threads_one_context():
    f = fec("rs10_14")
    layout("rs10_14", 5000, 3)  # built once, ahead of the threads
    errors = []

    def work(t):
        try:
            for rep in range(4):
                run = scattered_run("rs10_14", 5000, 3, seed=10 * t + rep + 20)
                st, cnt = run.call(f)
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

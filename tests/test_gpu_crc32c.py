"""GPU: the sector checksums -- rs_crc32c_stripes / _check_stripes, their
pointer twins and rs_correct_crc32c.

The model of every checksum is rs_crc32c_host on the sector's bytes, itself
pinned to RFC 3720 and a bitwise model by test_crc32c_host.py.  Images have a
pitch and strides with gaps and guard bands, all random bytes; after every call
the whole image, the whole checksum table (gaps and guard words included) and
first_bad are compared with what the call is documented to leave there.
Codewords come from the oracle, never from the engine.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from oracle import oracle  # noqa: E402

CLEAN = rsmi.RS_VERIFY_CLEAN
OK, TOO_MANY, EINVAL, NOT_ENOUGH = rsmi.RS_OK, rsmi.RS_ETOO_MANY_ERRORS, rsmi.RS_EINVAL, rsmi.RS_ENOT_ENOUGH
GUARD = 256          # bytes around each buffer
CG = 8               # guard words around the checksum table
PATTERN = 0xA5C35A3C  # what untouched checksum entries hold
CODES = [(10, 14), (64, 80), (3, 5)]
# below one 16-byte word | a word and its neighbours | around a 512-byte sector | around a 4 KiB sector (the
# lane-group width changes at 4 KiB) | several sectors and a ragged tail
LENGTHS = [1, 15, 16, 17, 511, 512, 513, 4095, 4096, 4097, 3 * 4096 + 5]
SECTORS = [512, 4096, 65536]
# The kernel serves a sector with 8, 16, 32 or 64 lanes (512 B, 1 KiB, 2 KiB, 4 KiB and up), each width with a
# stride table of its own, and from 8 KiB on a lane's loop and a block's run of sectors grow with the sector:
# every sector size the three above leave out, at lengths around one and several sectors of each and one past
# the 64 KiB (or four sectors) of a block, so that a shard takes more than one block; 512 again for that length.
OTHER_SECTORS = [512, 1024, 2048, 8192, 16384, 32768]
S_REPAIR = 3 * 4096 + 5

_FECS = {}


def fec(k, n):
    if (k, n) not in _FECS:
        _FECS[(k, n)] = rsmi.FEC(k, n, device=0)
    return _FECS[(k, n)]


def r16(x):
    return (x + 15) // 16 * 16


def dev(a):
    """The array on the device; unsigned words travel as signed ones of the
    same width (read them back with unsigned())."""
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint32, np.uint64):
        a = a.view(np.int32 if a.dtype == np.uint32 else np.int64)
    return torch.from_numpy(a).cuda()


def unsigned(t):
    h = t.cpu().numpy()
    return h.view(np.uint32 if h.dtype == np.int32 else np.uint64)


class Img:
    """Stripes in two buffers (data, parity) with a pitch gap of 32 bytes,
    stride gaps of 48 and 16 and guard bands, every byte random; coded=True
    makes every stripe a codeword (parity from the oracle)."""

    def __init__(self, k, n, S, stripes, seed=0, coded=False):
        self.k, self.n, self.m, self.S, self.stripes = k, n, n - k, S, stripes
        self.pitch = r16(S) + 32
        self.dss, self.pss = k * self.pitch + 48, self.m * self.pitch + 16
        self.rng = np.random.default_rng(seed + 1000 * k + n + 7 * S)
        self.h = [self.rng.integers(0, 256, size=2 * GUARD + stripes * ss, dtype=np.uint8) for ss in (self.dss, self.pss)]
        if coded:
            E = oracle.fec_matrix(k, n)
            for s in range(stripes):
                data = self.rng.integers(0, 256, size=k * S, dtype=np.uint8)
                par = np.frombuffer(oracle.encode(E, k, n, data.tobytes()), dtype=np.uint8)
                for i in range(n):
                    self.shard(s, i)[:] = data[i * S:(i + 1) * S] if i < k else par[(i - k) * S:(i - k + 1) * S]
        self.d = None

    def at(self, s, i):
        """(buffer, offset in it) of shard i of stripe s."""
        if i < self.k:
            return 0, GUARD + s * self.dss + i * self.pitch
        return 1, GUARD + s * self.pss + (i - self.k) * self.pitch

    def shard(self, s, i, length=None):
        b, o = self.at(s, i)
        return self.h[b][o:o + (self.S if length is None else length)]

    def refill_gaps(self):
        """Other random bytes everywhere but in the shards' [0, S)."""
        keep = [[(self.at(s, i), self.shard(s, i).copy()) for i in range(self.n)] for s in range(self.stripes)]
        for a in self.h:
            a[:] = self.rng.integers(0, 256, size=len(a), dtype=np.uint8)
        for row in keep:
            for (b, o), bytes_ in row:
                self.h[b][o:o + self.S] = bytes_

    def upload(self):
        self.d = [dev(a) for a in self.h]
        return self

    def args(self, skip=0, length=None):
        return (self.d[0].data_ptr() + GUARD + skip, self.dss, self.d[1].data_ptr() + GUARD + skip, self.pss, self.pitch,
                self.S - skip if length is None else length, self.stripes)

    def flip(self, s, i, off, xor=0x10):
        """A wrong byte on the device (and only there)."""
        b, o = self.at(s, i)
        self.d[b][o + off] ^= xor

    def unchanged(self):
        return all(np.array_equal(d.cpu().numpy(), h) for d, h in zip(self.d, self.h))

    def model(self, sector, skip=0):
        """[stripes * n][nsec] checksums of the host image's shards."""
        S = self.S - skip
        nsec = (S + sector - 1) // sector
        bufs = [self.shard(s, i)[skip + j * sector:skip + min((j + 1) * sector, S)].tobytes()
                for s in range(self.stripes) for i in range(self.n) for j in range(nsec)]
        return np.array(rsmi.crc32c_host(bufs), dtype=np.uint32).reshape(self.stripes * self.n, nsec)


class Table:
    """The checksum table on the device: guard words, then [shards][crc_pitch]
    with crc_pitch = nsec + 3, every word PATTERN; or, with `model`, the
    model's checksums in the entries."""

    def __init__(self, shards, nsec, model=None):
        self.shards, self.nsec, self.cp = shards, nsec, nsec + 3
        h = np.full(2 * CG + shards * self.cp, PATTERN, dtype=np.uint32)
        if model is not None:
            h[CG:CG + shards * self.cp].reshape(shards, self.cp)[:, :nsec] = model
        self.h = h
        self.d = dev(h)

    @property
    def ptr(self):
        return self.d.data_ptr() + 4 * CG

    def host(self):
        return unsigned(self.d)

    def entries(self):
        return self.host()[CG:CG + self.shards * self.cp].reshape(self.shards, self.cp)

    def want(self, model, skip_rows=()):
        """The whole table after a compute: the model in the entries of the
        rows that are not skipped, PATTERN everywhere else."""
        w = np.full_like(self.h, PATTERN)
        rows = w[CG:CG + self.shards * self.cp].reshape(self.shards, self.cp)
        for x in range(self.shards):
            if x not in skip_rows:
                rows[x, :self.nsec] = model[x]
        return w


def first_bad_buf(shards):
    return dev(np.full(shards + 2, 0x12345678, dtype=np.uint32))


def verdicts(fb, shards):
    h = unsigned(fb)
    assert h[shards] == 0x12345678 and h[shards + 1] == 0x12345678, "first_bad written past stripes * n"
    return h[:shards]


def flags(stripes, n, gone):
    er = np.zeros((stripes, n), dtype=np.uint8)
    for s, i in gone:
        er[s, i] = 1
    return er.tobytes()


# ---------------------------------------------------------------- compute ----
@pytest.mark.parametrize("sector", SECTORS)
@pytest.mark.parametrize("k,n", CODES)
def test_compute_and_clean_check(k, n, sector):
    f = fec(k, n)
    stripes = 3
    for S in LENGTHS:
        img = Img(k, n, S, stripes, seed=sector).upload()
        nsec = (S + sector - 1) // sector
        model = img.model(sector)
        tab = Table(stripes * n, nsec)
        f.crc32c_stripes(*img.args(), sector, tab.ptr, tab.cp)
        f.sync()
        assert np.array_equal(tab.host(), tab.want(model)), (S, "checksums, gaps or guards")
        assert img.unchanged(), (S, "the image was written")
        # the bytes between shard_len and the pitch, and every gap, are no part of a checksum
        img.refill_gaps()
        img.upload()
        tab2 = Table(stripes * n, nsec)
        f.crc32c_stripes(*img.args(), sector, tab2.ptr, tab2.cp)
        fb = first_bad_buf(stripes * n)
        f.crc32c_check_stripes(*img.args(), sector, tab.ptr, tab.cp, fb.data_ptr())
        f.sync()
        assert np.array_equal(tab2.host(), tab.want(model)), (S, "padding entered a checksum")
        assert (verdicts(fb, stripes * n) == CLEAN).all(), S
        assert img.unchanged() and np.array_equal(tab.host(), tab.want(model)), (S, "the check wrote something")


@pytest.mark.parametrize("sector", OTHER_SECTORS)
def test_compute_and_check_other_sector_sizes(sector):
    k, n, stripes = 3, 5, 2
    f = fec(k, n)
    for S in (1, sector - 1, sector, sector + 1, 2 * sector + 17, 5 * sector + 1000, 65536 + sector + 5):
        img = Img(k, n, S, stripes, seed=sector).upload()
        nsec = (S + sector - 1) // sector
        model = img.model(sector)
        tab = Table(stripes * n, nsec)
        f.crc32c_stripes(*img.args(), sector, tab.ptr, tab.cp)
        fb = first_bad_buf(stripes * n)
        f.crc32c_check_stripes(*img.args(), sector, tab.ptr, tab.cp, fb.data_ptr())
        f.sync()
        assert np.array_equal(tab.host(), tab.want(model)), (S, "checksums, gaps or guards")
        assert (verdicts(fb, stripes * n) == CLEAN).all(), S
        # the last byte of the shard and the first of its last sector, in different shards
        img.flip(1, 0, S - 1, 0x80)
        img.flip(0, n - 1, (nsec - 1) * sector, 0x01)
        fb = first_bad_buf(stripes * n)
        f.crc32c_check_stripes(*img.args(), sector, tab.ptr, tab.cp, fb.data_ptr())
        f.sync()
        want = np.full(stripes * n, CLEAN, dtype=np.uint32)
        want[n] = want[n - 1] = nsec - 1
        assert np.array_equal(verdicts(fb, stripes * n), want), S


@pytest.mark.parametrize("k,n", [(10, 14), (3, 5)])
def test_erased_shards_are_left_alone(k, n):
    f = fec(k, n)
    stripes, S, sector = 3, 4097, 512
    gone = [(0, 1), (0, n - 1), (2, 0), (2, 1), (2, k)]
    img = Img(k, n, S, stripes, seed=5).upload()
    nsec = (S + sector - 1) // sector
    model = img.model(sector)
    tab = Table(stripes * n, nsec)
    er = flags(stripes, n, gone)
    f.crc32c_stripes(*img.args(), sector, tab.ptr, tab.cp, erased=er)
    f.sync()
    skip = {s * n + i for s, i in gone}
    assert np.array_equal(tab.host(), tab.want(model, skip))
    # the check: erased shards are clean whatever their entries hold, a wrong byte in one is not looked at
    img.flip(2, 1, 100)
    img.flip(1, 2, 600)
    fb = first_bad_buf(stripes * n)
    f.crc32c_check_stripes(*img.args(), sector, tab.ptr, tab.cp, fb.data_ptr(), erased=er)
    f.sync()
    want = np.full(stripes * n, CLEAN, dtype=np.uint32)
    want[1 * n + 2] = 1
    assert np.array_equal(verdicts(fb, stripes * n), want)
    # every shard of every stripe missing: nothing to do
    fb = first_bad_buf(stripes * n)
    f.crc32c_check_stripes(*img.args(), sector, tab.ptr, tab.cp, fb.data_ptr(), erased=b"\1" * (stripes * n))
    f.sync()
    assert (verdicts(fb, stripes * n) == CLEAN).all()


# ------------------------------------------------------------------ check ----
@pytest.fixture(scope="module")
def checked():
    """RS(10,4), 3 stripes of 3 * 4096 + 5 bytes, 4 KiB sectors, the model's
    checksums stored."""
    k, n, S, sector = 10, 14, S_REPAIR, 4096
    img = Img(k, n, S, 3, seed=77).upload()
    tab = Table(3 * n, 4, img.model(sector))
    return fec(k, n), img, tab, sector


def run_check(f, img, tab, sector, **kw):
    shards = img.stripes * img.n
    fb = first_bad_buf(shards)
    f.crc32c_check_stripes(*img.args(), sector, tab.ptr, tab.cp, fb.data_ptr(), **kw)
    f.sync()
    return verdicts(fb, shards)


@pytest.mark.parametrize("shard", [2, 11])
@pytest.mark.parametrize("where", ["first", "last", "end_of_sector_0", "start_of_sector_1"])
def test_single_bit_flips(checked, shard, where):
    f, img, tab, sector = checked
    off, sec = {"first": (0, 0), "last": (img.S - 1, 3), "end_of_sector_0": (sector - 1, 0),
                "start_of_sector_1": (sector, 1)}[where]
    img.flip(1, shard, off, 1 << (off % 8))
    try:
        got = run_check(f, img, tab, sector)
    finally:
        img.flip(1, shard, off, 1 << (off % 8))
    want = np.full(3 * img.n, CLEAN, dtype=np.uint32)
    want[1 * img.n + shard] = sec
    assert np.array_equal(got, want)
    assert img.unchanged()


def test_check_further_cases(checked):
    f, img, tab, sector = checked
    n = img.n
    clean = np.full(3 * n, CLEAN, dtype=np.uint32)
    # two bad sectors in one shard: the lower
    img.flip(0, 3, 2 * sector + 9)
    img.flip(0, 3, sector + 4000)
    want = clean.copy()
    want[3] = 1
    assert np.array_equal(run_check(f, img, tab, sector), want)
    img.flip(0, 3, 2 * sector + 9)
    img.flip(0, 3, sector + 4000)
    # padding is no part of a checksum
    for s, i in ((0, 0), (2, 13)):
        img.flip(s, i, img.S)
        img.flip(s, i, r16(img.S) - 1)
    assert np.array_equal(run_check(f, img, tab, sector), clean)
    for s, i in ((0, 0), (2, 13)):
        img.flip(s, i, img.S)
        img.flip(s, i, r16(img.S) - 1)
    assert img.unchanged()
    # a flipped stored checksum
    x = 2 * n + 12
    tab.d[CG + x * tab.cp + 2] ^= 0x400
    want = clean.copy()
    want[x] = 2
    assert np.array_equal(run_check(f, img, tab, sector), want)
    tab.d[CG + x * tab.cp + 2] ^= 0x400
    assert np.array_equal(run_check(f, img, tab, sector), clean)


def test_slice_call_over_the_full_table(checked):
    """data / parity advanced by 2 sectors, crcs by 2 entries: the store's full
    table serves the slice, and the verdicts are slice-relative."""
    f, img, tab, sector = checked
    n, shards = img.n, 3 * img.n
    img.flip(1, 6, 3 * sector + 2)  # sector 3 = sector 1 of the slice
    img.flip(1, 7, sector + 2)      # in front of the slice: not looked at
    fb = first_bad_buf(shards)
    f.crc32c_check_stripes(*img.args(skip=2 * sector), sector, tab.ptr + 8, tab.cp, fb.data_ptr())
    f.sync()
    img.flip(1, 6, 3 * sector + 2)
    img.flip(1, 7, sector + 2)
    want = np.full(shards, CLEAN, dtype=np.uint32)
    want[n + 6] = 1
    assert np.array_equal(verdicts(fb, shards), want)
    # and the compute of the slice writes entries 2 and 3 of every row and nothing else
    fresh = Table(shards, 4)
    f.crc32c_stripes(*img.args(skip=2 * sector), sector, fresh.ptr + 8, fresh.cp)
    f.sync()
    model = img.model(sector)
    rows = fresh.entries()
    assert np.array_equal(rows[:, 2:4], model[:, 2:4])
    assert (rows[:, :2] == PATTERN).all() and (rows[:, 4:] == PATTERN).all()


# ---------------------------------------------------------- pointer twins ----
@pytest.mark.parametrize("k,n,S,sector", [(10, 14, 3 * 4096 + 5, 4096), (64, 80, 513, 512), (3, 5, 4097, 65536)])
def test_pointer_twins_agree_with_the_strided_calls(k, n, S, sector):
    f = fec(k, n)
    stripes = 3
    img = Img(k, n, S, stripes, seed=11).upload()
    shards, nsec = stripes * n, (S + sector - 1) // sector
    gone = [(0, 1), (2, n - 1)]
    er = flags(stripes, n, gone)
    # the same shards at shuffled rows of one pool; rows no entry of a present shard names hold other bytes
    rng = np.random.default_rng(S)
    row = r16(S) + 48
    order = rng.permutation(shards + 4)
    pool_h = rng.integers(0, 256, size=GUARD + (shards + 4) * row + GUARD, dtype=np.uint8)
    decoy = GUARD + int(order[shards]) * row  # where the entries of erased shards point: valid memory
    addr = np.zeros(shards, dtype=np.uint64)
    for s in range(stripes):
        for i in range(n):
            x = s * n + i
            o = GUARD + int(order[x]) * row
            if (s, i) in gone:
                o = decoy
            else:
                pool_h[o:o + S] = img.shard(s, i)
            addr[x] = o
    pool = dev(pool_h)
    table = dev(addr + np.uint64(pool.data_ptr()))
    t_str, t_ptr = Table(shards, nsec), Table(shards, nsec)
    f.crc32c_stripes(*img.args(), sector, t_str.ptr, t_str.cp, erased=er)
    f.crc32c_ptrs(table.data_ptr(), S, stripes, sector, t_ptr.ptr, t_ptr.cp, erased=er)
    f.sync()
    model = img.model(sector)
    assert np.array_equal(t_str.host(), t_str.want(model, {s * n + i for s, i in gone}))
    assert np.array_equal(t_ptr.host(), t_str.host()), "the decoy's checksums were produced, or an entry differs"
    # damage at the same places of both placements
    hits = [(0, 0, 0), (1, k, S - 1), (2, 2, min(S - 1, sector))]
    for s, i, off in hits:
        img.flip(s, i, off)
        pool[int(addr[s * n + i]) + off] ^= 0x10
    pool[decoy + 3] ^= 0xFF  # the decoy is not looked at
    fb_s, fb_p = first_bad_buf(shards), first_bad_buf(shards)
    f.crc32c_check_stripes(*img.args(), sector, t_str.ptr, t_str.cp, fb_s.data_ptr(), erased=er)
    f.crc32c_check_ptrs(table.data_ptr(), S, stripes, sector, t_ptr.ptr, t_ptr.cp, fb_p.data_ptr(), erased=er)
    f.sync()
    for s, i, off in hits:
        img.flip(s, i, off)
    want = np.full(shards, CLEAN, dtype=np.uint32)
    for s, i, off in hits:
        want[s * n + i] = off // sector
    assert np.array_equal(verdicts(fb_s, shards), want)
    assert np.array_equal(verdicts(fb_p, shards), want)
    pool_h[decoy + 3] ^= 0xFF
    for s, i, off in hits:
        pool_h[int(addr[s * n + i]) + off] ^= 0x10
    assert np.array_equal(pool.cpu().numpy(), pool_h), "the pool was written"
    assert np.array_equal(unsigned(table), addr + np.uint64(pool.data_ptr())), "the table was written"
    # without flags every entry is produced
    t2 = Table(shards, nsec)
    f.crc32c_stripes(*img.args(), sector, t2.ptr, t2.cp)
    f.sync()
    assert np.array_equal(t2.host(), t2.want(model))


# ---------------------------------------------------- what only this can do ----
def test_valid_codeword_of_the_wrong_data():
    """A stripe rewritten wholesale -- one data shard changed, parity
    re-encoded, checksums not updated -- is a codeword: the verify passes, the
    checksums flag the data shard and the four parity shards."""
    k, n, S, sector = 10, 14, 4096 + 100, 4096
    f = fec(k, n)
    img = Img(k, n, S, 2, seed=3, coded=True)
    model = img.model(sector)
    img.shard(1, 4)[:] = img.rng.integers(0, 256, size=S, dtype=np.uint8)
    data = np.concatenate([img.shard(1, i) for i in range(k)])
    par = np.frombuffer(oracle.encode(oracle.fec_matrix(k, n), k, n, data.tobytes()), dtype=np.uint8)
    for i in range(k, n):
        img.shard(1, i)[:] = par[(i - k) * S:(i - k + 1) * S]
    img.upload()
    tab = Table(2 * n, 2, model)
    fbv = dev(np.zeros(2, dtype=np.uint32))
    f.verify_stripes(*img.args(), fbv.data_ptr())
    f.sync()
    assert (unsigned(fbv) == CLEAN).all(), "the rewritten stripe is a codeword"
    got = run_check(f, img, tab, sector)
    bad = sorted(np.flatnonzero(got != CLEAN).tolist())
    assert bad == [n + 4] + [n + i for i in range(k, n)]


# ----------------------------------------------------------------- repair ----
def wreck(img, s, i, rng, sector_only=None):
    """Wrong bytes in shard i of stripe s: all of it, or only inside one sector."""
    sh = img.shard(s, i)
    if sector_only is None:
        sh[:] = sh ^ rng.integers(1, 256, size=len(sh), dtype=np.uint8)
    else:
        lo = sector_only * 4096
        sh[lo + 17:lo + 900] ^= rng.integers(1, 256, size=883, dtype=np.uint8)


def repaired_equals(img, pristine, before, rewritten_shards):
    """After a repair: the rewritten shards hold the pristine bytes over
    [0, S); every other byte of the image is what it was before the call, but
    for the pad up to 16 of a rewritten shard (unspecified)."""
    for b in range(2):
        got = img.d[b].cpu().numpy()
        want = before[b].copy()
        loose = np.zeros(len(want), dtype=bool)
        for s, i in rewritten_shards:
            bb, o = img.at(s, i)
            if bb == b:
                want[o:o + img.S] = pristine[b][o:o + img.S]
                loose[o + img.S:o + r16(img.S)] = True
        bad = np.flatnonzero((got != want) & ~loose)
        assert bad.size == 0, (b, bad[:8].tolist())


def raw_correct(f, args, sector, crcs_ptr, crc_pitch, erased=None, outputs=True):
    """rs_correct_crc32c itself: (return value, status, rewritten).  The binding
    folds RS_ETOO_MANY_ERRORS into the per-stripe status; the return value is
    all a caller has who passes status == NULL (outputs=False)."""
    stripes = args[6]
    buf = ctypes.c_char_p(erased) if erased is not None else None
    st = (ctypes.c_int * stripes)(*([77] * stripes))
    rw = ctypes.create_string_buffer(b"\x07" * (stripes * f.n), stripes * f.n + 1)
    rc = rsmi.load().rs_correct_crc32c(f.handle, *args, ctypes.cast(buf, ctypes.c_void_p), sector, crcs_ptr, crc_pitch,
                                       st if outputs else None, ctypes.cast(rw, ctypes.c_void_p) if outputs else None,
                                       None)
    if not outputs:
        assert list(st) == [77] * stripes and rw.raw[:stripes * f.n] == b"\x07" * (stripes * f.n)
        return rc, None, None
    return rc, list(st), rw.raw[:stripes * f.n]


def test_repair_rs10_4():
    k, n, S, sector = 10, 14, S_REPAIR, 4096
    f = fec(k, n)
    A, B, C, D, E = range(5)
    img = Img(k, n, S, 5, seed=21, coded=True)
    pristine = [a.copy() for a in img.h]
    model = img.model(sector)
    rng = np.random.default_rng(99)
    wrong = {A: [1, 5, 12], B: [0, 3, 10, 13], C: [0, 1, 2, 3, 11], D: [2, 7, 13], E: []}
    for s, ids in wrong.items():
        for i in ids:
            wreck(img, s, i, rng, sector_only=1 if s == B else None)
    img.shard(D, 4, r16(S))[:] = 0xEE  # the erased slot: a guard pattern
    er = flags(5, n, [(D, 4)])
    before = [a.copy() for a in img.h]
    # the gap this call closes: three wrong shards are beyond the column scrub's radius (existing behaviour)
    copy = Img(k, n, S, 5, seed=21)
    copy.h = [a.copy() for a in img.h]
    copy.upload()
    st_cols, _ = f.correct_columns(*copy.args(), erased=er)
    assert st_cols[A] == TOO_MANY
    img.upload()
    tab = Table(5 * n, 4, model)
    sectors0, regen0 = f.stat(f.STAT_CRC_SECTORS), f.stat(f.STAT_CRC_REGENERATED)
    rc, status, rewritten = raw_correct(f, img.args(), sector, tab.ptr, tab.cp, er)
    assert rc == TOO_MANY, "stripe C cannot be repaired: the call must say so"
    assert status == [OK, OK, TOO_MANY, OK, OK]
    located = [(s, i) for s in (A, B, D) for i in wrong[s]]
    assert sorted(x for x in range(5 * n) if rewritten[x]) == sorted(s * n + i for s, i in located)
    repaired_equals(img, pristine, before, located)  # C, E and D's erased slot included: as before the call
    assert np.array_equal(tab.host(), tab.h), "the checksums were written"
    # the check of 5 * 14 - 1 present shards, then of the 10 regenerated ones, 4 sectors each
    assert f.stat(f.STAT_CRC_SECTORS) - sectors0 == (5 * n - 1) * 4 + len(located) * 4
    assert f.stat(f.STAT_CRC_REGENERATED) - regen0 == len(located)
    # again: nothing left to do for A, B, D, E; C as before
    rc, status, rewritten = raw_correct(f, img.args(), sector, tab.ptr, tab.cp, er)
    assert rc == TOO_MANY and status == [OK, OK, TOO_MANY, OK, OK] and not any(rewritten)
    assert raw_correct(f, img.args(), sector, tab.ptr, tab.cp, er, outputs=False)[0] == TOO_MANY
    # and through the binding
    status, rewritten = f.correct_crc32c(*img.args(), sector, tab.ptr, tab.cp, erased=er)
    assert status == [OK, OK, TOO_MANY, OK, OK] and not any(rewritten)
    # the stripes that were repaired, alone (a slice of the same image and table): RS_OK
    two = (*img.args()[:6], 2)
    assert raw_correct(f, two, sector, tab.ptr, tab.cp) == (OK, [OK, OK], bytes(2 * n))
    assert raw_correct(f, two, sector, tab.ptr, tab.cp, outputs=False)[0] == OK


def test_repair_flipped_checksum_is_not_repairable():
    """A stripe whose one bad "shard" is really a flipped checksum: the shard
    is regenerated to the same bytes and still mismatches."""
    k, n, S, sector = 10, 14, S_REPAIR, 4096
    f = fec(k, n)
    img = Img(k, n, S, 2, seed=22, coded=True).upload()
    model = img.model(sector)
    model[n + 6, 2] ^= 0x00010000
    tab = Table(2 * n, 4, model)
    rc, status, rewritten = raw_correct(f, img.args(), sector, tab.ptr, tab.cp)
    assert rc == TOO_MANY
    assert status == [OK, TOO_MANY]
    assert [x for x in range(2 * n) if rewritten[x]] == [n + 6]
    repaired_equals(img, img.h, img.h, [(1, 6)])
    assert np.array_equal(tab.host(), tab.h)


def test_repair_rs64_16():
    k, n, S, sector = 64, 80, S_REPAIR, 4096
    f = fec(k, n)
    img = Img(k, n, S, 2, seed=23, coded=True)
    pristine = [a.copy() for a in img.h]
    model = img.model(sector)
    rng = np.random.default_rng(5)
    wrong = {0: sorted(rng.choice(n, size=16, replace=False).tolist()),
             1: sorted(rng.choice(n, size=17, replace=False).tolist())}
    for s, ids in wrong.items():
        for i in ids:
            wreck(img, s, i, rng)
    before = [a.copy() for a in img.h]
    img.upload()
    tab = Table(2 * n, 4, model)
    rc, status, rewritten = raw_correct(f, img.args(), sector, tab.ptr, tab.cp)
    assert rc == TOO_MANY, "17 wrong shards in stripe 1"
    assert status == [OK, TOO_MANY]
    assert [x for x in range(2 * n) if rewritten[x]] == wrong[0]
    repaired_equals(img, pristine, before, [(0, i) for i in wrong[0]])
    # stripe 0 alone had 16 wrong shards and is whole again: a repair that succeeds returns RS_OK
    img2 = Img(k, n, S, 2, seed=23)
    img2.h = [a.copy() for a in before]
    img2.upload()
    one = (*img2.args()[:6], 1)
    rc, status, rewritten = raw_correct(f, one, sector, tab.ptr, tab.cp)
    assert rc == OK and status == [OK] and [x for x in range(n) if rewritten[x]] == wrong[0]
    repaired_equals(img2, pristine, before, [(0, i) for i in wrong[0]])


def test_repair_erasure_limits():
    """More than m erasures: RS_OK while the stripe is clean, RS_ENOT_ENOUGH
    with nothing written once it has a mismatch too.  m == 0: any mismatch is
    RS_ETOO_MANY_ERRORS."""
    k, n, S, sector = 3, 5, 4097, 512
    f = fec(k, n)
    img = Img(k, n, S, 2, seed=24, coded=True).upload()
    tab = Table(2 * n, 9, img.model(sector))
    er = flags(2, n, [(1, 0), (1, 1), (1, 4)])
    assert raw_correct(f, img.args(), sector, tab.ptr, tab.cp, er) == (OK, [OK, OK], bytes(2 * n))
    status, rewritten = f.correct_crc32c(*img.args(), sector, tab.ptr, tab.cp, erased=er)
    assert status == [OK, OK] and not any(rewritten)
    img.flip(1, 2, 5)
    img.flip(0, 0, 5)  # repairable, but the call is refused as a whole
    with pytest.raises(rsmi.NotEnoughShares):
        f.correct_crc32c(*img.args(), sector, tab.ptr, tab.cp, erased=er)
    assert raw_correct(f, img.args(), sector, tab.ptr, tab.cp, er, outputs=False)[0] == NOT_ENOUGH
    img.flip(1, 2, 5)
    img.flip(0, 0, 5)
    assert img.unchanged()
    f0 = fec(4, 4)
    img0 = Img(4, 4, S, 2, seed=25).upload()
    tab0 = Table(2 * 4, 9, img0.model(sector))
    img0.flip(1, 3, 1000)
    args0 = (img0.d[0].data_ptr() + GUARD, img0.dss, None, 0, img0.pitch, S, 2)
    rc, status, rewritten = raw_correct(f0, args0, sector, tab0.ptr, tab0.cp)
    assert rc == TOO_MANY and status == [OK, TOO_MANY] and not any(rewritten)
    assert raw_correct(f0, args0, sector, tab0.ptr, tab0.cp, outputs=False)[0] == TOO_MANY
    img0.flip(1, 3, 1000)
    assert img0.unchanged()
    assert raw_correct(f0, args0, sector, tab0.ptr, tab0.cp) == (OK, [OK, OK], bytes(2 * 4))


# ---------------------------------------------------------- far addresses ----
def test_stripe_beyond_4gib():
    """Stripe 1 lies 2^32 + 4096 bytes behind stripe 0 in one allocation nobody
    initialises; only the two stripes' bytes are written.  An address cut to 32
    bits would read stripe 0's bytes 4096 further on."""
    k, n, S, sector = 3, 5, 2 * 4096 + 5, 4096
    f = fec(k, n)
    pitch = r16(S) + 16
    stride = (1 << 32) + 4096
    span = n * pitch
    rng = np.random.default_rng(44)
    buf = torch.empty(GUARD + stride + span + 8192 + GUARD, dtype=torch.uint8, device="cuda")
    host = [rng.integers(0, 256, size=span + 8192, dtype=np.uint8) for _ in range(2)]
    for s in range(2):
        buf[GUARD + s * stride:GUARD + s * stride + span + 8192] = dev(host[s])
    data = buf.data_ptr() + GUARD
    args = (data, stride, data + k * pitch, stride, pitch, S, 2)
    nsec = 3
    bufs = [host[s][i * pitch + j * sector:i * pitch + min((j + 1) * sector, S)].tobytes()
            for s in range(2) for i in range(n) for j in range(nsec)]
    model = np.array(rsmi.crc32c_host(bufs), dtype=np.uint32).reshape(2 * n, nsec)
    tab = Table(2 * n, nsec)
    f.crc32c_stripes(*args, sector, tab.ptr, tab.cp)
    fb = first_bad_buf(2 * n)
    f.crc32c_check_stripes(*args, sector, tab.ptr, tab.cp, fb.data_ptr())
    f.sync()
    assert np.array_equal(tab.host(), tab.want(model))
    assert (verdicts(fb, 2 * n) == CLEAN).all()
    buf[GUARD + stride + 4 * pitch + S - 1] ^= 1
    fb = first_bad_buf(2 * n)
    f.crc32c_check_stripes(*args, sector, tab.ptr, tab.cp, fb.data_ptr())
    f.sync()
    want = np.full(2 * n, CLEAN, dtype=np.uint32)
    want[n + 4] = 2
    assert np.array_equal(verdicts(fb, 2 * n), want)
    # the pointer twin on the same far shards
    addr = np.array([data + s * stride + i * pitch for s in range(2) for i in range(n)], dtype=np.uint64)
    table = dev(addr)
    tab_p = Table(2 * n, nsec)
    fb = first_bad_buf(2 * n)
    f.crc32c_ptrs(table.data_ptr(), S, 2, sector, tab_p.ptr, tab_p.cp)
    f.crc32c_check_ptrs(table.data_ptr(), S, 2, sector, tab.ptr, tab.cp, fb.data_ptr())
    f.sync()
    model[n + 4, 2] = rsmi.crc32c_host([bytes(host[1][4 * pitch + 2 * sector:4 * pitch + S - 1]) +
                                        bytes([host[1][4 * pitch + S - 1] ^ 1])])[0]
    assert np.array_equal(tab_p.host(), tab_p.want(model))
    assert np.array_equal(verdicts(fb, 2 * n), want)
    for s in range(2):
        got = buf[GUARD + s * stride:GUARD + s * stride + span + 8192].cpu().numpy()
        if s == 1:
            got[4 * pitch + S - 1] ^= 1
        assert np.array_equal(got, host[s])
    del buf
    torch.cuda.empty_cache()


# ------------------------------------------------------- names, arguments ----
def test_kernel_names():
    f = fec(10, 14)
    assert f.kernel_name(18).startswith("crc32c")
    assert f.kernel_name(19).startswith("crc32c") and f.kernel_name(19).endswith("_ptrs")
    assert f.kernel_name(18) != f.kernel_name(19)


def test_argument_validation(checked):
    f, img, tab, sector = checked
    n, shards = img.n, 3 * img.n
    fb = first_bad_buf(shards)
    a = img.args()
    table = dev(np.zeros(shards, dtype=np.uint64))
    fresh = Table(shards, 4)

    def refused(call, *args, **kw):
        with pytest.raises(rsmi.RSError) as ei:
            call(*args, **kw)
        assert ei.value.code == EINVAL, (call.__name__, args)

    for s_len in (0, 256, 3000, 4097, 131072):
        refused(f.crc32c_stripes, *a, s_len, fresh.ptr, fresh.cp)
        refused(f.crc32c_check_stripes, *a, s_len, tab.ptr, tab.cp, fb.data_ptr())
        refused(f.crc32c_ptrs, table.data_ptr(), img.S, 3, s_len, fresh.ptr, fresh.cp)
        refused(f.crc32c_check_ptrs, table.data_ptr(), img.S, 3, s_len, tab.ptr, tab.cp, fb.data_ptr())
        refused(f.correct_crc32c, *a, s_len, tab.ptr, tab.cp)
    for crcs in (0, fresh.ptr + 2):
        refused(f.crc32c_stripes, *a, sector, crcs, fresh.cp)
        refused(f.crc32c_check_stripes, *a, sector, crcs, fresh.cp, fb.data_ptr())
        refused(f.crc32c_ptrs, table.data_ptr(), img.S, 3, sector, crcs, fresh.cp)
        refused(f.crc32c_check_ptrs, table.data_ptr(), img.S, 3, sector, crcs, fresh.cp, fb.data_ptr())
        refused(f.correct_crc32c, *a, sector, crcs, fresh.cp)
    for bad_fb in (0, fb.data_ptr() + 1):
        refused(f.crc32c_check_stripes, *a, sector, tab.ptr, tab.cp, bad_fb)
        refused(f.crc32c_check_ptrs, table.data_ptr(), img.S, 3, sector, tab.ptr, tab.cp, bad_fb)
    # crc_pitch < nsec
    refused(f.crc32c_stripes, *a, sector, fresh.ptr, 3)
    refused(f.crc32c_check_stripes, *a, sector, tab.ptr, 3, fb.data_ptr())
    refused(f.correct_crc32c, *a, sector, tab.ptr, 3)
    refused(f.crc32c_ptrs, table.data_ptr(), img.S, 3, sector, fresh.ptr, 3)
    refused(f.crc32c_check_ptrs, table.data_ptr(), img.S, 3, sector, tab.ptr, 3, fb.data_ptr())
    # stripes * n >= 2^32
    many = (1 << 32) // n + 1
    refused(f.crc32c_stripes, *a[:6], many, sector, fresh.ptr, fresh.cp)
    refused(f.crc32c_ptrs, table.data_ptr(), img.S, many, sector, fresh.ptr, fresh.cp)
    refused(f.crc32c_check_ptrs, table.data_ptr(), img.S, many, sector, tab.ptr, tab.cp, fb.data_ptr())
    refused(f.crc32c_check_stripes, *a[:6], many, sector, tab.ptr, tab.cp, fb.data_ptr())
    # what rs_verify_stripes / rs_verify_ptrs refuse
    refused(f.crc32c_stripes, a[0] + 8, *a[1:], sector, fresh.ptr, fresh.cp)
    refused(f.crc32c_stripes, a[0], a[1] + 8, *a[2:], sector, fresh.ptr, fresh.cp)
    refused(f.crc32c_stripes, *a[:4], r16(img.S) - 16, *a[5:], sector, fresh.ptr, fresh.cp)
    refused(f.crc32c_check_stripes, a[0], a[1], 0, *a[3:], sector, tab.ptr, tab.cp, fb.data_ptr())
    refused(f.crc32c_ptrs, 0, img.S, 3, sector, fresh.ptr, fresh.cp)
    refused(f.crc32c_check_ptrs, table.data_ptr() + 4, img.S, 3, sector, tab.ptr, tab.cp, fb.data_ptr())
    f.sync()
    assert np.array_equal(fresh.host(), fresh.h) and np.array_equal(tab.host(), tab.h)
    assert (unsigned(fb) == 0x12345678).all()
    assert img.unchanged()
    # nothing to do
    f.crc32c_stripes(*a[:6], 0, sector, 0, 0)
    f.crc32c_check_stripes(*a[:5], 0, 3, sector, 0, 0, 0)
    f.crc32c_ptrs(0, 0, 3, sector, 0, 0)
    assert f.correct_crc32c(*a[:6], 0, sector, 0, 0) == ([], b"")

"""GPU: rs_correct_columns_ptrs_lens -- the column scrub of the pointer
placement for stripes that each have a shard length of their own.

Every case works on a lens_pool.LensPool: one device buffer between guard
bands, every shard at a random row of round_up(S_max, 16) + 32 bytes, stripe s
using the first S_s bytes of its rows and random bytes -- no continuation of
the codeword -- behind them.  Table entries of erased shards name decoy rows.
After every call the WHOLE buffer and the device table are compared with the
expected image, which never comes from the engine (lens_columns.ColumnRun,
proved on the CPU by test_lens_columns_model.py): pristine bytes for damage
within the radius, the oracle's per-column decode_correct beyond it.
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
from lens_columns import CLEAN, COUNT_SENTINEL, OK, STATUS_SENTINEL, TOO_MANY, ColumnRun, oracle_column  # noqa: E402
from lens_pool import LensPool, deal, windows  # noqa: E402
from strided_image import r16  # noqa: E402

# MG4, radius 1, register pointers | radius 2 | MG8 | MG16 | two rounds of 32
# LDS sources | r up to 256 | no radius | no parity
CODES = {"rs4_6": (4, 6), "rs10_14": (10, 14), "rs8_14": (8, 14), "rs3_19": (3, 19), "rs64_80": (64, 80),
         "rs240_256": (240, 256), "rs4_5": (4, 5), "rs4_4": (4, 4)}
TWIN = {"rs4_6": "columns_MG4_B256_ptrs_lens", "rs10_14": "columns_MG4_B256_ptrs_lens",
        "rs8_14": "columns_MG8_B256_ptrs_lens", "rs3_19": "columns_MG16_B256_ptrs_lens",
        "rs64_80": "columns_MG16_B256_ptrs_lens", "rs240_256": "columns_MG16_B256_ptrs_lens",
        "rs4_5": "columns_MG4_B256_ptrs_lens", "rs4_4": "none"}
# one column, a sub-column, two columns with one byte in the second, nothing |
# one 4 KiB chunk exactly, a chunk and a column | several chunks, no multiple of 16
MIXES = {"tiny": [16, 1, 17, 0], "chunk": [4096, 4112, 16, 0], "odd": [5000, 1, 3 * 4096 + 40, 17]}
MAIN = ("rs4_6", "rs10_14", "rs8_14", "rs3_19", "rs64_80")
CASES = ([(c, mix, st) for c in MAIN for st in (2, 3) for mix in MIXES] +
         [(c, mix, 37) for c in MAIN for mix in ("tiny", "chunk")] + [("rs10_14", "odd", 37)] +
         [("rs240_256", mix, st) for mix in ("tiny", "chunk") for st in (2, 3, 37)])

_POOLS = {}
_FECS = {}


def pool(code, lens):
    key = (code, tuple(lens))
    if key not in _POOLS:
        while len(_POOLS) >= 8:
            del _POOLS[next(iter(_POOLS))]
        k, n = CODES[code]
        _POOLS[key] = LensPool(k, n, lens, seed=k * 1000003 + n * 10007 + sum((i + 1) * x for i, x in enumerate(lens)))
    return _POOLS[key]


def fec(code):
    if code not in _FECS:
        _FECS[code] = rsmi.FEC(*CODES[code], device=0)
    return _FECS[code]


def deals(code, mix, stripes, **kw):
    """The pools of a case: every window of the mix's shuffle."""
    k, n = CODES[code]
    for w in range(windows(MIXES[mix], stripes)):
        yield w, pool(code, deal(MIXES[mix], stripes, seed=k + 7 * n + stripes, window=w, **kw))


def flags_cycle(P, shift, seed):
    """(s + shift) mod (m - 1) erasures in stripe s, 0 .. m - 2: every stripe
    keeps r - k >= 2; the ids are seeded."""
    rng = np.random.default_rng(seed)
    er = np.zeros((P.stripes, P.n), dtype=np.uint8)
    for s in range(P.stripes):
        er[s, rng.choice(P.n, size=(s + shift) % max(P.m - 1, 1), replace=False)] = 1
    return er


def damaged_stripes(stripes):
    """Every third stripe: both neighbours of a damaged stripe stay clean."""
    return list(range(1, stripes, 3)) if stripes >= 3 else [0]


STATS = ("STAT_COLUMN_STRIPES", "STAT_COLUMN_BYTES", "STAT_COLUMN_LENS_LAUNCHES", "STAT_SCRUB_LENS_LAUNCHES",
         "STAT_CHECK_STRIPES")


def stats(f):
    return [f.stat(getattr(f, w)) for w in STATS]


def run_and_count(f, run, what):
    """run.run, and the stats: the model's dirty stripes and corrected bytes,
    one twin launch when there is a job, a verify launch for each verify."""
    before = stats(f)
    st, cnt = run.run(f, torch, what)
    jobs = run.jobs()
    moved = [a - b for a, b in zip(stats(f), before)]
    e = run.er.sum(axis=1)
    live = np.array(run.P.lens) > 0
    degraded = live & (e > 0) & (e < run.P.m)  # what rs_verify_ptrs_lens counts as checked
    assert moved == [len(jobs), int(run.counts.sum()), 1 if jobs else 0, 2 if jobs else 1,
                     int(degraded.sum()) + int(degraded[jobs].sum())], (what, moved)
    return st, cnt


# ------------------------------------- 1. scattered damage within the radius ----
@pytest.mark.parametrize("code,mix,stripes", CASES)
def test_scattered_damage_is_corrected(code, mix, stripes):
    f = fec(code)
    for w, P in deals(code, mix, stripes):
        for shift in (None, w):
            er = None if shift is None else flags_cycle(P, shift, seed=100 * w + stripes)
            run = ColumnRun(P, er, seed=w)
            rng = np.random.default_rng(1000 * w + stripes)
            for s0 in damaged_stripes(stripes):
                s = (s0 + w) % stripes if stripes < 3 else s0
                if P.lens[s] == 0:
                    run.flip(s, run.present(s)[0], 0)  # at its length: not the stripe's byte
                run.scatter(s, rng)
            what = f"{code} {P.lens} flags {shift}"
            st, cnt = run_and_count(f, run, what)
            assert st == [OK] * stripes
            below = np.ones(len(run.want), dtype=bool)
            for s, offs in run.touched.items():
                for i in run.present(s):
                    for off in offs:
                        if off >= P.lens[s]:
                            below[run.at(s, i) + off] = False
            assert np.array_equal(run.want[below], run.base[below]), what  # pristine but for the lost shards' rows
            assert (run.verify(f, torch) == CLEAN).all(), what
            run.check(what + ", verified")


# ------------------------------------------------------ 2. a job's own length ----
@pytest.mark.parametrize("longest", ["first", "last"])
@pytest.mark.parametrize("mix", ["tiny", "odd"])
@pytest.mark.parametrize("code", MAIN)
def test_a_job_decodes_at_its_own_length(code, mix, longest):
    """Every stripe with bytes is dirty but one, which is damaged only at and
    beyond its length.  Dirty stripes with S % 16 != 0 also carry a flip at S
    (in their last column's pad) and one at round_up(S, 16): a kernel that
    decodes with a neighbour's or the longest length repairs the first, a
    second verify at another length fails the stripe."""
    f = fec(code)
    for w, P in deals(code, mix, 3, longest=longest):
        assert P.lens[0 if longest == "first" else -1] == max(P.lens)
        er = flags_cycle(P, w, seed=7 + w) if w % 2 else None
        run = ColumnRun(P, er, seed=w)
        rng = np.random.default_rng(31 + w)
        only_beyond = (w + 1) % 3
        kept = []
        for s, S in enumerate(P.lens):
            i, j = run.present(s)[s % 2], run.present(s)[-1 - s % 2]
            for off, who, mask in ((S, i, 0x01), (r16(S), j, 0xFF)):  # two shards: one offset when S % 16 == 0
                run.flip(s, who, off, mask)
                kept.append(run.at(s, who) + off)
            if s != only_beyond:
                run.scatter(s, rng, extra=2)
        what = f"{code} {P.lens} beyond {only_beyond}"
        st, cnt = run_and_count(f, run, what)
        assert st == [OK] * 3
        assert cnt[only_beyond].sum() == 0 and only_beyond not in run.jobs()
        assert all(run.want[o] != P.pristine[o] for o in kept)  # the model keeps them, and check() held the image to it
        assert (run.verify(f, torch) == CLEAN).all(), what


# ------------------------------------------- 3. neighbours of a dirty stripe ----
@pytest.mark.parametrize("code", MAIN)
def test_neighbours_of_dirty_stripes_are_untouched(code):
    f = fec(code)
    P = pool(code, [4112, 0, 16, 17, 0, 4096, 1])
    er = np.zeros((P.stripes, P.n), dtype=np.uint8)
    if P.m > 2:
        er[1, 0] = er[3, 2] = er[5, P.n - 1] = 1  # a zero-length, a dirty and a clean stripe with a flag
    run = ColumnRun(P, er, seed=3)
    rng = np.random.default_rng(5)
    for s in (0, 3, 6):
        run.scatter(s, rng)
    st, cnt = run_and_count(f, run, code)
    assert st == [OK] * 7 and run.jobs() == [0, 3, 6]
    assert cnt[[1, 2, 4, 5]].sum() == 0


# ---------------------------------------------------- 4. beyond the radius ----
def hopeless_column(run, s, off, seed):
    """radius + 1 flips in column off of stripe s for which the oracle finds
    no codeword (most draws: the spheres of the code are sparse)."""
    P = run.P
    for t in range(64):
        rng = np.random.default_rng(1000 * seed + t)
        who = [int(i) for i in rng.choice(run.present(s), size=run.radius(s) + 1, replace=False)]
        masks = [int(x) for x in rng.integers(1, 256, size=len(who))]
        col = dict(run.column(s, off))
        for i, mk in zip(who, masks):
            col[i] ^= mk
        if oracle_column(P.k, P.n, sorted(col.items()))[0] != 0:
            for i, mk in zip(who, masks):
                run.flip(s, i, off, mk)
            return
    raise AssertionError("no hopeless column found")


@pytest.mark.parametrize("code,flagged", [("rs10_14", False), ("rs4_6", False), ("rs10_14", True), ("rs64_80", True)])
def test_beyond_the_radius(code, flagged):
    f = fec(code)
    P = pool(code, [4112, 17, 0, 5000])
    er = np.zeros((P.stripes, P.n), dtype=np.uint8)
    if flagged:
        er[1, 2] = 1
        er[3, [0, P.n - 1]] = 1
    run = ColumnRun(P, er, seed=4)
    rng = np.random.default_rng(77)
    hopeless_column(run, 1, 16, seed=11)  # the one-byte second column of the short stripe
    run.flip(1, run.present(1)[3], 3, 0x10)  # its other columns are repaired
    run.flip(1, run.present(1)[0], 15, 0x08)
    run.scatter(3, rng)
    st, cnt = run_and_count(f, run, f"beyond radius {code}")
    assert st == [OK, TOO_MANY, OK, OK]
    assert cnt[1].sum() == 2
    fb = run.verify(f, torch)
    assert fb.tolist() == [CLEAN, 16, CLEAN, CLEAN]
    # the return value, through the C ABI, with NULL status and corrected
    tp = run.upload(torch)
    buf = ctypes.c_char_p(run.flags()) if run.flags() else None
    lens = (ctypes.c_size_t * P.stripes)(*P.lens)
    rc = rsmi.load().rs_correct_columns_ptrs_lens(f._h, tp, lens, P.stripes, ctypes.cast(buf, ctypes.c_void_p), None, None, None)
    assert rc == TOO_MANY
    run.check(f"beyond radius {code}, NULL status and corrected")


@pytest.mark.parametrize("code,gone", [("rs4_5", 0), ("rs10_14", 3), ("rs4_6", 1)])
def test_no_radius_is_failed_and_unwritten(code, gone):
    """r - k < 2 in stripes 1 and 2: an error can be seen, not located."""
    f = fec(code)
    P = pool(code, [4112, 17, 5000, 0, 16])
    er = np.zeros((P.stripes, P.n), dtype=np.uint8)
    er[1, :gone] = er[2, P.n - gone:] = 1
    if P.m >= 2:
        er[3, 0] = 1
    run = ColumnRun(P, er, seed=6)
    run.flip(1, run.present(1)[1], 16, 0x01)
    run.flip(2, run.present(2)[0], 4999, 0x80)
    run.flip(0, 0, 4111, 0x01)  # a whole stripe next to them: repaired where the code can
    run.flip(4, 1, 0, 0x55)
    st, cnt = run_and_count(f, run, f"no radius {code}")
    whole = OK if P.m >= 2 else TOO_MANY
    assert st == [whole, TOO_MANY, TOO_MANY, OK, whole]
    assert cnt[[1, 2, 3]].sum() == 0 and cnt.sum() == (2 if P.m >= 2 else 0)
    for s in (1, 2):
        for i in run.present(s):
            o = run.at(s, i)
            assert np.array_equal(run.want[o:o + P.row_bytes], run.cur[o:o + P.row_bytes])


# ---------------------------------------- 5. agreement with the other routes ----
@pytest.mark.parametrize("code,mix,stripes", [c for c in CASES if c[2] != 37 or c[1] == "chunk"])
def test_equals_one_call_per_length(code, mix, stripes):
    f = fec(code)
    for w, P in deals(code, mix, stripes):
        er = flags_cycle(P, w + 1, seed=300 + w)
        runs = [ColumnRun(P, er, seed=w) for _ in range(2)]
        for run in runs:
            rng = np.random.default_rng(9 + w)
            for s in range(0, stripes, 2):
                run.scatter(s, rng, extra=2)
        lens_st, lens_cnt = runs[0].call(f, torch)
        each_st, each_cnt = runs[1].call_by_length(f, torch)
        assert lens_st == each_st and np.array_equal(lens_cnt, each_cnt), (P.lens, lens_st, each_st)
        assert np.array_equal(runs[0].image(), runs[1].image())
        runs[0].expect().check("the call against the model")


@pytest.mark.parametrize("code", MAIN)
def test_equal_lengths_are_the_equal_length_call(code):
    f = fec(code)
    S, stripes = 4112, 3
    P = pool(code, [S] * stripes)
    er = flags_cycle(P, 1, seed=5)
    runs = [ColumnRun(P, er) for _ in range(2)]
    for run in runs:
        run.scatter(1, np.random.default_rng(2))
    before = stats(f)
    a_st, a_cnt = runs[0].run(f, torch, "pass-through")
    mid = stats(f)
    tp = runs[1].upload(torch)
    b_st, b_cnt = f.correct_columns_ptrs(tp, S, stripes, erased=runs[1].flags())
    after = stats(f)
    assert a_st == b_st and np.array_equal(a_cnt.reshape(-1), np.asarray(b_cnt, dtype=np.int64))
    assert np.array_equal(runs[0].image(), runs[1].image())
    lens_launches = (STATS.index("STAT_COLUMN_LENS_LAUNCHES"), STATS.index("STAT_SCRUB_LENS_LAUNCHES"))
    assert all(before[q] == mid[q] == after[q] for q in lens_launches), "an equal-length call ran the per-length kernels"
    assert [m - b for m, b in zip(mid, before)] == [x - m for x, m in zip(after, mid)], "not the same stats"
    assert mid[0] - before[0] == 1 and mid[1] - before[1] == int(runs[0].counts.sum())


# ----------------------------------------------------------- 6. refusals ----
def test_refusals_write_nothing():
    lib = rsmi.load()
    f = fec("rs10_14")
    P = pool("rs10_14", [4112, 0, 17])
    er = np.zeros((3, P.n), dtype=np.uint8)
    er[0, [0, 5]] = 1
    er[2, 3] = 1
    run = ColumnRun(P, er)
    run.flip(2, 0, 3)
    run.flip(0, 1, 4100)
    tp = run.upload(torch)
    status = (ctypes.c_int32 * 3)(*[STATUS_SENTINEL] * 3)
    corrected = np.full(3 * P.n, COUNT_SENTINEL, dtype=np.uint32)
    max_len = ((1 << 28) - 1) * 16
    before = stats(f)

    def call(table=tp, lens=P.lens, stripes=3, flags=er, h=f._h):
        buf = ctypes.c_char_p(flags.tobytes()) if flags is not None else None
        arr = (ctypes.c_size_t * len(lens))(*lens) if lens is not None else None
        return lib.rs_correct_columns_ptrs_lens(h, table, arr, stripes, ctypes.cast(buf, ctypes.c_void_p), status,
                                                ctypes.c_void_p(corrected.ctypes.data), None)

    assert call(h=None) == rsmi.RS_EINVAL
    assert call(lens=None) == rsmi.RS_EINVAL
    assert call(table=None) == rsmi.RS_EINVAL
    assert call(table=tp + 4) == rsmi.RS_EINVAL
    assert call(stripes=1 << 32) == rsmi.RS_EINVAL
    assert call(lens=[4112, max_len + 1, 17]) == rsmi.RS_EINVAL  # 2^28 columns
    assert call(lens=[4112, 0, 1 << 40]) == rsmi.RS_EINVAL
    # more than 2^31 - 1 blocks in the worst-case column launch (and in the
    # first verify launch): 2,048 stripes of 2^20 chunks each, none of them read
    assert "RSMI_ITERS" not in os.environ  # blocks of more than one chunk would make these calls servable
    many = np.zeros((2048, P.n), dtype=np.uint8)
    assert call(lens=[max_len] * 2048, stripes=2048, flags=many) == rsmi.RS_EINVAL
    assert call(lens=[max_len] * 2048, stripes=2048, flags=None) == rsmi.RS_EINVAL
    # more than m erasures: in a stripe with bytes, and in the zero-length one
    for s in (2, 1):
        too_many = er.copy()
        too_many[s, [1, 2, 4, 6, 8]] = 1
        assert call(flags=too_many) == rsmi.RS_ENOT_ENOUGH
    with pytest.raises(rsmi.RSError):
        f.correct_columns_ptrs_lens(tp, [16, 17], 3)  # one length per stripe
    with pytest.raises(rsmi.RSError):
        f.correct_columns_ptrs_lens(tp, P.lens, 3, erased=bytes(5))
    # the verify launches alone: RS(3,19) verifies in two row groups of 8, so
    # 1,024 such stripes are 2^30 column blocks and 2^31 verify blocks
    f2 = fec("rs3_19")
    assert f2.kernel_name(14) == "verify_K0_MG8_B256_lens" and "RSMI_ITERS" not in os.environ
    before2 = stats(f2)
    assert call(lens=[max_len] * 1024, stripes=1024, flags=None, h=f2._h) == rsmi.RS_EINVAL
    assert stats(f2) == before2
    # m > 16
    f17 = rsmi.FEC(4, 21, device=0)
    assert f17.kernel_name(17) == "none"
    assert call(flags=None, h=f17._h) == rsmi.RS_EINVAL
    assert [f17.stat(getattr(f17, w)) for w in STATS] == [0] * len(STATS)
    f17.close()
    f.sync()
    run.check("refused calls", want=run.cur)
    assert list(status) == [STATUS_SENTINEL] * 3 and (corrected == COUNT_SENTINEL).all()
    assert stats(f) == before
    # empty calls: RS_OK; stripes == 0 writes nothing, all lengths 0 reports every stripe clean
    assert call(stripes=0, lens=None, flags=None, table=None) == rsmi.RS_OK
    assert list(status) == [STATUS_SENTINEL] * 3 and (corrected == COUNT_SENTINEL).all()
    assert call(lens=[0, 0, 0]) == rsmi.RS_OK
    assert list(status) == [OK] * 3 and (corrected == 0).all()
    run.check("empty calls", want=run.cur)
    assert stats(f) == before


def test_no_parity_is_ok():
    """RS(4,4): every stripe is a codeword, nothing read or written; any flag is one too many."""
    f = fec("rs4_4")
    P = pool("rs4_4", [4112, 0, 17, 5000])
    run = ColumnRun(P)
    run.flip(0, 2, 5)
    before = stats(f)
    st, cnt = run.run(f, torch, "m == 0")
    assert st == [OK] * 4 and cnt.sum() == 0 and stats(f) == before
    one = np.zeros((4, 4), dtype=np.uint8)
    one[1, 2] = 1  # in the zero-length stripe
    with pytest.raises(rsmi.NotEnoughShares):
        f.correct_columns_ptrs_lens(run.table.data_ptr(), P.lens, 4, erased=one.tobytes())
    run.check("m == 0, refused", want=run.cur)


# ------------------------------------------------ 7. names and concurrency ----
@pytest.mark.parametrize("code", sorted(CODES))
def test_kernel_names(code):
    f = fec(code)
    assert f.kernel_name(17) == TWIN[code]
    assert f.kernel_name(11) == TWIN[code].replace("_lens", "")


def test_device_set():
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert fs.kernel_name(17) == "columns_MG4_B256_ptrs_lens"
    P = pool("rs10_14", [5000, 0, 17, 4096])
    run = ColumnRun(P, flags_cycle(P, 1, seed=9))
    rng = np.random.default_rng(3)
    run.scatter(0, rng)
    run.scatter(2, rng)
    st, cnt = run_and_count(fs, run, "device set")  # the stats are summed over the members
    assert st == [OK] * 4 and run.jobs() == [0, 2]
    fs.close()


def test_two_threads_one_context():
    f = fec("rs10_14")
    pools = [pool("rs10_14", [5000, 17, 0, 4112]), pool("rs10_14", [1, 3 * 4096 + 40, 16])]  # built ahead of the threads
    runs = []
    for t, P in enumerate(pools):
        mine = []
        for rep in range(4):
            run = ColumnRun(P, flags_cycle(P, rep, seed=10 * t + rep), seed=rep)
            rng = np.random.default_rng(20 * t + rep)
            for s in range(rep % 2, P.stripes, 2):
                run.scatter(s, rng, extra=2)
            mine.append(run.expect())
        runs.append(mine)
    errors = []

    def work(t):
        try:
            for rep, run in enumerate(runs[t]):
                st, cnt = run.call(f, torch)
                assert st == run.status and np.array_equal(cnt, run.counts), (st, run.status)
                run.check(f"thread {t} rep {rep}")
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors

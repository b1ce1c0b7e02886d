"""GPU: rs_verify_ptrs_lens and rs_reconstruct_checked_ptrs_lens -- the scrub
and the checked repair of the pointer placement for stripes that each have a
shard length of their own.

Every case works on a lens_pool.LensPool: one device buffer between guard
bands, every shard at a random row of round_up(S_max, 16) + 32 bytes, stripe s
using the first S_s bytes of its rows and random bytes -- no continuation of
the codeword -- behind them.  Table entries of erased shards name decoy rows
(for a repair distinct ones, the destinations).  After every call the WHOLE
buffer and the device table are compared with the expected image.  Expected
bytes never come from the engine: payload is seeded, parity and regenerated
shards come from the oracle (lens_pool.LensRun.expect).
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
from lens_pool import CLEAN, MIX, SENTINEL, LensPool, LensRun, deal, windows  # noqa: E402
from strided_image import r16  # noqa: E402

# register pointers (K4, K10) | two row groups (K8, m = 6) | runtime k, five
# row groups of the jobs (m = 16 .. 1 compared rows) | LDS pointers, MG = 16
# verify | r up to 256 | m = 0
CODES = {"rs4_6": (4, 6), "rs10_14": (10, 14), "rs8_14": (8, 14), "rs3_19": (3, 19), "rs64_80": (64, 80),
         "rs240_256": (240, 256), "rs4_4": (4, 4)}
VERIFY_NAME = {"rs4_6": "verify_K4_MG4_B256", "rs10_14": "verify_K10_MG4_B256", "rs8_14": "verify_K8_MG6_B256",
               "rs3_19": "verify_K0_MG8_B256", "rs64_80": "verify_K64_MG16_B256", "rs240_256": "verify_K0_MG8_B256",
               "rs4_4": "verify_K4_MG4_B256"}
JOB_K = {"rs4_6": 4, "rs10_14": 10, "rs8_14": 8, "rs3_19": 0, "rs64_80": 64, "rs240_256": 0, "rs4_4": 4}
# Every mix is a part of lens_pool.MIX; the first two are the smallest.
MIXES = {"tiny": [16, 1, 17, 0], "chunk": [4096, 4112, 16, 0], "odd": [5000, 1, 3 * 4096 + 40, 17], "full": MIX}
MAIN = ("rs4_6", "rs10_14", "rs8_14", "rs3_19", "rs64_80")
CASES = ([(c, mix, st) for c in MAIN for st in (2, 3) for mix in MIXES] +
         [(c, mix, 37) for c in MAIN for mix in ("tiny", "chunk")] +
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
    """Per-stripe erasure counts (s + shift) mod (m + 1): intact, degraded and
    saturated stripes side by side; the ids are seeded."""
    rng = np.random.default_rng(seed)
    er = np.zeros((P.stripes, P.n), dtype=np.uint8)
    for s in range(P.stripes):
        er[s, rng.choice(P.n, size=(s + shift) % (P.m + 1), replace=False)] = 1
    return er


def shifts(P):
    """Shifts of flags_cycle: with more than m stripes every count 0 .. m is in
    one call whatever the shift; two or three stripes get, over three calls,
    {intact, degraded}, {degraded, degraded} and {degraded, saturated}."""
    return (0, 5) if P.stripes > P.m else sorted({0, 1, max(P.m - 1, 0)})


def damage(run, s, kind, who):
    """One kind of damage in stripe s; returns the verdict it must get if the
    stripe has anything to compare (else CLEAN).  who picks the shard: a data
    shard, a parity shard, a survivor, a compared non-survivor -- whichever of
    them the stripe has present."""
    P = run.P
    S = P.lens[s]
    cands = [[i for i in run.present(s) if i < P.k], [i for i in run.present(s) if i >= P.k],
             run.survivors(s), run.compared(s)]
    cands = [c for c in cands if c]
    shard = cands[who % len(cands)]
    i = shard[(s + who) % len(shard)]
    can_tell = bool(run.compared(s)) and S > 0
    if S == 0:
        run.flip(s, i, 0)  # at S: not the stripe's byte
        return CLEAN
    if kind == 0:
        run.flip(s, i, 0)
        return 0 if can_tell else CLEAN
    if kind == 1:
        run.flip(s, i, S - 1, 0x80)
        return S - 1 if can_tell else CLEAN
    if kind == 2:  # the first byte behind the stripe's length: in the last column when S % 16 != 0
        run.flip(s, i, S, 0x01)
        return CLEAN
    if kind == 3:  # the first byte behind the columns the stripe has
        run.flip(s, i, r16(S), 0xFF)
        return CLEAN
    lo, hi = (S // 3, S - 1) if S > 1 else (0, 0)  # two flips: the lower offset wins
    j = shard[(s + who + 1) % len(shard)]
    if hi > lo:
        run.flip(s, j, hi, 0x04)
    run.flip(s, i, lo, 0x02)
    return lo if can_tell else CLEAN


def damaged_stripes(stripes):
    """Every third stripe: both neighbours of a damaged stripe stay clean."""
    return list(range(1, stripes, 3)) if stripes >= 3 else [0]


def run_damaged(f, P, er, repair, rounds, what):
    """Damage of every kind in the chosen stripes (round r starts the rotation
    at kind r and moves the damaged stripes by r); verdicts against the model
    AND against the offsets the damage was put at."""
    for r in rounds:
        run = LensRun(P, er, repair=repair, seed=r)
        told = np.full(P.stripes, CLEAN, dtype=np.uint32)
        for q, s0 in enumerate(damaged_stripes(P.stripes)):
            s = (s0 + (r if P.stripes < 3 else 0)) % P.stripes
            told[s] = damage(run, s, (q + r) % 5, q + r)
        got = run.run(f, torch, f"{what} round {r}")
        assert np.array_equal(got, told), (what, r, P.lens, got.tolist(), told.tolist())


# ------------------------------------------------------ 1. clean verify ----
@pytest.mark.parametrize("code,mix,stripes", CASES)
def test_verify_clean(code, mix, stripes):
    f = fec(code)
    for w, P in deals(code, mix, stripes):
        for erased in (None, bytes(stripes * P.n)):
            run = LensRun(P)
            got = run.run(f, torch, f"{code} {P.lens} clean", erased=erased)
            assert (got == CLEAN).all()
            run.check("clean", want=P.pristine)


# ----------------------------------------------------------- 2. damage ----
@pytest.mark.parametrize("code,mix,stripes", CASES)
def test_verify_damage(code, mix, stripes):
    f = fec(code)
    for w, P in deals(code, mix, stripes):
        run_damaged(f, P, None, False, range(5) if stripes < 37 else range(2), f"{code} {P.lens} intact")


# -------------------------------------------------- 3. degraded verify ----
@pytest.mark.parametrize("longest", ["first", "last"])
@pytest.mark.parametrize("code,mix,stripes", CASES)
def test_verify_degraded(code, mix, stripes, longest):
    f = fec(code)
    for w, P in deals(code, mix, stripes, longest=longest):
        assert P.lens[0 if longest == "first" else -1] == max(P.lens)
        for shift in shifts(P):
            er = flags_cycle(P, shift, seed=100 * w + shift)
            run = LensRun(P, er, seed=shift)
            got = run.run(f, torch, f"{code} {P.lens} shift {shift} clean")
            assert (got == CLEAN).all()
            run_damaged(f, P, er, False, [shift % 5], f"{code} {P.lens} shift {shift}")


# --------------------------------------------------- 4. checked repair ----
@pytest.mark.parametrize("code,mix,stripes", CASES)
def test_repair(code, mix, stripes):
    """Verdicts, the slots' first r16(S_s) bytes against the oracle, every
    other byte of the pool untouched."""
    f = fec(code)
    for w, P in deals(code, mix, stripes, longest="last" if stripes == 3 else None):
        for shift in shifts(P):
            er = flags_cycle(P, shift + 1, seed=200 * w + shift)
            run = LensRun(P, er, repair=True, seed=shift)
            got = run.run(f, torch, f"{code} {P.lens} shift {shift} clean")
            assert (got == CLEAN).all()
            written = sum(r16(P.lens[s]) * int(er[s].sum()) for s in range(P.stripes))
            assert int((run.want != run.cur).sum()) <= written and (written == 0 or (run.want != run.cur).any())
            run_damaged(f, P, er, True, [(shift + 1) % 5], f"{code} {P.lens} shift {shift}")


# ----------------------------------------------- 5. engine against engine ----
@pytest.mark.parametrize("repair", [False, True])
@pytest.mark.parametrize("code,mix,stripes", CASES)
def test_equals_the_equal_length_calls(code, mix, stripes, repair):
    """For each distinct length the equal-length call on a sub-table of the
    stripes of that length: the same verdicts, the same bytes."""
    f = fec(code)
    for w, P in deals(code, mix, stripes):
        er = flags_cycle(P, w + 1, seed=300 + w)
        runs = [LensRun(P, er, repair=repair, seed=w) for _ in range(2)]
        for q, s in enumerate(damaged_stripes(stripes)):
            for run in runs:
                damage(run, s, q % 5, q)
        lens_fb = runs[0].call(f, torch)
        each_fb = runs[1].call_by_length(f, torch)
        assert np.array_equal(lens_fb, each_fb), (P.lens, lens_fb.tolist(), each_fb.tolist())
        assert np.array_equal(runs[0].host_table - runs[0].dev.data_ptr(), runs[1].host_table - runs[1].dev.data_ptr())
        assert np.array_equal(runs[0].image(), runs[1].image())


# ------------------------------------ 6. pass-through, stats, kernel names ----
@pytest.mark.parametrize("repair", [False, True])
@pytest.mark.parametrize("code", MAIN)
def test_equal_lengths_are_the_equal_length_call(code, repair):
    f = fec(code)
    S, stripes = 4112, 3
    P = pool(code, [S] * stripes)
    er = flags_cycle(P, 0, seed=5)
    stats = (f.STAT_SCRUB_LENS_LAUNCHES, f.STAT_CHECK_STRIPES, f.STAT_REPAIR_CHECKED)
    before = [f.stat(w) for w in stats]
    a = LensRun(P, er, repair=repair)
    a.flip(1, a.present(1)[0], 4100)
    a.run(f, torch, "pass-through")
    mid = [f.stat(w) for w in stats]
    # the equal-length call itself, on the same image
    b = LensRun(P, er, repair=repair)
    b.flip(1, b.present(1)[0], 4100)
    b.expect().upload(torch)
    if repair:
        f.reconstruct_checked_ptrs(b.table.data_ptr(), S, stripes, b.flags(), b.first_bad.data_ptr())
    else:
        f.verify_ptrs(b.table.data_ptr(), S, stripes, b.first_bad.data_ptr(), erased=b.flags())
    f.sync()
    assert np.array_equal(b.verdicts(), a.verdicts()) and np.array_equal(a.image(), b.image())
    after = [f.stat(w) for w in stats]
    assert mid[0] == before[0] == after[0], "an equal-length call ran the per-stripe-length kernels"
    assert [m - b0 for m, b0 in zip(mid, before)] == [x - m for x, m in zip(after, mid)], "not the same stats"


@pytest.mark.parametrize("repair", [False, True])
@pytest.mark.parametrize("code", MAIN)
def test_mixed_call_stats(code, repair):
    f = fec(code)
    P = pool(code, [4112, 0, 16, 5000, 0, 17, 1])
    er = np.zeros((P.stripes, P.n), dtype=np.uint8)
    er[0, 1] = 1               # degraded, has bytes
    er[1, 0] = 1               # degraded, no bytes: counted nowhere
    er[3, :P.m] = 1            # saturated
    er[4, :P.m] = 1            # saturated, no bytes
    er[5, [0, P.n - 1]] = 1    # degraded (saturated when m is 2)
    stats = (f.STAT_SCRUB_LENS_LAUNCHES, f.STAT_CHECK_STRIPES, f.STAT_REPAIR_CHECKED)
    before = [f.stat(w) for w in stats]
    run = LensRun(P, er, repair=repair)
    got = run.run(f, torch, "mixed")
    assert (got == CLEAN).all()
    e = er.sum(axis=1)
    live = np.array(P.lens) > 0
    checked = 0 if repair else int((live & (e > 0) & (e < P.m)).sum())
    repaired = int((live & (e > 0)).sum()) if repair else 0
    assert [f.stat(w) - b for w, b in zip(stats, before)] == [1, checked, repaired]


@pytest.mark.parametrize("code", sorted(CODES))
def test_kernel_names(code):
    f = fec(code)
    assert f.kernel_name(14) == VERIFY_NAME[code] + "_lens"
    assert f.kernel_name(15) == f"check_K{JOB_K[code]}_MG4_B256_ptrs_lens"
    assert f.kernel_name(16) == f"repair_K{JOB_K[code]}_MG4_B256_ptrs_lens"
    assert f.kernel_name(2) == VERIFY_NAME[code]


def test_no_parity_is_clean():
    """RS(4,4): every stripe clean, nothing read or written, any flag too many."""
    f = fec("rs4_4")
    P = pool("rs4_4", [4112, 0, 17, 5000])
    for repair in (False, True):
        run = LensRun(P, repair=repair)
        run.flip(0, 2, 5)
        got = run.run(f, torch, "m == 0")
        assert got.tolist() == [CLEAN] * 4
        one = np.zeros((4, 4), dtype=np.uint8)
        one[1, 2] = 1  # in the zero-length stripe
        run.upload(torch)
        with pytest.raises(rsmi.NotEnoughShares):
            if repair:
                f.reconstruct_checked_ptrs_lens(run.table.data_ptr(), P.lens, 4, one.tobytes(), run.first_bad.data_ptr())
            else:
                f.verify_ptrs_lens(run.table.data_ptr(), P.lens, 4, run.first_bad.data_ptr(), erased=one.tobytes())
        f.sync()
        run.check("m == 0, refused", want=run.cur)
        assert run.verdicts().tolist() == [SENTINEL] * 4


# ----------------------------------------------------------- 7. refusals ----
@pytest.mark.parametrize("repair", [False, True])
def test_refusals_write_nothing(repair):
    lib = rsmi.load()
    f = fec("rs10_14")
    P = pool("rs10_14", [4112, 0, 17])
    er = np.zeros((3, P.n), dtype=np.uint8)
    er[0, [0, 5, 10, 13]] = 1
    er[2, 3] = 1
    run = LensRun(P, er, repair=repair)
    run.flip(2, 0, 3)
    run.upload(torch)
    tp, fbp = run.table.data_ptr(), run.first_bad.data_ptr()
    fn = lib.rs_reconstruct_checked_ptrs_lens if repair else lib.rs_verify_ptrs_lens
    max_len = ((1 << 28) - 1) * 16

    def call(table=tp, lens=P.lens, stripes=3, flags=er, fb=fbp, h=f._h):
        buf = ctypes.c_char_p(flags.tobytes()) if flags is not None else None
        arr = (ctypes.c_size_t * len(lens))(*lens) if lens is not None else None
        return fn(h, table, arr, stripes, ctypes.cast(buf, ctypes.c_void_p), fb, None)

    assert call(h=None) == rsmi.RS_EINVAL
    assert call(lens=None) == rsmi.RS_EINVAL
    assert call(table=None) == rsmi.RS_EINVAL
    assert call(table=tp + 4) == rsmi.RS_EINVAL
    assert call(fb=None) == rsmi.RS_EINVAL
    assert call(fb=fbp + 2) == rsmi.RS_EINVAL
    assert call(stripes=1 << 32) == rsmi.RS_EINVAL
    if repair:
        assert call(flags=None) == rsmi.RS_EINVAL
    assert call(lens=[4112, max_len + 1, 17]) == rsmi.RS_EINVAL       # 2^28 columns
    assert call(lens=[4112, 0, 1 << 40]) == rsmi.RS_EINVAL
    # more than 2^31 - 1 blocks in all: 2,048 intact stripes of 2^20 blocks each
    many = np.zeros((2048, P.n), dtype=np.uint8)
    assert call(lens=[max_len] * 2048, stripes=2048, flags=many) == rsmi.RS_EINVAL
    # more than m erasures: in a stripe with bytes, and in the zero-length one
    for s in (2, 1):
        too_many = er.copy()
        too_many[s, [1, 2, 4, 6, 8]] = 1
        assert call(flags=too_many) == rsmi.RS_ENOT_ENOUGH
    with pytest.raises(rsmi.RSError):
        f.verify_ptrs_lens(tp, [16, 17], 3, fbp)  # one length per stripe
    # empty calls: RS_OK, nothing written
    assert call(stripes=0, lens=None, flags=None, fb=None, table=None) == rsmi.RS_OK
    assert call(lens=[0, 0, 0]) == rsmi.RS_OK
    f.sync()
    run.check("refused calls", want=run.cur)
    assert run.verdicts().tolist() == [SENTINEL] * 3


# ------------------------------------------------------------ 8. sharing ----
def test_device_set():
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert fs.kernel_name(15) == "check_K10_MG4_B256_ptrs_lens"
    P = pool("rs10_14", [5000, 0, 17, 4096])
    er = flags_cycle(P, 1, seed=9)
    for repair in (False, True):
        before = fs.stat(fs.STAT_SCRUB_LENS_LAUNCHES)
        run = LensRun(P, er, repair=repair)
        run.flip(2, run.survivors(2)[1], 16)
        assert run.run(fs, torch, "device set").tolist() == [CLEAN, CLEAN, 16, CLEAN]
        assert fs.stat(fs.STAT_SCRUB_LENS_LAUNCHES) - before == 1  # summed over the members
    fs.close()


def test_two_threads_one_context():
    f = fec("rs10_14")
    pools = [pool("rs10_14", [5000, 17, 0, 4112]), pool("rs10_14", [1, 3 * 4096 + 40, 16])]  # built ahead of the threads
    runs = []
    for t, P in enumerate(pools):
        mine = []
        for rep in range(4):
            run = LensRun(P, flags_cycle(P, rep, seed=10 * t + rep), repair=rep % 2 == 1, seed=rep)
            damage(run, rep % P.stripes, rep, rep)
            mine.append(run.expect())
        runs.append(mine)
    errors = []

    def work(t):
        try:
            for rep, run in enumerate(runs[t]):
                got = run.call(f, torch)
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

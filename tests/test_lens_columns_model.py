"""CPU: the host model of rs_correct_columns_ptrs_lens (tests/lens_columns.py)
against a plain-Python engine that applies the call's contract stripe by
stripe, with the oracle's decode_correct on EVERY byte column below the
stripe's length -- where the model only looks at the columns it damaged and
takes the pristine bytes for damage within the radius.  Small codes, lengths
from [16, 1, 17, 0].  What tests/test_store_model.py does for the store
driver, this does for the model the GPU tests of the column scrub rely on."""
import numpy as np
import pytest

from lens_columns import OK, TOO_MANY, ColumnRun, oracle_column
from lens_pool import LensPool, deal, oracle_codeword, rebuild_choice, windows
from strided_image import r16

CODES = [(4, 6), (3, 7)]
MIX = [16, 1, 17, 0]


def engine(run):
    """(image, status, counts) of one call on run.cur: a stripe whose present
    shards lie on one codeword below its length is left alone; another one
    without a radius fails unwritten; otherwise every column below the length
    is decoded on its own."""
    P = run.P
    image = run.cur.copy()
    status = [OK] * P.stripes
    counts = np.zeros((P.stripes, P.n), dtype=np.int64)
    for s, S in enumerate(P.lens):
        present = run.present(s)
        if S == 0 or P.m == 0:
            continue
        chosen = rebuild_choice(P.k, P.n, run.er[s])
        word = oracle_codeword(P.k, P.n, [(i, image[run.at(s, i):run.at(s, i) + S].tobytes()) for i in chosen])
        if all(np.array_equal(image[run.at(s, i):run.at(s, i) + S], word[i]) for i in present):
            continue
        if len(present) - P.k < 2:
            status[s] = TOO_MANY
            continue
        for off in range(S):
            col = [(i, int(image[run.at(s, i) + off])) for i in present]
            rc, cw = oracle_column(P.k, P.n, col)
            if rc != 0:
                status[s] = TOO_MANY
                continue
            for i, b in col:
                if cw[i] != b:
                    image[run.at(s, i) + off] = cw[i]
                    counts[s, i] += 1
    return image, status, counts


def same(run, what):
    run.expect()
    image, status, counts = engine(run)
    assert status == run.status, (what, run.P.lens, status, run.status)
    assert np.array_equal(counts, run.counts), (what, run.P.lens, counts.tolist(), run.counts.tolist())
    bad = np.flatnonzero(image != run.want)
    assert bad.size == 0, (what, run.P.lens, bad[:8].tolist())
    jobs = [s for s in range(run.P.stripes) if counts[s].sum() > 0 or
            (status[s] == TOO_MANY and len(run.present(s)) - run.P.k >= 2)]
    assert run.jobs() == jobs, (what, run.jobs(), jobs)
    return status


def pools(k, n, stripes):
    for w in range(windows(MIX, stripes)):
        for longest in (None, "first", "last"):
            lens = deal(MIX, stripes, seed=k + 7 * n + stripes, window=w, longest=longest)
            yield LensPool(k, n, lens, seed=1000 * k + 10 * n + w)


def erasures(P, shift, seed, most):
    """(s + shift) mod (most + 1) erasures in stripe s."""
    rng = np.random.default_rng(seed)
    er = np.zeros((P.stripes, P.n), dtype=np.uint8)
    for s in range(P.stripes):
        er[s, rng.choice(P.n, size=(s + shift) % (most + 1), replace=False)] = 1
    return er


@pytest.mark.parametrize("k,n", CODES)
@pytest.mark.parametrize("stripes", [2, 3, 4])
def test_damage_within_the_radius(k, n, stripes):
    """Every stripe that has a radius returns to the pristine bytes; erasure
    counts 0 .. m - 2 cycle, so every stripe has one."""
    for P in pools(k, n, stripes):
        for shift in range(P.m - 1):
            er = erasures(P, shift, seed=shift, most=P.m - 2)
            run = ColumnRun(P, er, seed=shift)
            rng = np.random.default_rng(50 + shift)
            for s in range(stripes):
                run.scatter(s, rng, extra=3)
            status = same(run, f"RS({k},{n}) shift {shift}")
            assert status == [OK] * stripes
            assert np.array_equal(run.want, run.base)
            assert run.jobs() == [s for s in range(stripes) if P.lens[s] > 0]


@pytest.mark.parametrize("k,n", CODES)
def test_damage_at_and_beyond_the_length_stays(k, n):
    for P in pools(k, n, 4):
        run = ColumnRun(P)
        for s, S in enumerate(P.lens):
            run.flip(s, s % P.n, S, 0x01)           # the pad of the last column when S % 16 != 0
            run.flip(s, (s + 1) % P.n, r16(S), 0xFF)  # behind the columns the stripe has
            if s % 2 == 0 and S > 0:
                run.flip(s, (s + 2) % P.n, S - 1, 0x40)
        status = same(run, f"RS({k},{n}) beyond the length")
        assert status == [OK] * 4
        for s, S in enumerate(P.lens):
            kept = [run.at(s, s % P.n) + S, run.at(s, (s + 1) % P.n) + r16(S)]
            assert all(run.want[o] == run.cur[o] != P.pristine[o] for o in kept)
            assert run.counts[s].sum() == (1 if s % 2 == 0 and S > 0 else 0)


@pytest.mark.parametrize("k,n", CODES)
def test_beyond_the_radius_and_without_one(k, n):
    """radius + 1 errors in one column of a stripe among correctable columns:
    whatever the oracle does with that column; and stripes with r - k < 2."""
    outcomes = set()
    for P in pools(k, n, 3):
        for seed in range(6):
            rng = np.random.default_rng(seed)
            # stripe 0: r - k == 1, stripe 1: r == k, stripe 2: everything present
            er = np.zeros((3, P.n), dtype=np.uint8)
            er[0, rng.choice(P.n, size=P.m - 1, replace=False)] = 1
            er[1, rng.choice(P.n, size=P.m, replace=False)] = 1
            run = ColumnRun(P, er, seed=seed)
            for s in (0, 1):
                if P.lens[s]:
                    run.flip(s, run.present(s)[seed % P.k], int(rng.integers(P.lens[s])), 0x11)
            S = P.lens[2]
            if S:
                off = int(rng.integers(S))
                for i in rng.choice(P.n, size=run.radius(2) + 1, replace=False):
                    run.flip(2, int(i), off, int(rng.integers(1, 256)))
                if S > 1:
                    run.flip(2, seed % P.n, (off + 1) % S, 0x80)
            status = same(run, f"RS({k},{n}) seed {seed}")
            assert status[0] == (TOO_MANY if P.lens[0] else OK)  # seen, not locatable
            assert status[1] == OK                               # nothing to compare
            outcomes.add(status[2])
            for s in (0, 1):  # neither is written
                for i in run.present(s):
                    o = run.at(s, i)
                    assert np.array_equal(run.want[o:o + P.row_bytes], run.cur[o:o + P.row_bytes])
    assert TOO_MANY in outcomes

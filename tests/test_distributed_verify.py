"""CPU: the verify option of the survivor-gather reconstruct
(rsmi/distributed.py reconstruct_owned / run_step) with a stand-in engine that
records its calls: rs_verify_ptrs runs first, over the same table window, with
the erasure flags plus a flag for every shard the table does not hold; a stripe
that is not clean raises before anything is regenerated; the default calls
nothing new."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import rsmi.distributed as rd  # noqa: E402

K, N, S, STRIPES = 10, 14, 64, 23
CLEAN = 0xFFFFFFFF


class FakeFec:
    def __init__(self, verdicts=None):
        self.calls, self.verdicts = [], verdicts or {}

    def verify_ptrs(self, table_ptr, shard_len, stripes, first_bad_ptr, erased=None, stream=0):
        self.calls.append(("verify", table_ptr, shard_len, stripes, erased, stream))
        fb = np.full(stripes, CLEAN, dtype=np.uint32)
        for j, off in self.verdicts.items():
            fb[j] = off
        ctypes.memmove(first_bad_ptr, fb.ctypes.data, fb.nbytes)

    def sync(self, stream=0):
        self.calls.append(("sync", stream))

    def reconstruct_ptrs(self, table_ptr, shard_len, stripes, erased, stream=0):
        self.calls.append(("reconstruct", table_ptr, shard_len, stripes, erased, stream))


def setup(chunks=1):
    rng = np.random.default_rng(5)
    er = np.zeros((STRIPES, N), dtype=np.uint8)
    for s in range(STRIPES):
        er[s, rng.choice(N, size=int(rng.integers(0, N - K + 1)), replace=False)] = 1
    plan = rd.plan_exchange(er, K, N, 0, 2, S, chunks=chunks)
    table = torch.zeros(len(plan.owned) * N, dtype=torch.int64)
    return er[plan.owned], plan, table


def test_default_calls_only_the_reconstruct():
    er, plan, table = setup()
    f = FakeFec()
    rd.reconstruct_owned(f, plan, table, er, S, 3)
    assert [c[0] for c in f.calls] == ["reconstruct"]


def test_verify_runs_first_with_absent_shards_flagged():
    er, plan, table = setup(chunks=2)
    for c in range(len(plan.chunks)):
        f = FakeFec()
        lo, hi = plan.chunks[c].lo, plan.chunks[c].hi
        rd.reconstruct_owned(f, plan, table, er, S, 3, c, verify=True)
        assert [x[0] for x in f.calls] == ["verify", "sync", "reconstruct"]
        v, r = f.calls[0], f.calls[2]
        assert v[1] == r[1] == table.data_ptr() + lo * N * 8 and v[2:4] == r[2:4] == (S, hi - lo) and v[5] == 3
        flags = np.frombuffer(v[4], dtype=np.uint8).reshape(hi - lo, N)
        want = (er[lo:hi] != 0) | (plan.kind[lo:hi] == rd.UNUSED)
        assert np.array_equal(flags != 0, want)
        assert r[4] == er[lo:hi].tobytes()  # the reconstruct keeps the stripes' own flags
        # exactly the k shards the table holds stay unflagged
        assert ((flags == 0).sum(axis=1) == K).all()


def test_a_dirty_stripe_raises_before_the_reconstruct():
    er, plan, table = setup()
    f = FakeFec({2: 17, 5: 0})
    with pytest.raises(rd.InconsistentSurvivors) as e:
        rd.reconstruct_owned(f, plan, table, er, S, verify=True)
    assert e.value.stripes == [(2, 17), (5, 0)]
    assert "reconstruct" not in [c[0] for c in f.calls]

"""The pattern-cache protocol through the entry points other than
rs_reconstruct_stripes (rsmi.cpp with_patterns).

tests/test_gpu_concurrency.py reaches the protocol -- lookup under the shared
lock; on a miss the exclusive lock, eviction past the cap, the build, then
the launch -- only through rs_reconstruct_stripes.  These tests drive the same
eviction and failed-build rollback through its other callers:
rs_read_stripes, rs_verify_degraded and the fused path of rs_update_degraded.
They are built like their neighbours there (its _fec_env and _erase), over a
dense RS(10,14) image of 12 stripes with 4 KiB shards; every expectation is
the oracle's and every comparison bit-exact.  The calls run on the NULL stream
with no host sync before the device work that follows them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from oracle import oracle  # noqa: E402
from test_gpu_concurrency import _erase, _fec_env  # noqa: E402

_PK, _PN, _PS, _PST = 10, 14, 4096, 12
_PM = _PN - _PK


def _fresh_erasures(rng):
    """(flags [stripes][n], first [stripes]): 1..4 erased shards per stripe,
    the data shard first[s] among them."""
    er = np.zeros((_PST, _PN), dtype=np.uint8)
    first = rng.integers(0, _PK, size=_PST)
    for s in range(_PST):
        er[s, first[s]] = 1
        rest = [i for i in range(_PN) if i != first[s]]
        er[s, rng.choice(rest, size=int(rng.integers(0, _PM)), replace=False)] = 1
    return er, first


class _Entry:
    """One entry point over the image.  prepare() stages the storage (erased
    slots zeroed) and the call's inputs and destinations, call() makes the
    call, check() compares its results, untouched() says whether storage and
    destinations are as prepare() left them, patterns() is the number of
    distinct erasure sets the call looks up and planned() the amount each of
    its counters moves per call."""

    def __init__(self, f, seed):
        self.f = f
        self.E = oracle.fec_matrix(_PK, _PN)
        hd = oracle.splitmix_bytes(_PST * _PK * _PS, seed).copy()
        hp = oracle.encode_batch(self.E, _PK, _PN, hd, _PS, _PST)
        self.hd, self.hp = hd.reshape(_PST, _PK, _PS), hp.reshape(_PST, _PM, _PS)
        self.d0, self.p0 = torch.from_numpy(hd).cuda(), torch.from_numpy(hp).cuda()
        self.data, self.parity = self.d0.clone(), self.p0.clone()
        self.rng = np.random.default_rng(seed)
        self.calls = 0

    def stage(self, er, first):
        self.er, self.first = er, first
        self.data.copy_(self.d0)
        self.parity.copy_(self.p0)
        _erase(self.data, self.parity, er, _PK, _PM, _PS, _PST)
        self.before = (self.data.clone(), self.parity.clone())

    def args(self):
        return (self.data.data_ptr(), _PK * _PS, self.parity.data_ptr(), _PM * _PS, _PS, _PS, _PST)

    def storage_unchanged(self):
        return torch.equal(self.data, self.before[0]) and torch.equal(self.parity, self.before[1])

    def patterns(self):
        return len({row.tobytes() for row in self.er})


class _ReadEntry(_Entry):
    """rs_read_stripes: every erased shard of every stripe and one present
    shard of it."""

    def prepare(self, er, first):
        self.stage(er, first)
        self.want = []
        for s in range(_PST):
            self.want += [(s, int(i)) for i in np.flatnonzero(er[s])]
            self.want.append((s, int(self.rng.choice(np.flatnonzero(er[s] == 0)))))
        self.dst = torch.full((len(self.want), _PS), 0x5A, dtype=torch.uint8, device="cuda")

    def call(self):
        self.calls += 1
        reads = [(s, i, self.dst.data_ptr() + q * _PS) for q, (s, i) in enumerate(self.want)]
        self.f.read_stripes(*self.args(), self.er.tobytes(), reads)

    def check(self):
        full = np.concatenate([self.hd, self.hp], axis=1)
        ref = np.stack([full[s, i] for s, i in self.want])
        assert torch.equal(self.dst.cpu(), torch.from_numpy(ref))
        assert self.storage_unchanged()

    def untouched(self):
        return bool((self.dst == 0x5A).all()) and self.storage_unchanged()

    def planned(self):
        return {self.f.STAT_READ_REGENERATED: int(self.er.sum()), self.f.STAT_READ_COPIED: _PST}


class _VerifyEntry(_Entry):
    """rs_verify_degraded: the clean image, then one flipped byte in a
    present shard of one stripe.  A stripe with m erasures has no redundancy
    left to check; the others look up their flags plus the m - e
    lowest-numbered present parity shards (check_plan.hpp)."""

    def prepare(self, er, first):
        self.stage(er, first)
        self.jobs = [s for s in range(_PST) if er[s].sum() < _PM]
        assert self.jobs
        self.fb = torch.full((_PST,), 7, dtype=torch.int32, device="cuda")

    def call(self):
        self.calls += 1
        self.f.verify_degraded(*self.args(), self.er.tobytes(), self.fb.data_ptr())

    def verdicts(self):
        return self.fb.cpu().numpy().view(np.uint32)

    def check(self):
        want = np.full(_PST, rsmi.RS_VERIFY_CLEAN, dtype=np.uint32)
        assert (self.verdicts() == want).all()
        assert self.storage_unchanged()
        s = int(self.rng.choice(self.jobs))
        i = int(self.rng.choice(np.flatnonzero(self.er[s] == 0)))
        off = int(self.rng.integers(0, _PS))
        slot = self.data.view(_PST, _PK, _PS)[s, i] if i < _PK else self.parity.view(_PST, _PM, _PS)[s, i - _PK]
        slot[off] ^= 0x40
        self.fb.fill_(7)
        self.call()
        want[s] = off
        assert (self.verdicts() == want).all(), (s, i, off)
        slot[off] ^= 0x40
        assert self.storage_unchanged()

    def untouched(self):
        return bool((self.fb == 7).all()) and self.storage_unchanged()

    def patterns(self):
        sets = set()
        for s in self.jobs:
            x = self.er[s].copy()
            left = _PM - int(x.sum())
            for i in range(_PK, _PN):
                if not x[i] and left > 0:
                    x[i] = 1
                    left -= 1
            sets.add(x.tobytes())
        return len(sets)

    def planned(self):
        return {self.f.STAT_CHECK_STRIPES: len(self.jobs)}


class _UpdateEntry(_Entry):
    """rs_update_degraded (m = 4: the fused path): every stripe changes one
    present data shard and its erased data shard first[s]."""

    def prepare(self, er, first):
        self.stage(er, first)
        self.ups = []
        for s in range(_PST):
            self.ups.append((s, int(self.rng.choice(np.flatnonzero(er[s, :_PK] == 0)))))
            self.ups.append((s, int(first[s])))
        self.src_h = self.rng.integers(0, 256, size=(len(self.ups), _PS), dtype=np.uint8)
        self.src = torch.from_numpy(self.src_h).cuda()

    def call(self):
        self.calls += 1
        ups = [(s, i, self.src.data_ptr() + q * _PS) for q, (s, i) in enumerate(self.ups)]
        self.f.update_degraded(*self.args(), self.er.tobytes(), ups)

    def check(self):
        new = self.hd.copy()
        want_d = self.before[0].cpu().numpy().reshape(_PST, _PK, _PS).copy()
        for q, (s, i) in enumerate(self.ups):
            new[s, i] = self.src_h[q]
            if not self.er[s, i]:
                want_d[s, i] = self.src_h[q]
        par = oracle.encode_batch(self.E, _PK, _PN, new.reshape(-1), _PS, _PST).reshape(_PST, _PM, _PS)
        was_p = self.before[1].cpu().numpy().reshape(_PST, _PM, _PS)
        want_p = np.where(self.er[:, _PK:, None] != 0, was_p, par)
        assert torch.equal(self.parity.cpu(), torch.from_numpy(want_p.reshape(-1)))
        assert torch.equal(self.data.cpu(), torch.from_numpy(want_d.reshape(-1)))
        assert torch.equal(self.src.cpu(), torch.from_numpy(self.src_h))

    def untouched(self):
        return torch.equal(self.src.cpu(), torch.from_numpy(self.src_h)) and self.storage_unchanged()

    def planned(self):
        return {self.f.STAT_UPDATE_DEGRADED: _PST, self.f.STAT_UPDATE_ABSORBED: _PST}


_ENTRIES = [_ReadEntry, _VerifyEntry, _UpdateEntry]
_ENTRY_IDS = ["read_stripes", "verify_degraded", "update_degraded"]


@pytest.mark.parametrize("entry", _ENTRIES, ids=_ENTRY_IDS)
def test_pattern_cache_eviction_through_other_entry_points(entry):
    """With a pattern cap of 8, six rounds of fresh erasure sets for all 12
    stripes make every round's first call miss, take the exclusive lock and
    evict (rsmi.cpp with_patterns).  Every result stays exact, the cache is
    evicted again and again, and the call's own counters move by the planned
    amounts."""
    f = _fec_env(_PK, _PN, RSMI_PATTERN_CAP="8")
    op = entry(f, 31)
    rng = np.random.default_rng(32)
    for rnd in range(6):
        op.prepare(*_fresh_erasures(rng))
        stats = {w: f.stat(w) for w in op.planned()}
        calls = op.calls
        op.call()
        op.check()
        for w, d in op.planned().items():
            assert f.stat(w) - stats[w] == d * (op.calls - calls), (rnd, w)
    assert f.pattern_evictions() >= 4
    f.close()


@pytest.mark.parametrize("entry", _ENTRIES, ids=_ENTRY_IDS)
def test_failed_pattern_build_rolls_back_through_other_entry_points(entry):
    """test_failed_pattern_build_rolls_back for the other callers of the
    protocol: the context's first build fails (RSMI_TEST_FAIL_FLUSH=1), the
    call reports RS_ENOMEM, the cache is empty again and -- nothing is launched
    before the build -- storage and destinations are as they were.  The same
    call then succeeds through the exclusive path (which builds the patterns)
    and through the shared path (which finds them)."""
    f = _fec_env(_PK, _PN, RSMI_TEST_FAIL_FLUSH="1")
    op = entry(f, 41)
    er, first = _fresh_erasures(np.random.default_rng(42))
    op.prepare(er, first)
    with pytest.raises(rsmi.RSError) as ei:
        op.call()
    assert ei.value.code == rsmi.RS_ENOMEM
    assert f.pattern_count() == 0
    assert op.untouched()
    for _ in range(2):
        op.prepare(er, first)
        op.call()
        op.check()
    assert f.pattern_count() == op.patterns()
    f.close()

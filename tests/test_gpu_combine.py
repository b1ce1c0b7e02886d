"""GPU: rs_combine -- caller-chosen GF(2^8) combinations of device buffers
(rs_combine_kernel) -- and rs_pattern_survivors.

The expected bytes always come from the oracle (oracle.matmul_stripe,
oracle.encode_batch) or from the pristine payload, never from the engine, and
every comparison is bit-exact.  Destinations sit in buffers of random bytes
with guard bands: after a call the len bytes of every dst hold the expected
bytes, everything outside [dst, dst + round_up(len, 16)) is byte-identical to
before, and so is every source; only the <= 15 padding bytes behind len of a
written dst are exempt.
"""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the RSMI_ITERS child of test_combine_multi_iteration_child
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "noise-erasurecode-plugin_amd"), os.path.join(_root, "tests")):
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from oracle import oracle  # noqa: E402

# one column | exactly one 4 KiB block chunk | a chunk plus one column (the
# second block is all tail lanes but one) | not a multiple of 16
SHAPES = [16, 4096, 4112, 5000]
# 199 | 200: the most sources whose tables fit the LDS with row groups of 16
# (199 * 328 = 65,272 bytes), and the first call that takes row groups of 8
# instead -- the only LDS-driven switch (256 sources fit with row groups of 8
# and of 4).  Both sides matter for nout 16, 17 and 40.
NSRC = [1, 2, 3, 10, 64, 199, 200, 256]
# MG4 | MG4 | MG8, partial last sub-step | MG16 | two row groups, the second of
# one row | three row groups of 16 (five of 8 past the switch)
NOUT = [1, 4, 5, 16, 17, 40]
MAXOUT = 40
ITERS_S = 3 * 4096 + 40


def r16(x):
    return (x + 15) // 16 * 16


_FECS = {}


def fec(k=10, n=14):
    if (k, n) not in _FECS:
        _FECS[(k, n)] = rsmi.FEC(k, n, device=0)
    return _FECS[(k, n)]


class Sources:
    """256 source buffers of S bytes on the host (read-only) and the device,
    16 random bytes between neighbours."""

    def __init__(self, S, seed):
        self.S, self.slot = S, r16(S) + 16
        rng = np.random.default_rng(seed)
        self.host = rng.integers(0, 256, size=256 * self.slot, dtype=np.uint8)
        self.host.setflags(write=False)
        self.dev = torch.from_numpy(self.host.copy()).cuda()

    def ptr(self, c):
        return self.dev.data_ptr() + c * self.slot

    def shard(self, c):
        return self.host[c * self.slot:c * self.slot + self.S]

    def check(self):
        assert np.array_equal(self.dev.cpu().numpy(), self.host), "a source changed"


_SOURCES = {}


def sources(S):
    if S not in _SOURCES:
        _SOURCES[S] = Sources(S, seed=S * 31 + 7)
    return _SOURCES[S]


class Dst:
    """`rows` destination buffers of S bytes inside random bytes: a 64-byte
    guard band in front and 32 random bytes behind round_up(S, 16) of each."""

    def __init__(self, rows, S, seed):
        self.S, self.slot = S, r16(S) + 32
        rng = np.random.default_rng(seed)
        self.pristine = rng.integers(0, 256, size=64 + rows * self.slot, dtype=np.uint8)
        self.pristine.setflags(write=False)
        self.pristine_dev = torch.from_numpy(self.pristine.copy()).cuda()
        self.dev = self.pristine_dev.clone()

    def reset(self):
        self.dev.copy_(self.pristine_dev)

    def off(self, r):
        return 64 + r * self.slot

    def ptr(self, r):
        return self.dev.data_ptr() + self.off(r)

    def old(self, r):
        return self.pristine[self.off(r):self.off(r) + self.S]

    def check(self, expected, what=""):
        """expected: {row: its S bytes}; every other byte as in pristine."""
        want = self.pristine.copy()
        loose = np.zeros(len(want), dtype=bool)
        for r, v in expected.items():
            o = self.off(r)
            want[o:o + self.S] = v
            loose[o + self.S:o + r16(self.S)] = True
        got = self.dev.cpu().numpy()
        bad = np.flatnonzero((got != want) & ~loose)
        assert bad.size == 0, (what, bad[:8].tolist(), bad.size)


def matrix(rng, nout, nsrc, zero_row):
    """Random coefficients with zeros and ones sprinkled in and, if asked, an
    all-zero row."""
    M = rng.integers(2, 256, size=(nout, nsrc), dtype=np.uint8)
    flat = M.reshape(-1)
    some = rng.permutation(flat.size)
    few = max(1, flat.size // 6)
    if flat.size >= 2:
        flat[some[:few]] = 1
    if flat.size >= 3:
        flat[some[few:2 * few]] = 0
    if zero_row is not None:
        M[zero_row] = 0
    return M


def matrices(rng, nout, nsrc):
    """The matrices of one shape: with zeros, ones and an all-zero row in the
    middle; a single row cannot be both, so nout = 1 gets two matrices."""
    if nout == 1:
        return [matrix(rng, 1, nsrc, None), matrix(rng, 1, nsrc, 0)]
    return [matrix(rng, nout, nsrc, nout // 2)]


def check_cross(f, S, nsrcs, nouts):
    """Every (nsrc, nout) of the lists as a call of one job, overwriting rows
    [0, nout) and accumulating into rows [MAXOUT, MAXOUT + nout)."""
    src = sources(S)
    d = Dst(2 * MAXOUT, S, seed=S + 1)
    rng = np.random.default_rng(S * 13 + 5)
    jobs0, rows0 = f.stat(f.STAT_COMBINE_JOBS), f.stat(f.STAT_COMBINE_ROWS)
    jobs = rows = 0
    for nsrc, nout in itertools.product(nsrcs, nouts):
        ids = [int(c) for c in rng.permutation(256)[:nsrc]]
        shards = [src.shard(c) for c in ids]
        for M in matrices(rng, nout, nsrc):
            prod = oracle.matmul_stripe(M, shards)
            d.reset()
            sp = [src.ptr(c) for c in ids]
            f.combine([(sp, [d.ptr(r) for r in range(nout)], M.tobytes(), 0)], S)
            f.combine([(sp, [d.ptr(MAXOUT + r) for r in range(nout)], M.tobytes(), 1)], S)
            f.sync()
            expected = {r: prod[r] for r in range(nout)}
            expected.update({MAXOUT + r: d.old(MAXOUT + r) ^ prod[r] for r in range(nout)})
            d.check(expected, f"S {S} nsrc {nsrc} nout {nout}")
            if not M[nout // 2].any():  # the all-zero row: zeroes when overwriting, a no-op when accumulating
                assert not expected[nout // 2].any()
                assert np.array_equal(expected[MAXOUT + nout // 2], d.old(MAXOUT + nout // 2))
            jobs, rows = jobs + 2, rows + 2 * nout
    src.check()
    assert f.stat(f.STAT_COMBINE_JOBS) - jobs0 == jobs
    assert f.stat(f.STAT_COMBINE_ROWS) - rows0 == rows


@pytest.mark.parametrize("S", SHAPES)
def test_combine_cross(S):
    check_cross(fec(), S, NSRC, NOUT)


def check_multi_job(f, S, count, seed):
    """One call of `count` jobs whose nsrc, nout and mode differ per job; the
    jobs draw their sources from one small set, so many are shared, and some
    jobs list a source twice."""
    src = sources(S)
    rng = np.random.default_rng(seed)
    shapes = [(int(rng.choice([1, 2, 3, 10, 64])), int(rng.choice([1, 4, 5, 16, 17, 40])), int(rng.integers(0, 2)))
              for _ in range(count)]
    d = Dst(sum(nout for _, nout, _ in shapes), S, seed=seed + 1)
    jobs, expected, row = [], {}, 0
    for nsrc, nout, acc in shapes:
        ids = [int(c) for c in rng.integers(0, 70, size=nsrc)]  # with repeats
        M = matrix(rng, nout, nsrc, nout // 2 if nout > 1 else None)
        prod = oracle.matmul_stripe(M, [src.shard(c) for c in ids])
        for r in range(nout):
            expected[row + r] = d.old(row + r) ^ prod[r] if acc else prod[r]
        jobs.append(([src.ptr(c) for c in ids], [d.ptr(row + r) for r in range(nout)], M.tobytes(), acc))
        row += nout
    jobs0, rows0 = f.stat(f.STAT_COMBINE_JOBS), f.stat(f.STAT_COMBINE_ROWS)
    f.combine(jobs, S)
    f.sync()
    d.check(expected, f"{count} jobs")
    src.check()
    assert f.stat(f.STAT_COMBINE_JOBS) - jobs0 == count
    assert f.stat(f.STAT_COMBINE_ROWS) - rows0 == row


@pytest.mark.parametrize("count", [1, 3, 37])
def test_combine_multi_job(count):
    check_multi_job(fec(), 4112, count, seed=100 + count)


class Stripes:
    """Stripes of RS(k, n) encoded by the oracle, stripe s with 1 + s % m
    erasures, on the device with random bytes in the erased slots."""

    def __init__(self, k, n, S, stripes, seed):
        self.k, self.n, self.m, self.S, self.stripes = k, n, n - k, S, stripes
        self.pitch = r16(S)
        self.E = oracle.fec_matrix(k, n)
        rng = np.random.default_rng(seed)
        self.payload = rng.integers(0, 256, size=(stripes, k, S), dtype=np.uint8)
        par = oracle.encode_batch(self.E, k, n, np.ascontiguousarray(self.payload).reshape(-1), S, stripes)
        self.shards = np.concatenate([self.payload, par.reshape(stripes, self.m, S)], axis=1)  # [stripes][n][S]
        self.erased = np.zeros((stripes, n), dtype=np.uint8)
        for s in range(stripes):
            self.erased[s, rng.choice(n, size=1 + s % self.m, replace=False)] = 1
        host = rng.integers(0, 256, size=(stripes, n, self.pitch), dtype=np.uint8)
        keep = self.erased == 0
        host[:, :, :S][keep] = self.shards[keep]
        self.host = host
        self.data = torch.from_numpy(np.ascontiguousarray(host[:, :k]).reshape(-1)).cuda()
        self.parity = torch.from_numpy(np.ascontiguousarray(host[:, k:]).reshape(-1)).cuda()

    def ptr(self, s, i):
        if i < self.k:
            return self.data.data_ptr() + (s * self.k + i) * self.pitch
        return self.parity.data_ptr() + (s * self.m + i - self.k) * self.pitch


def check_partial_sum_repair(f, k, n, S, holders, seed):
    """Every erased shard of every stripe as the XOR of `holders` partial
    sums: holder h multiplies its share of the survivors by their columns of
    the decode row; the first call overwrites the output, the later ones
    accumulate into it on the same stream."""
    L = Stripes(k, n, S, n - k, seed)
    wanted = [(s, int(i)) for s in range(L.stripes) for i in np.flatnonzero(L.erased[s])]
    out = Dst(len(wanted), S, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    calls = [[] for _ in range(holders)]
    row = 0
    for s in range(L.stripes):
        flags = L.erased[s].tobytes()
        rows, cnt = f.pattern_rows(flags)
        ids = f.pattern_survivors(flags)
        missing = [int(i) for i in np.flatnonzero(L.erased[s])]
        assert cnt == len(missing) and len(ids) == k and not any(L.erased[s, i] for i in ids)
        rows = np.frombuffer(rows, dtype=np.uint8).reshape(n - k, k)
        # a random split of the k columns into `holders` disjoint, non-empty sets
        cols = rng.permutation(k)
        cuts = sorted(int(c) for c in rng.choice(np.arange(1, k), size=holders - 1, replace=False))
        parts = np.split(cols, cuts)
        for t in range(cnt):
            for h, part in enumerate(parts):
                calls[h].append(([L.ptr(s, ids[c]) for c in part], [out.ptr(row)],
                                 bytes(rows[t, c] for c in part), int(h > 0)))
            row += 1
    for jobs in calls:
        f.combine(jobs, S)
    f.sync()
    out.check({r: L.shards[s, i] for r, (s, i) in enumerate(wanted)}, f"RS({k},{n - k}) {holders} holders")  # the pristine shards
    # ... and what rs_reconstruct_stripes writes for the same flags
    f.reconstruct_stripes(L.data.data_ptr(), k * L.pitch, L.parity.data_ptr(), (n - k) * L.pitch, L.pitch, S, L.stripes,
                          L.erased.tobytes())
    f.sync()
    got = out.dev.cpu().numpy()
    rec = np.concatenate([L.data.cpu().numpy().reshape(L.stripes, k, L.pitch),
                          L.parity.cpu().numpy().reshape(L.stripes, n - k, L.pitch)], axis=1)
    for r, (s, i) in enumerate(wanted):
        assert np.array_equal(got[out.off(r):out.off(r) + S], rec[s, i, :S]), (s, i)
    # the survivors were only read
    keep = L.erased == 0
    assert np.array_equal(rec[keep], L.host[keep])


@pytest.mark.parametrize("code,holders", [((10, 14), 2), ((10, 14), 3), ((64, 80), 2), ((64, 80), 3)])
def test_combine_partial_sum_repair(code, holders):
    check_partial_sum_repair(fec(*code), *code, 4112, holders, seed=code[0] * 10 + holders)


def survivors_rule(erased, k, n):
    """Rebuild's choice as documented: slot i holds shard i if it is present,
    otherwise the highest-numbered remaining parity."""
    spare = [i for i in range(n - 1, k - 1, -1) if not erased[i]]
    return [i if not erased[i] else spare.pop(0) for i in range(k)]


def test_pattern_survivors_is_the_documented_rule():
    f, k, n = fec(), 10, 14
    assert f.pattern_survivors(bytes(n)) == list(range(k))
    for e in (1, 2):
        for gone in itertools.combinations(range(n), e):
            flags = bytearray(n)
            for i in gone:
                flags[i] = 1
            assert f.pattern_survivors(bytes(flags)) == survivors_rule(flags, k, n), gone
    # four erasures are served, five are not
    assert f.pattern_survivors(bytes([1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 1])) == [12, 1, 2, 10, 4, 5, 6, 7, 8, 9]
    with pytest.raises(rsmi.NotEnoughShares):
        f.pattern_survivors(bytes([1, 1, 1, 1, 1] + [0] * 9))
    fs = rsmi.FEC(k, n, devices=[0, 0])
    assert fs.pattern_survivors(bytes([0, 1] + [0] * 12)) == [0, 13, 2, 3, 4, 5, 6, 7, 8, 9]
    fs.close()


def test_combine_parity_delta():
    """The update of one data shard per stripe in two halves: the data holder
    turns old and new contents into the m deltas E[k + r][c] * (old ^ new),
    the parity holder XORs them into the stored parity."""
    k, n, S, stripes = 10, 14, 5000, 3
    m, pitch = n - k, r16(S)
    f = fec(k, n)
    E = oracle.fec_matrix(k, n)
    rng = np.random.default_rng(61)
    payload = rng.integers(0, 256, size=(stripes, k, S), dtype=np.uint8)
    par = oracle.encode_batch(E, k, n, payload.reshape(-1), S, stripes).reshape(stripes, m, S)
    data_h = rng.integers(0, 256, size=(stripes, k, pitch), dtype=np.uint8)
    data_h[:, :, :S] = payload
    parity_h = rng.integers(0, 256, size=(stripes, m, pitch), dtype=np.uint8)
    parity_h[:, :, :S] = par
    changed = [(s, int(rng.integers(0, k))) for s in range(stripes)]
    new = Dst(stripes, S, seed=62)     # the new contents: only read
    delta = Dst(stripes * m, S, seed=63)
    data = torch.from_numpy(data_h.reshape(-1).copy()).cuda()
    parity = torch.from_numpy(parity_h.reshape(-1).copy()).cuda()
    data2, parity2 = data.clone(), parity.clone()
    first = [([data.data_ptr() + (s * k + c) * pitch, new.ptr(s)], [delta.ptr(s * m + r) for r in range(m)],
              bytes(int(E[k + r, c]) for r in range(m) for _ in range(2)), 0) for s, c in changed]
    second = [([delta.ptr(s * m + r)], [parity.data_ptr() + (s * m + r) * pitch], b"\x01", 1)
              for s in range(stripes) for r in range(m)]
    f.combine(first, S)
    f.combine(second, S)
    f.sync()
    new.check({}, "the new contents changed")
    assert np.array_equal(data.cpu().numpy(), data_h.reshape(-1)), "the data changed"
    updated = payload.copy()
    for s, c in changed:
        updated[s, c] = new.old(s)
    # the deltas themselves, from the oracle
    for s, c in changed:
        col = np.ascontiguousarray(E[k:, c]).reshape(m, 1)
        want = oracle.matmul_stripe(col, [payload[s, c] ^ new.old(s)])
        delta_want = {s * m + r: want[r] for r in range(m)}
        got = delta.dev.cpu().numpy()
        for r, v in delta_want.items():
            assert np.array_equal(got[delta.off(r):delta.off(r) + S], v), (s, r)
    ref = oracle.encode_batch(E, k, n, updated.reshape(-1), S, stripes).reshape(stripes, m, S)
    got_p = parity.cpu().numpy().reshape(stripes, m, pitch)
    assert np.array_equal(got_p[:, :, :S], ref), "parity is not the oracle's encode of the updated payload"
    # ... and what rs_update_stripes leaves on a clone
    f.update_stripes(data2.data_ptr(), k * pitch, parity2.data_ptr(), m * pitch, pitch, S, stripes,
                     [(s, c, new.ptr(s)) for s, c in changed])
    f.sync()
    assert np.array_equal(parity2.cpu().numpy().reshape(stripes, m, pitch)[:, :, :S], got_p[:, :, :S])


def test_combine_refusals_leave_memory_alone():
    S = 4112
    f, src = fec(), sources(S)
    d = Dst(4, S, seed=9)
    lib = rsmi.load()
    jobs0, rows0 = f.stat(f.STAT_COMBINE_JOBS), f.stat(f.STAT_COMBINE_ROWS)
    u64, u8 = ctypes.c_uint64, ctypes.c_uint8
    keep = []

    def job(srcs, dsts, coef=None, accumulate=0, reserved=0, nsrc=None, nout=None):
        hs = (u64 * max(len(srcs), 1))(*srcs) if srcs is not None else None
        hd = (u64 * max(len(dsts), 1))(*dsts) if dsts is not None else None
        nsrc = len(srcs) if nsrc is None else nsrc
        nout = len(dsts) if nout is None else nout
        hc = (u8 * max(nsrc * nout, 1))(*([7] * (nsrc * nout))) if coef is None else coef
        keep.append((hs, hd, hc))
        return rsmi.CombineJob(hs, hd, hc if hc else None, nsrc, nout, accumulate, reserved)

    def call(jobs, count=None, length=S):
        arr = (rsmi.CombineJob * max(len(jobs), 1))(*jobs)
        return lib.rs_combine(f._h, arr, len(jobs) if count is None else count, length, None)

    a, b = src.ptr(0), src.ptr(1)
    good = job([a, b], [d.ptr(0)])
    bad = [
        job(None, [d.ptr(1)], nsrc=1),                    # NULL src
        job([a], None, nout=1),                           # NULL dst
        job([a], [d.ptr(1)], coef=False),                 # NULL coef
        job([a], [d.ptr(1)], nsrc=0),                     # nsrc outside 1..256
        job([a] * 257, [d.ptr(1)]),
        job([a], [d.ptr(1)], nout=0),                     # nout outside 1..256
        job([a], [d.ptr(1)] * 2, nout=257),
        job([a], [d.ptr(1)], accumulate=2),
        job([a], [d.ptr(1)], reserved=1),
        job([a, 0], [d.ptr(1)]),                          # NULL address
        job([a], [0]),
        job([a + 8], [d.ptr(1)]),                         # misaligned address
        job([a], [d.ptr(1) + 4]),
        job([a], [d.ptr(1), d.ptr(1)]),                   # a dst twice
        job([a], [d.ptr(1), d.ptr(1) + r16(S) - 16]),     # two dsts share 16 bytes
        job([a], [d.ptr(0) + r16(S) - 16]),               # a dst meets the good job's dst
        job([d.ptr(1)], [d.ptr(1)]),                      # src is dst
        job([d.ptr(1) + r16(S) - 16], [d.ptr(1)]),        # src shares the dst's last 16 bytes
        job([d.ptr(0) + 16], [d.ptr(1)]),                 # src meets the good job's dst
        job([a], [b]),                                    # dst is the good job's src
    ]
    for i, j in enumerate(bad):
        assert call([good, j]) == rsmi.RS_EINVAL, i
        assert call([j, good]) == rsmi.RS_EINVAL, i
    assert lib.rs_combine(f._h, None, 1, S, None) == rsmi.RS_EINVAL          # NULL jobs
    assert call([good], count=1 << 32) == rsmi.RS_EINVAL                     # count >= 2^32
    assert call([job([16], [1 << 40])], length=1 << 32) == rsmi.RS_EINVAL    # a len the stripe calls refuse
    # 2^31 blocks: 4,096 jobs x 2^19 column chunks of 2 GiB buffers (refused before anything
    # is read: the addresses are bare aligned numbers 4 GiB apart)
    big = [job([16], [(i + 1) << 32]) for i in range(4096)]
    assert call(big, length=1 << 31) == rsmi.RS_EINVAL
    # nothing to do: RS_OK whatever the jobs hold
    assert call([bad[3]], count=0) == rsmi.RS_OK
    assert call([bad[3]], length=0) == rsmi.RS_OK
    assert lib.rs_combine(f._h, None, 0, S, None) == rsmi.RS_OK
    f.sync()
    d.check({}, "refusals")  # byte-identical: nothing is loose
    src.check()
    assert (f.stat(f.STAT_COMBINE_JOBS), f.stat(f.STAT_COMBINE_ROWS)) == (jobs0, rows0)
    # ranges that touch are served: dst rows 32 bytes apart, and a src right behind a dst
    tight = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=4 * r16(S), dtype=np.uint8)).cuda()
    before = tight.cpu().numpy()
    t = tight.data_ptr()
    f.combine([([t + 2 * r16(S), t + 3 * r16(S)], [t, t + r16(S)], bytes([1, 0, 0, 1]), 0)], S)
    f.sync()
    after = tight.cpu().numpy()
    assert np.array_equal(after[2 * r16(S):], before[2 * r16(S):])
    for r in range(2):
        assert np.array_equal(after[r * r16(S):r * r16(S) + S], before[(2 + r) * r16(S):(2 + r) * r16(S) + S])


def test_combine_two_calls_on_one_stream_are_sequential():
    S = 5000
    f, src = fec(), sources(S)
    d = Dst(5, S, seed=17)
    rng = np.random.default_rng(18)
    A, B, C = (matrix(rng, 5, 10, None) for _ in range(3))
    ids = [list(range(q, q + 10)) for q in (0, 5, 40)]
    pa, pb, pc = (oracle.matmul_stripe(M, [src.shard(c) for c in i]) for M, i in zip((A, B, C), ids))
    dp = [d.ptr(r) for r in range(5)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    f.combine([([src.ptr(c) for c in ids[0]], dp, A.tobytes(), 0)], S, stream=stream.cuda_stream)
    f.combine([([src.ptr(c) for c in ids[1]], dp, B.tobytes(), 1)], S, stream=stream.cuda_stream)
    f.sync(stream.cuda_stream)
    d.check({r: pa[r] ^ pb[r] for r in range(5)}, "overwrite, accumulate")
    f.combine([([src.ptr(c) for c in ids[1]], dp, B.tobytes(), 1)], S, stream=stream.cuda_stream)
    f.combine([([src.ptr(c) for c in ids[2]], dp, C.tobytes(), 0)], S, stream=stream.cuda_stream)
    f.combine([([src.ptr(c) for c in ids[0]], dp, A.tobytes(), 1)], S, stream=stream.cuda_stream)
    f.sync(stream.cuda_stream)
    d.check({r: pc[r] ^ pa[r] for r in range(5)}, "accumulate, overwrite, accumulate")
    src.check()


def test_combine_device_set_routes_the_call():
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert fs.kernel_name(6) == "combine_MG4_B256"
    check_multi_job(fs, 4112, 3, seed=300)
    check_multi_job(fs, 4112, 1, seed=301)
    fs.close()


def test_combine_kernel_names():
    assert fec().kernel_name(6).startswith("combine_")
    assert fec().kernel_name(6) == "combine_MG4_B256"        # nsrc 10, nout 4
    assert fec(64, 80).kernel_name(6) == "combine_MG4_B256"  # nsrc 64, nout min(16, 4)
    f = rsmi.FEC(4, 4, device=0)                             # m = 0: nout 1
    assert f.kernel_name(6) == "combine_MG4_B256"
    f.close()


def test_combine_multi_iteration_child():
    """RSMI_ITERS is read once per process: a child with RSMI_ITERS=2 runs
    shapes of every variant over a several-chunk length (two column chunks
    per block, the second one's loads issued from inside the loop)."""
    env = dict(os.environ, RSMI_ITERS="2")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "iters child ok" in run.stdout


if __name__ == "__main__":
    assert os.environ.get("RSMI_ITERS") == "2"
    check_cross(fec(), ITERS_S, [1, 3, 10, 200], [1, 4, 5, 17])
    check_multi_job(fec(), ITERS_S, 3, seed=400)
    check_partial_sum_repair(fec(), 10, 14, ITERS_S, 3, seed=401)
    print("iters child ok")

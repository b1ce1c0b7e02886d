"""GPU: rs_combine_lens -- rs_combine with a length per job, served by the
per-job-length twin of the combine kernel (rs_combine_kernel<.., VARLEN>).

The expected bytes always come from the oracle (oracle.matmul_stripe) or from
the pristine bytes, never from the engine, and every comparison is bit-exact.
Every destination sits in random bytes with a 64-byte guard band in front and
another behind round_up(len, 16): after a call the len bytes of every dst hold
the expected bytes and everything else is byte-identical to before, the
sources included; only the <= 15 bytes in [len, round_up(len, 16)) of a
written dst are exempt.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the RSMI_ITERS child of test_combine_lens_multi_iteration_child
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "noise-erasurecode-plugin_amd"), os.path.join(_root, "tests")):
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from oracle import oracle  # noqa: E402

# nothing | one byte | a column less one | one column | a column and a byte |
# a 4 KiB block chunk less a byte | exactly one block of 256 lanes x 16 B |
# a second block with one live lane | two blocks | three and one live lane
LENGTHS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289]
# MG4 | MG4 | a second row group of one row (of MG 4) | two row groups of any
# MG | MG16 | the call takes row groups of 8: 200 sources do not fit with 16
SHAPES = [(1, 1), (10, 4), (10, 5), (3, 17), (64, 16), (200, 9)]
MAXLEN = 12289
GUARD = 64


def r16(x):
    return (x + 15) // 16 * 16


_FECS = {}


def fec(k=10, n=14):
    if (k, n) not in _FECS:
        _FECS[(k, n)] = rsmi.FEC(k, n, device=0)
    return _FECS[(k, n)]


class Sources:
    """256 source buffers of MAXLEN bytes on the host (read-only) and the
    device, 16 random bytes between neighbours; a job of length L reads the
    first round_up(L, 16) bytes of the ones it names."""

    def __init__(self, seed):
        self.slot = r16(MAXLEN) + 16
        rng = np.random.default_rng(seed)
        self.host = rng.integers(0, 256, size=256 * self.slot, dtype=np.uint8)
        self.host.setflags(write=False)
        self.dev = torch.from_numpy(self.host.copy()).cuda()

    def ptr(self, c):
        return self.dev.data_ptr() + c * self.slot

    def shard(self, c, length):
        return self.host[c * self.slot:c * self.slot + length]

    def check(self):
        assert np.array_equal(self.dev.cpu().numpy(), self.host), "a source changed"


_SOURCES = []


def sources():
    if not _SOURCES:
        _SOURCES.append(Sources(seed=20250))
    return _SOURCES[0]


class Dst:
    """Destination buffers of their own lengths inside random bytes: GUARD
    bytes in front of each and GUARD bytes behind its round_up(len, 16)."""

    def __init__(self, lengths, seed):
        self.lengths = list(lengths)
        self.offs, at = [], 0
        for length in self.lengths:
            self.offs.append(at + GUARD)
            at += GUARD + r16(length) + GUARD
        rng = np.random.default_rng(seed)
        self.pristine = rng.integers(0, 256, size=max(at, 16), dtype=np.uint8)
        self.pristine.setflags(write=False)
        self.dev = torch.from_numpy(self.pristine.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self, r):
        return self.dev.data_ptr() + self.offs[r]

    def old(self, r):
        return self.pristine[self.offs[r]:self.offs[r] + self.lengths[r]]

    def check(self, expected, what=""):
        """expected: {row: its bytes}; every other byte, the guard bands
        included, as in pristine."""
        want = self.pristine.copy()
        loose = np.zeros(len(want), dtype=bool)
        for r, v in expected.items():
            o, length = self.offs[r], self.lengths[r]
            assert len(v) == length
            want[o:o + length] = v
            loose[o + length:o + r16(length)] = True
        got = self.dev.cpu().numpy()
        bad = np.flatnonzero((got != want) & ~loose)
        assert bad.size == 0, (what, bad[:8].tolist(), bad.size)


def matrix(rng, nout, nsrc):
    """Random coefficients with zeros and ones sprinkled in."""
    M = rng.integers(2, 256, size=(nout, nsrc), dtype=np.uint8)
    flat = M.reshape(-1)
    some = rng.permutation(flat.size)
    few = max(1, flat.size // 6)
    if flat.size >= 2:
        flat[some[:few]] = 1
    if flat.size >= 3:
        flat[some[few:2 * few]] = 0
    return M


class Call:
    """One rs_combine_lens call of the jobs `specs` = [(length, nsrc, nout,
    accumulate)]: its job list, its destinations and what the oracle expects
    in them."""

    def __init__(self, specs, seed):
        self.specs = list(specs)
        src = sources()
        rng = np.random.default_rng(seed)
        self.dst = Dst([length for length, _, nout, _ in self.specs for _ in range(nout)], seed=seed + 1)
        self.jobs, self.lens, self.expected, row = [], [], {}, 0
        for length, nsrc, nout, acc in self.specs:
            ids = [int(c) for c in rng.integers(0, 256, size=nsrc)]  # with repeats
            M = matrix(rng, nout, nsrc)
            if length:
                prod = oracle.matmul_stripe(M, [src.shard(c, length) for c in ids])
                for r in range(nout):
                    self.expected[row + r] = self.dst.old(row + r) ^ prod[r] if acc else prod[r]
            self.jobs.append(([src.ptr(c) for c in ids], [self.dst.ptr(row + r) for r in range(nout)], M.tobytes(), acc))
            self.lens.append(length)
            row += nout
        self.live = sum(1 for length, _, _, _ in self.specs if length)
        self.rows = sum(nout for length, _, nout, _ in self.specs if length)

    def run(self, f, what, stream=0):
        jobs0, rows0 = f.stat(f.STAT_COMBINE_JOBS), f.stat(f.STAT_COMBINE_ROWS)
        f.combine_lens(self.jobs, self.lens, stream=stream)
        f.sync(stream)
        self.dst.check(self.expected, what)
        sources().check()
        assert f.stat(f.STAT_COMBINE_JOBS) - jobs0 == self.live       # empty jobs are not counted
        assert f.stat(f.STAT_COMBINE_ROWS) - rows0 == self.rows


def mixed_specs():
    """Every length with every shape, overwrite and accumulate alternating
    along both."""
    return [(length, nsrc, nout, (i + j) & 1) for i, length in enumerate(LENGTHS) for j, (nsrc, nout) in enumerate(SHAPES)]


def check_mixed(f, seed):
    launches0 = f.stat(f.STAT_COMBINE_LENS_LAUNCHES)
    Call(mixed_specs(), seed).run(f, "mixed shapes")
    assert f.stat(f.STAT_COMBINE_LENS_LAUNCHES) - launches0 == 1
    # the narrow shapes alone: row groups of 4, and a call of one row group
    launches0 = f.stat(f.STAT_COMBINE_LENS_LAUNCHES)
    Call([(length, nsrc, nout, i & 1) for i, length in enumerate(LENGTHS) for nsrc, nout in SHAPES[:2]], seed + 10).run(f, "MG 4")
    Call([(length, nsrc, nout, i & 1) for i, length in enumerate(LENGTHS) for nsrc, nout in SHAPES[:3]], seed + 20).run(f, "MG 8")
    assert f.stat(f.STAT_COMBINE_LENS_LAUNCHES) - launches0 == 2


def test_combine_lens_mixed_shapes():
    check_mixed(fec(), seed=1000)


def many_lengths(count, seed):
    """Seeded lengths in [0, 9000] with runs of empty jobs at the start, in
    the middle and at the end."""
    lens = [int(v) for v in np.random.default_rng(seed).integers(0, 9001, size=count)]
    for b in range(6):
        lens[b] = lens[count // 2 + b] = lens[count - 1 - b] = 0
    return lens


def test_combine_lens_block_search_over_many_jobs():
    """1500 jobs of (4, 2): the search of the block map on the device; every
    job's output and guard bands are checked."""
    f = fec()
    lens = many_lengths(1500, seed=77)
    assert min(lens[6:700]) < 4096 < max(lens) and sum(1 for v in lens if v == 0) >= 18
    launches0 = f.stat(f.STAT_COMBINE_LENS_LAUNCHES)
    Call([(length, 4, 2, b & 1) for b, length in enumerate(lens)], seed=78).run(f, "1500 jobs")
    assert f.stat(f.STAT_COMBINE_LENS_LAUNCHES) - launches0 == 1


def test_combine_lens_multi_iteration_child():
    """RSMI_ITERS is read once per process: a child with RSMI_ITERS=3 runs the
    mixed call -- several column chunks of one job per block, the next block
    starting in the middle of the job -- and a many-job call."""
    env = dict(os.environ, RSMI_ITERS="3")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "iters child ok" in run.stdout


def test_combine_lens_equal_lengths_is_combine():
    """One length for all jobs: the bytes rs_combine leaves, written by
    rs_combine's kernel -- the twin's launch counter stays where it is."""
    f = fec()
    assert f.kernel_name(6) == "combine_MG4_B256" and f.kernel_name(9) == "combine_lens_MG4_B256"
    assert fec(64, 80).kernel_name(9) == "combine_lens_MG4_B256"
    for length in (4097, 5000, 16):
        specs = [(length, nsrc, nout, i & 1) for i, (nsrc, nout) in enumerate(SHAPES[:5])]
        a, b = Call(specs, seed=length), Call(specs, seed=length)  # the same jobs over two sets of destinations
        launches0 = f.stat(f.STAT_COMBINE_LENS_LAUNCHES)
        a.run(f, f"equal lengths {length}")
        assert f.stat(f.STAT_COMBINE_LENS_LAUNCHES) == launches0
        f.combine(b.jobs, length)
        f.sync()
        b.dst.check(b.expected, f"rs_combine {length}")
        got_a, got_b = a.dst.dev.cpu().numpy(), b.dst.dev.cpu().numpy()
        for r in range(len(a.dst.lengths)):
            o = a.dst.offs[r]
            assert np.array_equal(got_a[o:o + length], got_b[o:o + length]), r
    # lengths that differ only within a 16-byte column are one length to the kernels
    specs = [(4081 + i, 10, 4, 0) for i in range(16)]
    launches0 = f.stat(f.STAT_COMBINE_LENS_LAUNCHES)
    Call(specs, seed=5).run(f, "one column count")
    assert f.stat(f.STAT_COMBINE_LENS_LAUNCHES) == launches0
    # an empty job among them, or one more column, takes the twin
    Call(specs + [(0, 10, 4, 0)], seed=6).run(f, "and an empty job")
    Call(specs + [(4097, 10, 4, 0)], seed=7).run(f, "and a longer job")
    assert f.stat(f.STAT_COMBINE_LENS_LAUNCHES) - launches0 == 2


def test_combine_lens_refusals_leave_memory_alone():
    f, src = fec(), sources()
    S, L = 1000, 9000
    d = Dst([L, L, L, L], seed=9)
    lib = rsmi.load()
    stats0 = [f.stat(w) for w in (f.STAT_COMBINE_JOBS, f.STAT_COMBINE_ROWS, f.STAT_COMBINE_LENS_LAUNCHES)]
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

    def call(jobs, lens, count=None):
        arr = (rsmi.CombineJob * max(len(jobs), 1))(*jobs)
        hl = (ctypes.c_size_t * max(len(lens), 1))(*lens) if lens is not None else None
        return lib.rs_combine_lens(f._h, arr, len(jobs) if count is None else count, hl, None)

    a, b = src.ptr(0), src.ptr(1)
    good = job([a, b], [d.ptr(0)])
    bad = [  # (job, its length): refused next to the good job of L bytes, in either order
        (job(None, [d.ptr(1)], nsrc=1), S),                    # NULL src
        (job([a], None, nout=1), S),                           # NULL dst
        (job([a], [d.ptr(1)], coef=False), S),                 # NULL coef
        (job([a], [d.ptr(1)], nsrc=0), S),                     # nsrc outside 1..256
        (job([a], [d.ptr(1)], nout=0), S),                     # nout outside 1..256
        (job([a], [d.ptr(1)], accumulate=2), S),
        (job([a], [d.ptr(1)], reserved=1), S),
        (job([a, 0], [d.ptr(1)]), S),                          # NULL address
        (job([a + 8], [d.ptr(1)]), S),                         # misaligned address
        (job([a], [d.ptr(1) + 4]), S),
        (job([a], [d.ptr(1)], reserved=1), 0),                 # an empty job is validated like any other
        (job([a + 8], [d.ptr(1)]), 0),
        (job([a], [d.ptr(1), d.ptr(1)]), S),                   # a dst twice
        (job([a], [d.ptr(0) + r16(L) - 16]), S),               # a short dst in the good job's last column
        (job([d.ptr(0) + 4096], [d.ptr(1)]), S),               # a short src deep inside the good job's dst
        (job([d.ptr(1)], [d.ptr(1)]), S),                      # src is dst
        (job([a], [b]), S),                                    # dst is the good job's src
        (job([a], [d.ptr(1)]), 1 << 32),                       # 2^28 columns
    ]
    for i, (j, length) in enumerate(bad):
        assert call([good, j], [L, length]) == rsmi.RS_EINVAL, i
        assert call([j, good], [length, L]) == rsmi.RS_EINVAL, i
    assert call([good], None) == rsmi.RS_EINVAL                                       # NULL lens
    assert lib.rs_combine_lens(f._h, None, 1, (ctypes.c_size_t * 1)(S), None) == rsmi.RS_EINVAL   # NULL jobs
    # 2^31 blocks: 4,096 jobs of 2^19 column chunks (refused before anything is read: the
    # addresses are bare aligned numbers 4 GiB apart)
    big = [job([16], [(i + 1) << 32]) for i in range(4096)]
    assert call(big, [1 << 31] * 4096) == rsmi.RS_EINVAL
    # nothing to do: RS_OK
    assert call([bad[3][0]], [S], count=0) == rsmi.RS_OK
    assert call([good, good], [0, 0]) == rsmi.RS_OK
    assert lib.rs_combine_lens(f._h, None, 0, None, None) == rsmi.RS_OK
    f.sync()
    d.check({}, "refusals")  # byte-identical: nothing is loose
    src.check()
    assert [f.stat(w) for w in (f.STAT_COMBINE_JOBS, f.STAT_COMBINE_ROWS, f.STAT_COMBINE_LENS_LAUNCHES)] == stats0
    # ranges that touch are served: a long dst that starts right behind a short one's span
    tight = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=r16(S) + r16(L) + 64, dtype=np.uint8)).cuda()
    before = tight.cpu().numpy()
    t = tight.data_ptr()
    f.combine_lens([([a], [t], b"\x01", 0), ([b], [t + r16(S)], b"\x01", 0)], [S, L])
    f.sync()
    after = tight.cpu().numpy()
    assert np.array_equal(after[:S], src.shard(0, S)) and np.array_equal(after[r16(S):r16(S) + L], src.shard(1, L))
    assert np.array_equal(after[r16(S) + r16(L):], before[r16(S) + r16(L):])


def test_combine_lens_two_calls_on_one_stream_are_sequential():
    f, src = fec(), sources()
    lens = [5000, 17, 4097]
    d = Dst([length for length in lens for _ in range(5)], seed=17)
    rng = np.random.default_rng(18)
    A, B, C = ([matrix(rng, 5, 10) for _ in lens] for _ in range(3))
    ids = [list(range(q, q + 10)) for q in (0, 5, 40)]

    def prod(Ms, i):
        return [oracle.matmul_stripe(M, [src.shard(c, length) for c in i]) for M, length in zip(Ms, lens)]

    pa, pb, pc = prod(A, ids[0]), prod(B, ids[1]), prod(C, ids[2])

    def jobs(Ms, i, acc):
        return [([src.ptr(c) for c in i], [d.ptr(5 * b + r) for r in range(5)], M.tobytes(), acc) for b, M in enumerate(Ms)]

    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    f.combine_lens(jobs(A, ids[0], 0), lens, stream=stream.cuda_stream)
    f.combine_lens(jobs(B, ids[1], 1), lens, stream=stream.cuda_stream)
    f.sync(stream.cuda_stream)
    d.check({5 * b + r: pa[b][r] ^ pb[b][r] for b in range(3) for r in range(5)}, "overwrite, accumulate")
    f.combine_lens(jobs(B, ids[1], 1), lens, stream=stream.cuda_stream)
    f.combine_lens(jobs(C, ids[2], 0), lens, stream=stream.cuda_stream)
    f.combine_lens(jobs(A, ids[0], 1), lens, stream=stream.cuda_stream)
    f.sync(stream.cuda_stream)
    d.check({5 * b + r: pc[b][r] ^ pa[b][r] for b in range(3) for r in range(5)}, "accumulate, overwrite, accumulate")
    src.check()


def test_combine_lens_device_set_routes_the_call():
    fs = rsmi.FEC(10, 14, devices=[0, 0])
    assert fs.kernel_name(9) == "combine_lens_MG4_B256"
    launches0 = fs.stat(fs.STAT_COMBINE_LENS_LAUNCHES)
    # the first job is empty and names no device memory: the first destination of the first
    # job with bytes routes the call
    call = Call([(0, 3, 2, 0), (4097, 10, 4, 0), (17, 3, 17, 1), (0, 1, 1, 1), (8192, 10, 5, 0)], seed=300)
    call.jobs[0] = ([16, 32, 48], [64, 80], call.jobs[0][2], 0)
    call.run(fs, "device set")
    Call([(4097, 10, 4, 1), (16, 10, 4, 0)], seed=301).run(fs, "device set, two jobs")
    assert fs.stat(fs.STAT_COMBINE_LENS_LAUNCHES) - launches0 == 2
    fs.close()


if __name__ == "__main__":
    assert os.environ.get("RSMI_ITERS") == "3"
    check_mixed(fec(), seed=2000)
    Call([(length, 4, 2, b & 1) for b, length in enumerate(many_lengths(300, seed=79))], seed=80).run(fec(), "300 jobs")
    # lengths of many chunks: blocks of three iterations whose neighbours start in the middle of the job
    Call([(length, 10, 4, i & 1) for i, length in enumerate([12289, 4096 * 3, 4096 * 3 + 16, 4096 * 2, 4096 * 2 + 16, 4097])],
         seed=81).run(fec(), "whole iterations")
    print("iters child ok")

"""GPU: far addresses through every strided call -- stripes past 4 GiB, shards
past 2 GiB (far_image.py).

Every strided kernel addresses a shard as base + stripe * stripe_stride +
shard * pitch + column * 16, and the host planning computes the same
addresses.  Three ways of making a term of that sum large, none of which needs
a large workload:

  far pitch / far stride   a few stripes of ~5,000-byte shards whose pitch is
                           2^26 .. 2^29 bytes, in an allocation nothing
                           initialises: shard * pitch and stripe * stride pass
                           2^31 and 2^32 (FAR below);
  far by stripe index      2^22 + 3 stripes of 80-byte pitch of which three
                           are listed (the list-driven calls);
  long shards              one stripe of (2^31 + 8,232)-byte shards: the
                           column offset passes 2^31.

The sparse layouts are checked through FarDevice.check(): every window around
a shard slot, and around every place a truncated form of its address would
point to, is compared bit-exact with a host model whose expected bytes come
from the oracle, and per-segment sums prove that nothing else in the
allocation was written.  The long shards are filled by fill_splitmix and
compared with the oracle at sampled columns (far_image.sampled_columns) and,
wherever the expected bytes exist on the device, over their full length.

Each test asserts the kernel names and the counters of its call, frees its
tensors and empties the cache; no layout is kept across tests.  A test skips
only if the device has less free memory than it allocates plus 1 GiB.
"""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import far_image as fi  # noqa: E402
import rsmi  # noqa: E402
from oracle import oracle  # noqa: E402
from strided_image import r16  # noqa: E402

CLEAN = rsmi.RS_VERIFY_CLEAN
G31, G32 = 1 << 31, 1 << 32

# name: (k, n), S, pitch, mode, stripes
FAR = {
    # K-specialised kernels, MG4
    "far10j": ((10, 14), 5000, (1 << 29) + 48, "joined", 2),
    # separate parity base
    "far10s": ((10, 14), 5000, (1 << 29) + 48, "split", 3),
    # runtime-k kernels, two row groups of 16, update copy commit
    "far12": ((12, 40), 4112, (1 << 27) + 48, "joined", 2),
    # bit-sliced encode, syndrome reconstruct, K64 read / check
    "far64": ((64, 80), 4112, (1 << 26) + 48, "joined", 2),
}
NAMES = list(FAR)
# rs_kernel_name(ctx, which) per code: encode, reconstruct, verify, update,
# read, check, combine, degraded update, column scrub, combine_lens
KERNELS = {
    (10, 14): ("K10_MG4_B256", "K10_MG4_B256", "verify_K10_MG4_B256", "update_MG4_B256", "read_K10_MG4_B256",
               "check_K10_MG4_B256", "combine_MG4_B256", "update_degraded_MG4_B256", "columns_MG4_B256",
               "combine_lens_MG4_B256"),
    (12, 40): ("K0_MG8_B256", "K0_MG8_B256", "verify_K0_MG8_B256", "update_MG16_B256", "read_K0_MG4_B256",
               "check_K0_MG4_B256", "combine_MG4_B256", "update_degraded_MG16_B256", None, "combine_lens_MG4_B256"),
    (64, 80): ("bitslice_k64_m16", "bitslice_rec_k64_m16", "verify_K64_MG16_B256", "update_MG16_B256",
               "read_K64_MG4_B256", "check_K64_MG4_B256", "combine_MG4_B256", "update_degraded_MG16_B256",
               "columns_MG16_B256", "combine_lens_MG4_B256"),
    (4, 6): ("K4_MG4_B256", "K4_MG4_B256", "verify_K4_MG4_B256", "update_MG4_B256", "read_K4_MG4_B256",
             "check_K4_MG4_B256", "combine_MG4_B256", "update_degraded_MG4_B256", "columns_MG4_B256",
             "combine_lens_MG4_B256"),
    (5, 7): ("K0_MG4_B256", "K0_MG4_B256", "verify_K0_MG4_B256", "update_MG4_B256", "read_K0_MG4_B256",
             "check_K0_MG4_B256", "combine_MG4_B256", "update_degraded_MG4_B256", "columns_MG4_B256",
             "combine_lens_MG4_B256"),
    (8, 14): ("bitslice_k8_m6", "bitslice_rec_k8_m6", "verify_K8_MG6_B256", "update_MG8_B256", "read_K8_MG4_B256",
              "check_K8_MG4_B256", "combine_MG4_B256", "update_degraded_MG8_B256", "columns_MG8_B256",
              "combine_lens_MG4_B256"),
}
ENC, REC, VERIFY, UPDATE, READ, CHECK, COMBINE, UPDATE_DEG, COLUMNS, COMBINE_LENS = range(10)


def _fec_env(k, n, **env):
    """FEC built with RSMI_* knobs set (the kernel choice is made at rs_new)."""
    old = {key: os.environ.get(key) for key in env}
    os.environ.update(env)
    try:
        return rsmi.NewFEC(k, n)
    finally:
        for key, v in old.items():
            if v is None:
                del os.environ[key]
            else:
                os.environ[key] = v


_CTX = {}


def ctx(k, n, **env):
    key = (k, n, tuple(sorted(env.items())))
    if key not in _CTX:
        _CTX[key] = _fec_env(k, n, **env)
    return _CTX[key]


def assert_kernel(f, which):
    want = KERNELS[(f.k, f.n)][which]
    assert want is not None and f.kernel_name(which) == want, (f.k, f.n, which, f.kernel_name(which))


def need(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + (1 << 30):
        pytest.skip(f"needs {(nbytes >> 30) + 1} GiB free on the device, {free >> 30} GiB are")


@pytest.fixture(autouse=True)
def _report(request):
    """Peak torch allocation and wall time of every test, one line each."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    held, t0 = torch.cuda.memory_allocated(), time.perf_counter()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"\nFAR-REPORT {request.node.name} peak_GiB={peak / 2**30:.2f} wall_s={time.perf_counter() - t0:.2f}")
    assert torch.cuda.memory_allocated() < held + (64 << 20), "a test left its big tensors allocated"


# ---------------------------------------------------------------- layouts ----
def far_layout(name):
    (k, n), S, pitch, mode, stripes = FAR[name]
    L = fi.FarLayout(k, n, S, stripes, pitch, mode)
    assert L.margin == G31 + 256
    rel = lambda s, i: L.shard_at(s, i)[1] - L.margin  # noqa: E731  offset from the buffer's base pointer
    if name == "far10j":
        assert rel(0, 4) == G31 + 192 and rel(0, 8) == G32 + 384 and rel(1, 0) == L.dss > 7 << 30
    elif name == "far10s":
        assert rel(0, 4) == G31 + 192 and rel(0, 8) == G32 + 384 and rel(1, 0) == L.dss > 5 << 30
        assert L.shard_at(2, 10) == (1, L.margin + 2 * L.pss) and 2 * L.pss == G32 + 416  # parity stripe 2
    elif name == "far12":
        assert rel(0, 32) == G32 + 1536 and 32 - 12 == 20 and 20 >= 16  # parity row 20: the second row group
    elif name == "far64":
        assert rel(0, 32) == G31 + 1536 and rel(0, 64) == G32 + 3072
    assert sum(L.sizes) < 26 << 30
    return L


def rel(L, s, i):
    return L.shard_at(s, i)[1] - L.margin


def far_pair(L, s):
    """Two far shards of stripe s: the first and the last of those that lie
    2^32 or more behind their base pointer (2^31 where there are not two)."""
    for bound in (G32, G31):
        far = [i for i in range(L.n) if rel(L, s, i) >= bound]
        if len(far) >= 2:
            return far[0], far[-1]
    raise AssertionError("no far shards")


def far_data(L, s):
    """The farthest data shard of stripe s."""
    return max(range(L.k), key=lambda i: rel(L, s, i))


def open_far(img):
    need(sum(img.L.sizes))
    return img.upload(fi.TorchBuffers("cuda"))


def first_bad(f, call, dev, stripes, *extra):
    fb = torch.full((stripes,), 0x55555555, dtype=torch.int32, device="cuda")
    call(*dev.args(), *extra, fb.data_ptr())
    f.sync()
    return fb.cpu().numpy().view(np.uint32).tolist()


class Src:
    """New contents for update calls: slots of round_up(S, 16) + 16 random
    bytes in one small device buffer of their own."""

    def __init__(self, count, S, seed):
        self.S, self.slot = S, r16(S) + 16
        self.host = np.random.default_rng(seed).integers(0, 256, size=count * self.slot, dtype=np.uint8)
        self.dev = torch.from_numpy(self.host.copy()).cuda()

    def ptr(self, q):
        return self.dev.data_ptr() + q * self.slot

    def shard(self, q):
        return self.host[q * self.slot:q * self.slot + self.S]

    def check(self):
        assert np.array_equal(self.dev.cpu().numpy(), self.host), "the src buffers changed"


class Dst:
    """Destinations of read calls: slots of round_up(S, 16) bytes inside 64
    random bytes on each side."""

    def __init__(self, count, S, seed):
        self.S, self.slot = S, r16(S) + 128
        self.host = np.random.default_rng(seed).integers(0, 256, size=count * self.slot, dtype=np.uint8)
        self.dev = torch.from_numpy(self.host.copy()).cuda()

    def ptr(self, q):
        return self.dev.data_ptr() + q * self.slot + 64

    def check(self, shards, what):
        got = self.dev.cpu().numpy()
        want, loose = self.host.copy(), np.zeros(len(self.host), dtype=bool)
        for q, sh in enumerate(shards):
            o = q * self.slot + 64
            want[o:o + self.S] = sh
            loose[o + self.S:o + r16(self.S)] = True
        bad = np.flatnonzero((got != want) & ~loose)
        assert bad.size == 0, (what, bad[:8].tolist(), bad.size)


def updated_image(L, ups, src, flags=None):
    """The image of an update call: ups = [(stripe, shard)], entry q taking
    src.shard(q).  Present changed shards hold the new bytes, present parity
    shards the oracle's parity of the new payload; erased slots (flags) hold
    garbage before and after."""
    img = L.image()
    rng = np.random.default_rng(len(ups) + 17)
    if flags is not None:
        for s, i in zip(*np.nonzero(flags)):
            img.garbage(int(s), int(i), rng)
    for s in sorted({s for s, _ in ups}):
        new = np.stack([L.shard(s, i) for i in range(L.k)])
        for q, (s2, i) in enumerate(ups):
            if s2 == s:
                new[i] = src.shard(q)
                if flags is None or not flags[s, i]:
                    img.expect_written(s, i, new[i])
        par = fi.oracle_parity_columns(L.k, L.n, new)
        for r in range(L.m):
            if flags is None or not flags[s, L.k + r]:
                img.expect_written(s, L.k + r, par[r])
    return img


# ------------------------------------------------- far pitch, far stride ----
@pytest.mark.parametrize("name", NAMES)
def test_far_encode_stripes(name):
    L = far_layout(name)
    f = ctx(L.k, L.n)
    assert_kernel(f, ENC)
    img, rng = L.image(), np.random.default_rng(1)
    for s in range(L.stripes):
        for i in range(L.k, L.n):
            img.garbage(s, i, rng)
            img.expect_written(s, i)
    dev = open_far(img)
    try:
        f.encode_stripes(*dev.args())
        f.sync()
        dev.check(f"{name} encode")
    finally:
        dev.free()


def test_far_checker_notices_a_truncated_stride_and_a_stray_store():
    """The checker's teeth on the device, with calls that stay inside the
    allocation: an encode whose caller hands in the stripe stride mod 2^32
    (what a kernel with a 32-bit stripe product would compute) leaves stripe
    1's parity unwritten and stores elsewhere; a correct encode followed by 16
    bytes stored just behind a window passes the windows and fails the
    segment sums."""
    L = far_layout("far12")
    f = ctx(L.k, L.n)
    img, rng = L.image(), np.random.default_rng(1)
    for s in range(L.stripes):
        for i in range(L.k, L.n):
            img.garbage(s, i, rng)
            img.expect_written(s, i)
    dev = open_far(img)
    try:
        data, dss, parity, pss, pitch, S, stripes = dev.args()
        assert dss % G32 != dss and dss % G32 + (L.n - 1) * pitch + r16(S) < L.sizes[0] - L.margin
        f.encode_stripes(data, dss % G32, parity, pss % G32, pitch, S, stripes)
        f.sync()
        with pytest.raises(AssertionError, match="bytes differ in window"):
            dev.check("truncated stride")
        dev.load(img)
        f.encode_stripes(*dev.args())
        b, o = L.shard_at(1, L.k)
        past = o + r16(S) + fi.GUARD
        with pytest.raises(AssertionError, match="outside every window"):
            L.locate(b, past, 16)
        f.fill_splitmix(dev.ptrs[b] + past, 16, 77)
        f.sync()
        with pytest.raises(AssertionError, match="segment sums differ"):
            dev.check("stray store")
    finally:
        dev.free()


def erasure_sets(L):
    """A single erasure below 2^31, one above 2^32, m erasures straddling
    (shards spread over the whole stripe) -- in every stripe."""
    low = next(i for i in range(L.n) if 0 < rel(L, 0, i) < G31)
    high = max(range(L.k), key=lambda i: rel(L, 0, i)) if L.mode == "split" else \
        next(i for i in range(L.n) if rel(L, 0, i) >= G32)
    spread = sorted({int(x) for x in np.linspace(0, L.n - 1, L.m)})
    assert rel(L, 0, high) >= G32 and len(spread) == L.m
    assert min(rel(L, 0, i) for i in spread) < G31 and max(rel(L, 0, i) for i in spread) >= G32
    return [[low], [high], spread]


@pytest.mark.parametrize("name,small_split", [(n, None) for n in NAMES] + [("far64", "0")])
def test_far_reconstruct_stripes(name, small_split):
    L = far_layout(name)
    f = ctx(L.k, L.n) if small_split is None else ctx(L.k, L.n, RSMI_SMALL_SPLIT=small_split)
    assert_kernel(f, REC)
    syndrome = small_split == "0"  # else a call of so few stripes goes to the split-table kernel
    dev = None
    try:
        for q, ids in enumerate(erasure_sets(L)):
            er = np.zeros((L.stripes, L.n), dtype=np.uint8)
            er[:, ids] = 1
            img, rng = L.image(), np.random.default_rng(2 + q)
            for s in range(L.stripes):
                for i in ids:
                    img.garbage(s, i, rng)
                    img.expect_written(s, i)
            if dev is None:
                dev = open_far(img)
            else:
                dev.load(img)
            tab0, syn0 = f.stat(f.STAT_REC_STRIPES_TABLE), f.stat(f.STAT_REC_STRIPES_SYNDROME)
            f.reconstruct_stripes(*dev.args(), er.tobytes())
            f.sync()
            dev.check(f"{name} reconstruct {ids}")
            assert f.stat(f.STAT_REC_STRIPES_SYNDROME) - syn0 == (L.stripes if syndrome else 0)
            assert f.stat(f.STAT_REC_STRIPES_TABLE) - tab0 == (0 if syndrome else L.stripes)
    finally:
        if dev:
            dev.free()


@pytest.mark.parametrize("name", NAMES)
def test_far_verify_stripes(name):
    L = far_layout(name)
    f = ctx(L.k, L.n)
    assert_kernel(f, VERIFY)
    par = max(range(L.k, L.n), key=lambda i: rel(L, 1, i))   # a far parity shard of stripe 1
    ds = 0 if rel(L, 0, far_data(L, 0)) >= G32 else 1        # a far data shard, in stripe 0 where there is one
    # (a separate parity buffer's stripe 1 starts 2^31 + 208 bytes in: past 2^31, not yet 2^32)
    assert rel(L, 1, par) >= (G31 if L.mode == "split" else G32) and rel(L, ds, far_data(L, ds)) >= G32
    cases = [(None, [CLEAN] * L.stripes)]
    want = [CLEAN] * L.stripes
    want[1] = 1234
    cases.append(((1, par, 1234), want))
    want = [CLEAN] * L.stripes
    want[ds] = L.S - 1
    cases.append(((ds, far_data(L, ds), L.S - 1), want))
    dev = None
    try:
        for flip, want in cases:
            img = L.image()
            if flip:
                img.flip(*flip, 0x5A)
            if dev is None:
                dev = open_far(img)
            else:
                dev.load(img)
            assert first_bad(f, f.verify_stripes, dev, L.stripes) == want, (name, flip)
            dev.check(f"{name} verify {flip}")  # nothing is written
    finally:
        if dev:
            dev.free()


@pytest.mark.parametrize("name", NAMES)
def test_far_correct_stripes(name):
    L = far_layout(name)
    f = ctx(L.k, L.n)
    img, rng = L.image(), np.random.default_rng(3)
    wrong = [(s, far_pair(L, s)[s % 2]) for s in range(L.stripes)]  # one wholly wrong far shard per stripe
    for s, i in wrong:
        img.garbage(s, i, rng)
        img.expect_written(s, i)
    dev = open_far(img)
    try:
        status, rewritten = f.correct_stripes(*dev.args())
        assert status == [rsmi.RS_OK] * L.stripes
        assert [(x // L.n, x % L.n) for x, b in enumerate(rewritten) if b] == wrong
        dev.check(f"{name} correct")
    finally:
        dev.free()


@pytest.mark.parametrize("name", NAMES)
def test_far_update_stripes(name):
    L = far_layout(name)
    f = ctx(L.k, L.n)
    assert_kernel(f, UPDATE)
    ups = [(0, 1), (1, L.k - 1), (1, 2)]  # below 2^31 in stripe 0; stripe 1 lies past 2^32 as a whole
    assert rel(L, 0, 1) < G31 and rel(L, 1, 2) >= G32
    src = Src(len(ups), L.S, seed=4)
    dev = open_far(updated_image(L, ups, src))
    try:
        patched0, copies0 = f.stat(f.STAT_UPDATE_STRIPES), f.stat(f.STAT_UPDATE_COPY_COMMITS)
        f.update_stripes(*dev.args(), [(s, i, src.ptr(q)) for q, (s, i) in enumerate(ups)])
        f.sync()
        dev.check(f"{name} update")
        src.check()
        assert f.stat(f.STAT_UPDATE_STRIPES) - patched0 == 2
        assert f.stat(f.STAT_UPDATE_COPY_COMMITS) - copies0 == (1 if name == "far12" else 0)
    finally:
        dev.free()
        del src


@pytest.mark.parametrize("name", NAMES)
def test_far_read_stripes(name):
    L = far_layout(name)
    f = ctx(L.k, L.n)
    assert_kernel(f, READ)
    er = np.zeros((L.stripes, L.n), dtype=np.uint8)
    img, rng, wants = L.image(), np.random.default_rng(5), []
    for s in range(L.stripes):
        gone, present = far_pair(L, s)
        er[s, gone] = 1
        img.garbage(s, gone, rng)           # comes back as it was: storage is only read
        wants += [(s, gone), (s, present)]  # regenerated | copied (the copy-pieces kernel)
    dst = Dst(len(wants), L.S, seed=6)
    dev = open_far(img)
    try:
        regen0, copied0 = f.stat(f.STAT_READ_REGENERATED), f.stat(f.STAT_READ_COPIED)
        f.read_stripes(*dev.args(), er.tobytes(), [(s, i, dst.ptr(q)) for q, (s, i) in enumerate(wants)])
        f.sync()
        dst.check([L.shard(s, i) for s, i in wants], f"{name} read")
        dev.check(f"{name} read: storage")
        assert f.stat(f.STAT_READ_REGENERATED) - regen0 == L.stripes
        assert f.stat(f.STAT_READ_COPIED) - copied0 == L.stripes
    finally:
        dev.free()
        del dst


def degraded_image(L, repaired):
    """Per stripe one far shard erased (garbage, never read or written) and
    one far present shard with wrong bytes at offsets 77 and S - 2."""
    er = np.zeros((L.stripes, L.n), dtype=np.uint8)
    img, rng, bad = L.image(), np.random.default_rng(7), []
    for s in range(L.stripes):
        gone, present = far_pair(L, s)
        if s % 2:
            gone, present = present, gone
        er[s, gone] = 1
        img.garbage(s, gone, rng)
        img.flip(s, present, 77 + s, 0xA5, repaired)
        img.flip(s, present, L.S - 2, 0x01, repaired)
        if repaired:
            img.expect_written(s, present)  # regenerated in place
        bad.append((s, present))
    return img, er, bad


@pytest.mark.parametrize("name", NAMES)
def test_far_verify_degraded(name):
    L = far_layout(name)
    f = ctx(L.k, L.n)
    assert_kernel(f, CHECK)
    img, er, _ = degraded_image(L, repaired=False)
    dev = open_far(img)
    try:
        checked0 = f.stat(f.STAT_CHECK_STRIPES)
        got = first_bad(f, f.verify_degraded, dev, L.stripes, er.tobytes())
        assert got == [77 + s for s in range(L.stripes)], name
        assert f.stat(f.STAT_CHECK_STRIPES) - checked0 == L.stripes
        dev.check(f"{name} verify_degraded")
    finally:
        dev.free()


@pytest.mark.parametrize("name", NAMES)
def test_far_correct_degraded(name):
    L = far_layout(name)
    f = ctx(L.k, L.n)
    assert_kernel(f, CHECK)
    img, er, bad = degraded_image(L, repaired=True)
    dev = open_far(img)
    try:
        regen0, checked0 = f.stat(f.STAT_SCRUB_REGENERATED), f.stat(f.STAT_CHECK_STRIPES)
        status, rewritten = f.correct_degraded(*dev.args(), er.tobytes())
        assert status == [rsmi.RS_OK] * L.stripes
        assert [(x // L.n, x % L.n) for x, b in enumerate(rewritten) if b] == bad
        dev.check(f"{name} correct_degraded")
        assert f.stat(f.STAT_SCRUB_REGENERATED) - regen0 >= L.stripes
        assert f.stat(f.STAT_CHECK_STRIPES) - checked0 >= L.stripes
    finally:
        dev.free()


@pytest.mark.parametrize("form", ["pair", "decode"])
@pytest.mark.parametrize("name", NAMES)
def test_far_update_degraded(name, form):
    L = far_layout(name)
    f = ctx(L.k, L.n)
    assert_kernel(f, UPDATE_DEG)
    flags = np.zeros((L.stripes, L.n), dtype=np.uint8)
    if form == "pair":    # the changed shards present, a far parity shard erased (the last two stripes)
        a, b = L.stripes - 2, L.stripes - 1
        ups = [(a, 1), (b, far_data(L, b))]
        flags[a, L.n - 1] = flags[b, L.k] = 1
        assert rel(L, a, L.n - 1) >= G31 and rel(L, b, L.k) >= G32
    else:                 # the changed far shards erased: regenerated from the survivors for the patch
        ups = [(0, far_data(L, 0)), (1, 3)]
        for s, i in ups:
            flags[s, i] = 1
        assert rel(L, 1, 3) >= G32
    src = Src(len(ups), L.S, seed=8)
    dev = open_far(updated_image(L, ups, src, flags))
    try:
        stats = (f.STAT_UPDATE_DEGRADED, f.STAT_UPDATE_ABSORBED, f.STAT_UPDATE_STRIPES)
        before = [f.stat(x) for x in stats]
        f.update_degraded(*dev.args(), flags.tobytes(), [(s, i, src.ptr(q)) for q, (s, i) in enumerate(ups)])
        f.sync()
        dev.check(f"{name} update_degraded {form}")
        src.check()
        assert [f.stat(x) - b for x, b in zip(stats, before)] == [2, 0 if form == "pair" else 2, 0]
    finally:
        dev.free()
        del src


@pytest.mark.parametrize("name", [x for x in NAMES if FAR[x][0][1] - FAR[x][0][0] <= 16])
def test_far_correct_columns(name):
    L = far_layout(name)
    f = ctx(L.k, L.n)
    assert_kernel(f, COLUMNS)
    # three wrong bytes in three far shards at three offsets of stripe 1, one in stripe 0
    hits = [(1, 0, 5), (1, L.k - 1, L.S - 1), (1, L.n - 1, 2049), (0, far_pair(L, 0)[0], 4097)]
    img = L.image()
    for s, i, off in hits:
        assert rel(L, s, i) >= (G31 if L.mode == "split" else G32)
        img.flip(s, i, off, 0x3C, repaired=True)
    dev = open_far(img)
    try:
        handed0, bytes0 = f.stat(f.STAT_COLUMN_STRIPES), f.stat(f.STAT_COLUMN_BYTES)
        status, counts = f.correct_columns(*dev.args())
        assert status == [rsmi.RS_OK] * L.stripes
        assert {x: c for x, c in enumerate(counts) if c} == {s * L.n + i: 1 for s, i, _ in hits}
        dev.check(f"{name} correct_columns")  # only the wrong bytes are overwritten: nothing is loose
        assert f.stat(f.STAT_COLUMN_STRIPES) - handed0 == 2 and f.stat(f.STAT_COLUMN_BYTES) - bytes0 == 4
    finally:
        dev.free()


def decode_jobs(f, L, dev, img, lengths):
    """Two jobs that apply the decode row of one erased far shard from the far
    slots of its survivors into its own far slot: stripe 1 overwriting, stripe
    0 accumulating into the garbage the slot holds."""
    jobs = []
    for s, length, accumulate in ((1, lengths[0], 0), (0, lengths[1], 1)):
        gone = far_pair(L, s)[0]
        er = np.zeros(L.n, dtype=np.uint8)
        er[gone] = 1
        rows, count = f.pattern_rows(er.tobytes())
        ids = f.pattern_survivors(er.tobytes())
        assert count == 1 and gone not in ids and len(ids) == L.k
        img.garbage(s, gone, np.random.default_rng(9 + s))
        old = img.slot_bytes(s, gone)[:L.S]
        img.expect_written(s, gone, (old ^ L.shard(s, gone)) if accumulate else None, length=length)
        jobs.append(([dev_addr(dev, s, c) for c in ids], [dev_addr(dev, s, gone)], rows[:L.k], accumulate))
    return jobs


def dev_addr(dev, s, i):
    return dev.addr(s, i)


@pytest.mark.parametrize("lens", [False, True], ids=["combine", "combine_lens"])
@pytest.mark.parametrize("name", NAMES)
def test_far_combine(name, lens):
    L = far_layout(name)
    f = ctx(L.k, L.n)
    assert_kernel(f, COMBINE_LENS if lens else COMBINE)
    lengths = (L.S, L.S - 1003) if lens else (L.S, L.S)  # two lengths: the per-job-length kernel
    need(sum(L.sizes))
    dev = L.image().upload(fi.TorchBuffers("cuda"))      # the addresses first: the jobs name them
    try:
        img = L.image()
        jobs = decode_jobs(f, L, dev, img, lengths)
        dev.load(img)
        stats = (f.STAT_COMBINE_JOBS, f.STAT_COMBINE_ROWS, f.STAT_COMBINE_LENS_LAUNCHES)
        before = [f.stat(x) for x in stats]
        if lens:
            f.combine_lens(jobs, list(lengths))
        else:
            f.combine(jobs, L.S)
        f.sync()
        dev.check(f"{name} combine")
        assert [f.stat(x) - b for x, b in zip(stats, before)] == [2, 2, 1 if lens else 0]
    finally:
        dev.free()


# ------------------------------------------------------ far by stripe index ----
def index_layout():
    """RS(10,14), 40-byte shards at a pitch of 80, 2^22 + 3 stripes (~5 GiB):
    stripe 0, the first stripe whose offset passes 2^32 and the last are
    materialised and listed."""
    stripes = (1 << 22) + 3
    stride = 14 * 80 + 64
    mid = -(-G32 // stride)
    L = fi.FarLayout(10, 14, 40, stripes, 80, "joined", listed=[0, mid, stripes - 1], merge=True)
    assert L.dss == stride and (mid - 1) * stride < G32 <= mid * stride and mid == 3627507
    assert (stripes - 1) * stride > G32 + (1 << 29) and sum(L.sizes) < 7 << 30
    return L, mid


def test_far_index_update_stripes():
    L, mid = index_layout()
    f = ctx(10, 14)
    assert_kernel(f, UPDATE)
    ups = [(L.stripes - 1, 9), (0, 0), (mid, 4), (mid, 0), (L.stripes - 1, 3)]
    src = Src(len(ups), L.S, seed=10)
    dev = open_far(updated_image(L, ups, src))
    try:
        patched0 = f.stat(f.STAT_UPDATE_STRIPES)
        f.update_stripes(*dev.args(), [(s, i, src.ptr(q)) for q, (s, i) in enumerate(ups)])
        f.sync()
        dev.check("index update")
        src.check()
        assert f.stat(f.STAT_UPDATE_STRIPES) - patched0 == 3
    finally:
        dev.free()
        del src


def test_far_index_read_stripes():
    L, mid = index_layout()
    f = ctx(10, 14)
    assert_kernel(f, READ)
    er = np.zeros((L.stripes, L.n), dtype=np.uint8)
    img, rng, wants = L.image(), np.random.default_rng(11), []
    for s, gone, present in ((L.stripes - 1, 13, 0), (0, 2, 11), (mid, 0, 13)):
        er[s, gone] = 1
        img.garbage(s, gone, rng)
        wants += [(s, gone), (s, present)]
    dst = Dst(len(wants), L.S, seed=12)
    dev = open_far(img)
    try:
        regen0, copied0 = f.stat(f.STAT_READ_REGENERATED), f.stat(f.STAT_READ_COPIED)
        f.read_stripes(*dev.args(), er.tobytes(), [(s, i, dst.ptr(q)) for q, (s, i) in enumerate(wants)])
        f.sync()
        dst.check([L.shard(s, i) for s, i in wants], "index read")
        dev.check("index read: storage")
        assert f.stat(f.STAT_READ_REGENERATED) - regen0 == 3 and f.stat(f.STAT_READ_COPIED) - copied0 == 3
    finally:
        dev.free()
        del dst


def test_far_index_update_degraded():
    L, mid = index_layout()
    f = ctx(10, 14)
    assert_kernel(f, UPDATE_DEG)
    flags = np.zeros((L.stripes, L.n), dtype=np.uint8)
    ups = [(mid, 7), (L.stripes - 1, 0), (0, 5), (L.stripes - 1, 9)]
    flags[mid, 7] = flags[mid, 12] = 1          # decode form, a parity shard missing too
    flags[L.stripes - 1, 0] = 1                 # decode form next to a present changed shard
    flags[0, 13] = 1                            # pair form
    src = Src(len(ups), L.S, seed=13)
    dev = open_far(updated_image(L, ups, src, flags))
    try:
        stats = (f.STAT_UPDATE_DEGRADED, f.STAT_UPDATE_ABSORBED, f.STAT_UPDATE_STRIPES)
        before = [f.stat(x) for x in stats]
        f.update_degraded(*dev.args(), flags.tobytes(), [(s, i, src.ptr(q)) for q, (s, i) in enumerate(ups)])
        f.sync()
        dev.check("index update_degraded")
        src.check()
        assert [f.stat(x) - b for x, b in zip(stats, before)] == [3, 2, 0]
    finally:
        dev.free()
        del src


# ------------------------------------------------------------- long shards ----
LONG_S = G31 + 8192 + 40          # test_bitslice_rec_past_2gib's shape: ragged, past 2 GiB
LONG_CODES = [(4, 6), (5, 7)]     # K4 kernels | runtime k


class Long:
    """One stripe of LONG_S-byte shards in one buffer (parity = data + k *
    pitch), pitch round_up(S, 16) + 32, behind a margin of 2^31 + 256 bytes
    (FarLayout's: a column offset sign-extended from 32 bits stays inside the
    allocation) and with 256 bytes behind; the whole buffer is
    fill_splitmix's, the parity then encode_stripes'."""
    MARGIN = G31 + 256

    def __init__(self, f, k, n, extra=0, encode=True):
        self.f, self.k, self.n, self.m, self.S = f, k, n, n - k, LONG_S
        self.Sp = r16(LONG_S)
        self.pitch = self.Sp + 32
        self.size = self.MARGIN + n * self.pitch + 256
        need(self.size + extra)
        self.buf = torch.empty(self.size, dtype=torch.uint8, device="cuda")
        f.fill_splitmix(self.buf.data_ptr(), self.size, 0xFA5 + k)
        self.cols = fi.sampled_columns(self.Sp // 16)
        if encode:
            f.encode_stripes(*self.args())
            f.sync()

    def off(self, i):
        return self.MARGIN + i * self.pitch

    def addr(self, i):
        return self.buf.data_ptr() + self.off(i)

    def shard(self, i, buf=None):
        o = self.off(i)
        return (self.buf if buf is None else buf)[o:o + self.S]

    def args(self):
        return (self.addr(0), self.n * self.pitch, self.addr(self.k), self.n * self.pitch, self.pitch, self.S, 1)

    def columns(self, i):
        return fi.gather_columns(self.buf, self.off(i), self.cols)

    def check_parity_columns(self, what, rows=None):
        """The stored parity (rows: all of it) at the sampled columns against
        the oracle's of the stored data there (the 8 padding bytes of the
        ragged last column are not compared)."""
        live = len(self.cols) * 16 - (self.Sp - self.S)
        want = fi.oracle_parity_columns(self.k, self.n, np.stack([self.columns(i) for i in range(self.k)]))
        for r in range(self.m) if rows is None else rows:
            got = self.columns(self.k + r)
            bad = np.flatnonzero(got[:live] != want[r][:live])
            assert bad.size == 0, (what, "parity row", r, "sampled bytes", bad[:8].tolist())

    def free(self):
        del self.buf
        torch.cuda.empty_cache()


def same(a, b, chunk=1 << 30):
    """torch.equal in pieces of 1 GiB: its temporary is as large as its inputs."""
    assert a.shape == b.shape and a.dim() == 1
    return all(torch.equal(a[o:o + chunk], b[o:o + chunk]) for o in range(0, a.numel(), chunk))


def test_long_columns_cover_the_shape():
    cols = fi.sampled_columns(r16(LONG_S) // 16)
    assert cols[-1] * 16 + 16 == r16(LONG_S) and (1 << 27) in cols and (1 << 27) - 1 in cols and 0 in cols
    assert LONG_S % 16 == 8 and LONG_S - 1 > G31 + 5


@pytest.mark.parametrize("k,n", LONG_CODES + [(8, 14)])
def test_long_encode_stripes(k, n):
    f = ctx(k, n)
    assert_kernel(f, ENC)
    X = Long(f, k, n)
    try:
        X.check_parity_columns("encode")
    finally:
        X.free()


@pytest.mark.parametrize("degraded", [False, True], ids=["verify_stripes", "verify_degraded"])
@pytest.mark.parametrize("k,n", LONG_CODES)
def test_long_verify(k, n, degraded):
    f = ctx(k, n)
    assert_kernel(f, CHECK if degraded else VERIFY)
    X = Long(f, k, n)
    try:
        er = np.zeros((1, n), dtype=np.uint8)
        er[0, 1] = 1  # verify_degraded: data shard 1 is missing
        fb = torch.zeros(1, dtype=torch.int32, device="cuda")

        def run():
            fb.fill_(0x55555555)
            if degraded:
                f.verify_degraded(*X.args(), er.tobytes(), fb.data_ptr())
            else:
                f.verify_stripes(*X.args(), fb.data_ptr())
            f.sync()
            return int(fb.cpu().numpy().view(np.uint32)[0])

        assert run() == CLEAN
        X.shard(n - 1)[X.S - 1] ^= 0x80         # the last byte of the last parity shard
        assert run() == X.S - 1 and X.S - 1 > G31
        X.shard(2)[G31 + 5] ^= 0x01             # a data shard, just past 2 GiB: the lower offset wins
        assert run() == G31 + 5
        X.shard(0)[G31 - 1] ^= 0x10             # and just below
        assert run() == G31 - 1
    finally:
        X.free()


@pytest.mark.parametrize("call", ["read_stripes", "reconstruct_stripes"])
@pytest.mark.parametrize("k,n", LONG_CODES)
def test_long_regenerate(k, n, call):
    f = ctx(k, n)
    assert_kernel(f, READ if call == "read_stripes" else REC)
    X = Long(f, k, n, extra=3 * r16(LONG_S) + (1 << 30))
    try:
        gone = [1, n - 1]
        clones = [X.shard(i).clone() for i in gone]
        er = np.zeros((1, n), dtype=np.uint8)
        er[0, gone] = 1
        for i in gone:
            f.fill_splitmix(X.addr(i), X.Sp, 99 + i)
        # the oracle's Rebuild of data shard 1 at the sampled columns: the other
        # data shards and the highest-numbered present parity shard
        span, live = 16 * len(X.cols), 16 * len(X.cols) - (X.Sp - X.S)
        shares = [(i, X.columns(i).tobytes()) for i in [i for i in range(k) if i != 1] + [n - 2]]
        rc, ref = oracle.decode(oracle.fec_matrix(k, n), k, n, shares)
        assert rc == 0
        want = ref[span:span + live]
        if call == "reconstruct_stripes":
            f.reconstruct_stripes(*X.args(), er.tobytes())
            f.sync()
            assert X.columns(1).tobytes()[:live] == want
            for i, c in zip(gone, clones):
                assert same(X.shard(i), c), (call, i)
        else:
            for i, c in zip(gone, clones):  # one regenerated shard at a time: a dst of its own
                dst = torch.zeros(X.Sp, dtype=torch.uint8, device="cuda")
                f.read_stripes(*X.args(), er.tobytes(), [(0, i, dst.data_ptr())])
                f.sync()
                assert i != 1 or fi.gather_columns(dst, 0, X.cols).tobytes()[:live] == want
                assert same(dst[:X.S], c), (call, i)
                del dst
        del clones
    finally:
        X.free()


@pytest.mark.parametrize("call", ["update_stripes", "update_degraded_pair", "update_degraded_decode"])
@pytest.mark.parametrize("k,n", LONG_CODES)
def test_long_update(k, n, call):
    """One changed shard.  update_degraded in its pair form (the changed shard
    present, the last parity shard missing and left alone) and in its decode
    form (the changed shard missing: its old contents are regenerated for the
    patch, its slot is left alone)."""
    f = ctx(k, n)
    assert_kernel(f, UPDATE if call == "update_stripes" else UPDATE_DEG)
    X = Long(f, k, n, extra=(1 + (n - k)) * (r16(LONG_S) + 32) + (1 << 30))
    try:
        changed, rows = 2, list(range(X.m))
        src = torch.empty(X.Sp, dtype=torch.uint8, device="cuda")
        f.fill_splitmix(src.data_ptr(), X.Sp, 0xBEEF)
        if call == "update_stripes":
            f.update_stripes(*X.args(), [(0, changed, src.data_ptr())])
            f.sync()
        else:
            gone = n - 1 if call == "update_degraded_pair" else changed
            er = np.zeros((1, n), dtype=np.uint8)
            er[0, gone] = 1
            old_mid, old_cols = X.shard(gone)[G31 - 64:G31 + 64].clone(), X.columns(gone)
            stats = (f.STAT_UPDATE_DEGRADED, f.STAT_UPDATE_ABSORBED)
            before = [f.stat(x) for x in stats]
            f.update_degraded(*X.args(), er.tobytes(), [(0, changed, src.data_ptr())])
            f.sync()
            assert [f.stat(x) - b for x, b in zip(stats, before)] == [1, int(gone == changed)]
            assert same(X.shard(gone)[G31 - 64:G31 + 64], old_mid) and np.array_equal(X.columns(gone), old_cols), \
                "the erased slot was written"
            if gone == changed:
                X.buf[X.off(changed):X.off(changed) + X.Sp] = src  # what a repair would produce
            else:
                rows.remove(gone - k)
        assert same(X.shard(changed), src[:X.S]), "the data shard is not the source"
        X.check_parity_columns(call, rows)
        fresh = torch.empty(X.m * X.pitch, dtype=torch.uint8, device="cuda")
        f.encode_stripes(X.addr(0), n * X.pitch, fresh.data_ptr(), X.m * X.pitch, X.pitch, X.S, 1)
        f.sync()
        for r in rows:
            assert same(X.shard(k + r), fresh[r * X.pitch:r * X.pitch + X.S]), (call, "parity row", r)
        del src, fresh
    finally:
        X.free()


@pytest.mark.parametrize("call", ["correct_columns", "correct_stripes"])
@pytest.mark.parametrize("k,n", LONG_CODES)
def test_long_correct(k, n, call):
    f = ctx(k, n)
    X = Long(f, k, n, extra=Long.MARGIN + n * (r16(LONG_S) + 32) + 256 + (1 << 30))  # the clone, a piece of same()
    try:
        clone = X.buf.clone()
        if call == "correct_columns":   # wrong bytes in different shards, one per column
            assert_kernel(f, COLUMNS)
            hits = [(0, 5), (1, G31 - 1), (k, G31 + 5), (n - 1, X.S - 1), (0, G31 + 4096)]
        else:                           # all in one shard: located and regenerated
            hits = [(1, 5), (1, G31 - 1), (1, G31 + 5), (1, X.S - 1)]
        for i, off in hits:
            X.shard(i)[off] ^= 0x42
        if call == "correct_columns":
            status, counts = f.correct_columns(*X.args())
            assert counts == [sum(1 for i, _ in hits if i == x) for x in range(n)]
        else:
            status, rewritten = f.correct_stripes(*X.args())
            assert [int(b != 0) for b in rewritten] == [int(x == 1) for x in range(n)]
        assert status == [rsmi.RS_OK]
        for i in range(n):
            assert same(X.shard(i), X.shard(i, clone)), (call, "shard", i)
        if call == "correct_columns":   # only the wrong bytes are overwritten
            assert same(X.buf, clone)
        del clone
    finally:
        X.free()


@pytest.mark.parametrize("lens", [False, True], ids=["combine", "combine_lens"])
@pytest.mark.parametrize("k,n", LONG_CODES)
def test_long_combine(k, n, lens):
    """One job of LONG_S bytes: the encode matrix's parity rows applied to the
    data shards give the stored parity (overwrite), and accumulated onto the
    stored parity give zeros.  combine_lens gets a short second job, so that
    the per-job-length kernel serves the long one."""
    f = ctx(k, n)
    assert_kernel(f, COMBINE_LENS if lens else COMBINE)
    m = n - k
    X = Long(f, k, n, extra=2 * m * r16(LONG_S) + (1 << 30))
    try:
        E = np.frombuffer(f.matrix(), dtype=np.uint8).reshape(n, k)
        out = [torch.empty(X.Sp, dtype=torch.uint8, device="cuda") for _ in range(m)]
        acc = [X.buf[X.off(k + r):X.off(k + r) + X.Sp].clone() for r in range(m)]
        srcs = [X.addr(i) for i in range(k)]
        jobs = [(srcs, [t.data_ptr() for t in out], E[k:].tobytes(), 0),
                (srcs, [t.data_ptr() for t in acc], E[k:].tobytes(), 1)]
        launches0 = f.stat(f.STAT_COMBINE_LENS_LAUNCHES)
        if lens:
            small = torch.zeros(48, dtype=torch.uint8, device="cuda")
            f.combine_lens(jobs + [([X.addr(0)], [small.data_ptr()], b"\x01", 0)], [X.S, X.S, 40])
            f.sync()
            assert same(small[:40], X.shard(0)[:40])
        else:
            f.combine(jobs, X.S)
            f.sync()
        assert f.stat(f.STAT_COMBINE_LENS_LAUNCHES) - launches0 == (1 if lens else 0)
        live = len(X.cols) * 16 - (X.Sp - X.S)
        want = fi.oracle_parity_columns(k, n, np.stack([X.columns(i) for i in range(k)]))
        for r in range(m):
            assert np.array_equal(fi.gather_columns(out[r], 0, X.cols)[:live], want[r][:live]), ("oracle", r)
            assert same(out[r][:X.S], X.shard(k + r)), ("overwrite", r)
            assert not acc[r][:X.S].any(), ("accumulate", r)
        del out, acc
    finally:
        X.free()

"""Whole-image models for the strided and pointer-mode encode / reconstruct
tests (test_gpu_strided_image.py; unit-tested on the CPU in
test_strided_image.py).  A plain helper module: no fixtures, no GPU needed to
import it.

A Layout is a set of pristine stripes on the host with a strided device
layout in which nothing is dense: the shard pitch lies above round_up(S, 16),
both stripe strides carry a gap, and every device buffer has a guard band in
front and behind.  Payloads, pitch padding, gaps and guards are seeded random
bytes; the parity always comes from the oracle.  A Pool holds the same shards
at random rows of one buffer, for rs_reconstruct_ptrs.

An Image is the host model of a call: the bytes every device buffer holds
before it (`init`), the bytes it must hold afterwards (`want`), and the
`loose` mask of bytes that are not compared.  rsmi.h (device-resident batched
API): "bytes between shard_len and the next multiple of 16 are coded too:
padding, never read back by the host API" -- so bytes [S, round_up(S, 16)) of
a shard the call writes are the only loose ones, and check() counts them.
"""
import numpy as np

from oracle import oracle

GUARD = 256       # bytes of guard band in front of and behind every device buffer
DECOYS = 32       # pool rows that no table entry names


def r16(x):
    return (x + 15) // 16 * 16


def fixed_patterns(k, n):
    """Edge erasure sets (test_gpu_parity._fixed_patterns): every single
    erasure, all-data, all-parity, the m highest data shards, alternating,
    the first/last shard pairs, and sets straddling data shard 31/32 (the two
    words of the syndrome kernel's present-data mask)."""
    m = n - k
    pats = [[i] for i in range(n)]
    if k > 33:
        pats += [[31, 32], [33, 40, k - 1], [30, 31, 32, 33][:m], [32, k][:m]]
    pats += [list(range(min(m, k))), list(range(k, n)), list(range(k - min(m, k), k)),
             list(range(0, n, 2))[:m], [0, n - 1], [k - 1, k]]
    out = np.zeros((len(pats), n), dtype=np.uint8)
    for r, p in enumerate(pats):
        out[r, p[:m]] = 1
    return out


def random_erasures(rng, stripes, n, m, emin=1, emax=None):
    emax = m if emax is None else emax
    er = np.zeros((stripes, n), dtype=np.uint8)
    for s in range(stripes):
        e = int(rng.integers(emin, emax + 1))
        er[s, rng.choice(n, size=e, replace=False)] = 1
    return er


def erasure_set(k, n, seed):
    """The reconstruct tests' stripes: the edge sets, 16 random sets of 1..m
    erasures, and one stripe with nothing erased."""
    rng = np.random.default_rng(seed)
    return np.concatenate([fixed_patterns(k, n), random_erasures(rng, 16, n, n - k),
                           np.zeros((1, n), dtype=np.uint8)])


def lowest_parity_row(er_row, k, n):
    """The lowest parity row a pattern uses (erased parity outputs and
    Rebuild's parity survivors: the d highest present parity rows for d
    erased data shards), m if none.  Decides which syndrome kernel serves it."""
    m = n - k
    d = int(er_row[:k].sum())
    lo = m
    for t in range(m - 1, -1, -1):
        if er_row[k + t]:
            lo = t
        elif d > 0:
            lo, d = t, d - 1
    return lo


_CODED = {}


def coded(k, n, S, stripes):
    """(payload [stripes][k][S], oracle parity [stripes][m][S]), read-only,
    computed once per geometry (the last few geometries are kept)."""
    key = (k, n, S, stripes)
    if key not in _CODED:
        while len(_CODED) >= 8:
            del _CODED[next(iter(_CODED))]
        rng = np.random.default_rng(k * 1000003 + n * 10007 + S * 31 + stripes)
        payload = rng.integers(0, 256, size=(stripes, k, S), dtype=np.uint8)
        E = oracle.fec_matrix(k, n)
        ref = oracle.encode_batch(E, k, n, payload.reshape(-1), S, stripes).reshape(stripes, n - k, S).copy()
        payload.setflags(write=False)
        ref.setflags(write=False)
        _CODED[key] = (payload, ref)
    return _CODED[key]


class Image:
    """Host model of the device buffers around one call (or several on the
    same buffers): init / want / loose are lists of equally shaped arrays,
    one per device buffer; `written` is the number of shards the call is
    documented to write."""

    def __init__(self, names, init, S):
        self.names, self.S = list(names), S
        self.init = [b.copy() for b in init]
        self.want = [b.copy() for b in init]
        self.loose = [np.zeros(len(b), dtype=bool) for b in init]
        self.written = 0

    def garbage(self, buf, off, length, rng):
        """Random bytes in place before the call (and expected after it until
        expect_written says otherwise)."""
        g = rng.integers(0, 256, size=length, dtype=np.uint8)
        self.init[buf][off:off + length] = g
        self.want[buf][off:off + length] = g

    def expect_written(self, buf, off, shard):
        """The call writes a shard at off: [0, S) must hold `shard`, the
        padding up to round_up(S, 16) is loose, everything behind it stays."""
        S = self.S
        self.want[buf][off:off + S] = shard
        self.loose[buf][off + S:off + r16(S)] = True
        self.written += 1

    def check(self, got, what=""):
        """got: the device buffers' bytes after the call, one array per buffer."""
        n_loose = sum(int(lo.sum()) for lo in self.loose)
        assert n_loose == self.written * (r16(self.S) - self.S), \
            (what, "loose bytes", n_loose, "written shards", self.written, "S", self.S)
        assert len(got) == len(self.want)
        for name, g, w, lo in zip(self.names, got, self.want, self.loose):
            assert g.shape == w.shape, (what, name, g.shape, w.shape)
            bad = np.flatnonzero((g != w) & ~lo)
            assert bad.size == 0, f"{what} {name}: {bad.size} bytes differ, first offsets {bad[:8].tolist()}"


class Layout:
    """Pristine stripes of one geometry (read-only) and their strided layout.

    mode "split":  separate data and parity buffers, dss = k * pitch + 48 and
                   pss = m * pitch + 16.
    mode "joined": one buffer of whole stripes, parity = data + k * pitch and
                   dss == pss == n * pitch + 64."""

    def __init__(self, k, n, S, stripes, seed, mode):
        assert mode in ("split", "joined")
        self.k, self.n, self.m, self.S, self.stripes, self.mode = k, n, n - k, S, stripes, mode
        m = self.m
        self.pitch = r16(S) + 32
        if mode == "split":
            self.dss, self.pss = k * self.pitch + 48, m * self.pitch + 16
            self.names = ["data", "parity"]
            sizes = [stripes * self.dss, stripes * self.pss]
        else:
            self.dss = self.pss = n * self.pitch + 64
            self.names = ["stripes"]
            sizes = [stripes * self.dss]
        self.payload, self.ref = coded(k, n, S, stripes)
        rng = np.random.default_rng(seed)
        self.pristine = [rng.integers(0, 256, size=GUARD + sz + GUARD, dtype=np.uint8) for sz in sizes]
        for s in range(stripes):
            for i in range(n):
                b, o = self.shard_at(s, i)
                self.pristine[b][o:o + S] = self.payload[s, i] if i < k else self.ref[s, i - k]
        for a in self.pristine:
            a.setflags(write=False)

    def shard_at(self, s, i):
        """(buffer index, byte offset in that buffer) of shard i of stripe s."""
        if i < self.k:
            return 0, GUARD + s * self.dss + i * self.pitch
        if self.mode == "split":
            return 1, GUARD + s * self.pss + (i - self.k) * self.pitch
        return 0, GUARD + self.k * self.pitch + s * self.pss + (i - self.k) * self.pitch

    def shard(self, s, i):
        return self.payload[s, i] if i < self.k else self.ref[s, i - self.k]

    def args(self, ptrs):
        """The engine's (data, dss, parity, pss, pitch, S, stripes) for device
        buffers that start at ptrs (the guards included)."""
        data = ptrs[0] + GUARD
        parity = ptrs[1] + GUARD if self.mode == "split" else data + self.k * self.pitch
        return (data, self.dss, parity, self.pss, self.pitch, self.S, self.stripes)

    def encode_image(self, seed):
        """Before: every parity shard's whole pitch is random bytes.  After:
        [0, S) of every parity shard is the oracle's."""
        img = Image(self.names, self.pristine, self.S)
        rng = np.random.default_rng(seed)
        for s in range(self.stripes):
            for i in range(self.k, self.n):
                b, o = self.shard_at(s, i)
                img.garbage(b, o, self.pitch, rng)
        for s in range(self.stripes):
            for i in range(self.k, self.n):
                b, o = self.shard_at(s, i)
                img.expect_written(b, o, self.shard(s, i))
        return img

    def reconstruct_image(self, er, seed, repaired=None):
        """Before: every shard flagged in er is random bytes over its whole
        pitch.  After: those also flagged in `repaired` (default: all of
        them) hold the pristine shard in [0, S)."""
        assert er.shape == (self.stripes, self.n)
        repaired = er if repaired is None else repaired
        img = Image(self.names, self.pristine, self.S)
        rng = np.random.default_rng(seed)
        for s, i in zip(*np.nonzero(er)):
            b, o = self.shard_at(s, i)
            img.garbage(b, o, self.pitch, rng)
        for s, i in zip(*np.nonzero(er & repaired)):
            b, o = self.shard_at(s, i)
            img.expect_written(b, o, self.shard(s, i))
        return img


class Pool:
    """The shards of a geometry at random rows of one pool of stripes * n +
    DECOYS rows of round_up(S, 16) + 32 bytes, inside guard bands.  Rows,
    their padding, the decoys and the guards are random bytes."""

    def __init__(self, k, n, S, stripes, seed):
        self.k, self.n, self.m, self.S, self.stripes = k, n, n - k, S, stripes
        self.row_bytes = r16(S) + 32
        self.nrows = stripes * n + DECOYS
        self.payload, self.ref = coded(k, n, S, stripes)
        rng = np.random.default_rng(seed)
        perm = rng.permutation(self.nrows)
        self.rows = perm[:stripes * n].reshape(stripes, n)   # row of shard i of stripe s
        self.decoys = np.sort(perm[stripes * n:])
        buf = rng.integers(0, 256, size=GUARD + self.nrows * self.row_bytes + GUARD, dtype=np.uint8)
        for s in range(stripes):
            for i in range(n):
                o = self.row_at(self.rows[s, i])
                buf[o:o + S] = self.payload[s, i] if i < k else self.ref[s, i - k]
        buf.setflags(write=False)
        self.pristine = [buf]

    def row_at(self, row):
        return GUARD + int(row) * self.row_bytes

    def table(self, ptr):
        """The [stripes][n] address table for a device buffer that starts at
        ptr (the guard included): every entry names its shard's real row."""
        return (ptr + GUARD + self.rows.astype(np.int64) * self.row_bytes).astype(np.int64)

    def reconstruct_image(self, er, seed):
        assert er.shape == (self.stripes, self.n)
        img = Image(["pool"], self.pristine, self.S)
        rng = np.random.default_rng(seed)
        for s, i in zip(*np.nonzero(er)):
            img.garbage(0, self.row_at(self.rows[s, i]), self.row_bytes, rng)
        for s, i in zip(*np.nonzero(er)):
            img.expect_written(0, self.row_at(self.rows[s, i]),
                               self.payload[s, i] if i < self.k else self.ref[s, i - self.k])
        return img

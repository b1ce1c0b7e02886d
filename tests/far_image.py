"""Sparse images for the far-address tests (test_gpu_far_offsets.py; unit-
tested on the CPU in test_far_image.py).  A plain helper module in the style
of strided_image.py: no fixtures, no GPU needed to import it.

Every strided kernel addresses a shard as
    base + stripe * stripe_stride + shard * pitch + column * 16
and so does the host planning.  A far address needs a big stride, not a big
workload: a FarLayout gives a few small shards a pitch of hundreds of MiB, so
that shard * pitch and stripe * stride leave the low 32 bits in an allocation
nobody initialises (torch.empty) and of which only small windows are written.

Windows.  Every shard slot has the window [slot - 256, slot + r16(S) + 256),
seeded random bytes around the shard.  For every slot whose offset o from the
buffer start is >= wrap / 2 there are alias windows of the same size at
o mod wrap, at o mod (wrap / 2) and at margin + (o - margin) mod wrap: the
places an address truncated to 32 (or 31) bits would read or write.  `margin`
bytes lie in front of the image inside the same allocation, so that an offset
sign-extended from 32 bits lands inside the allocation as well: a latent bug
shows as a miscompare, never as a fault.  Construction asserts that every
window lies inside the allocation and that the slot windows are pairwise
disjoint.  Alias windows cannot all be: with a pitch of 2^29 + 48 shard 8 of a
stripe lies 2^32 + 384 bytes behind shard 0, so its alias is 384 bytes into
shard 0's own slot, whatever the margin.  Windows that meet are therefore
merged into one region, every byte of which is modelled and compared exactly
like a lone window's; a truncated access that lands on another shard's slot is
seen there.  (`merge=True` is for the one layout whose pitch is smaller than a
window -- many stripes of 80-byte pitch, far by stripe index: there the slot
windows of neighbouring shards are merged as well.)

A FarImage is the host model of a call over those windows (strided_image.Image's
init / want / loose), a FarDevice the allocation: upload() writes the windows
and takes a wrap-around int64 sum of every segment (wrap / 16 bytes: 256 MiB)
of the allocation; check() compares every window with the model, writes the
pre-call bytes back into the windows, and requires the segment sums to be what
they were.  The sums need no knowledge of the bytes torch.empty returned and
no second buffer, and they catch a store anywhere outside the windows.
"""
import bisect

import numpy as np

from oracle import oracle
from strided_image import coded, r16

GUARD = 256          # bytes of window on each side of a shard slot
SEGMENTS = 16        # segment sums per `wrap` bytes: 256 MiB at wrap = 2^32


class FarLayout:
    """Stripes of one geometry with a given shard pitch.

    mode "split":  separate data and parity buffers, dss = k * pitch + 48 and
                   pss = m * pitch + 16.
    mode "joined": one buffer of whole stripes, parity = data + k * pitch and
                   dss == pss == n * pitch + 64.
    Every buffer starts with `margin` bytes (default wrap / 2 + 256).  `listed`
    names the stripes that are materialised (default: all); payload[j] and
    ref[j] belong to stripe listed[j]."""

    def __init__(self, k, n, S, stripes, pitch, mode, margin=None, wrap=1 << 32, listed=None, merge=False, seed=0):
        assert mode in ("split", "joined")
        assert pitch % 16 == 0 and pitch >= r16(S), "the pitch must hold a shard"
        self.k, self.n, self.m, self.S, self.stripes, self.mode = k, n, n - k, S, stripes, mode
        self.pitch, self.wrap = pitch, wrap
        self.margin = wrap // 2 + 256 if margin is None else margin
        assert self.margin % 16 == 0
        m = self.m
        if mode == "split":
            self.dss, self.pss = k * pitch + 48, m * pitch + 16
            self.names = ["data", "parity"]
            sizes = [stripes * self.dss, stripes * self.pss]
        else:
            self.dss = self.pss = n * pitch + 64
            self.names = ["stripes"]
            sizes = [stripes * self.dss]
        self.sizes = [r16(self.margin + sz + GUARD) for sz in sizes]
        self.listed = list(range(stripes)) if listed is None else [int(s) for s in listed]
        assert len(set(self.listed)) == len(self.listed) and all(0 <= s < stripes for s in self.listed)
        self._row = {s: j for j, s in enumerate(self.listed)}
        self.payload, self.ref = coded(k, n, S, len(self.listed))
        self.win = r16(S) + 2 * GUARD
        self._windows(merge)
        rng = np.random.default_rng(seed + k * 7919 + n * 104729 + S * 13 + stripes)
        self.pristine = [rng.integers(0, 256, size=hi - lo, dtype=np.uint8) for _, lo, hi in self.regions]
        for s in self.listed:
            for i in range(n):
                r, at = self.locate(*self.shard_at(s, i), r16(S))
                self.pristine[r][at:at + S] = self.shard(s, i)
        for a in self.pristine:
            a.setflags(write=False)

    # -- addressing (strided_image.Layout's, the guard replaced by the margin) --
    def shard_at(self, s, i):
        """(buffer index, byte offset in that buffer) of shard i of stripe s."""
        if i < self.k:
            return 0, self.margin + s * self.dss + i * self.pitch
        if self.mode == "split":
            return 1, self.margin + s * self.pss + (i - self.k) * self.pitch
        return 0, self.margin + self.k * self.pitch + s * self.pss + (i - self.k) * self.pitch

    def shard(self, s, i):
        j = self._row[s]
        return self.payload[j, i] if i < self.k else self.ref[j, i - self.k]

    def args(self, ptrs):
        """The engine's (data, dss, parity, pss, pitch, S, stripes) for device
        buffers that start at ptrs (the margins included)."""
        data = ptrs[0] + self.margin
        parity = ptrs[1] + self.margin if self.mode == "split" else data + self.k * self.pitch
        return (data, self.dss, parity, self.pss, self.pitch, self.S, self.stripes)

    # -- windows ---------------------------------------------------------------
    def aliases(self, o):
        """Where a truncated form of the buffer offset o would point."""
        if o < self.wrap // 2:
            return []
        cand = (o % self.wrap, o % (self.wrap // 2), self.margin + (o - self.margin) % self.wrap)
        return sorted({a for a in cand if a != o})

    def _windows(self, merge):
        slots = [self.shard_at(s, i) for s in self.listed for i in range(self.n)]
        taken = set(slots)
        wins = [(b, o - GUARD, o - GUARD + self.win, "slot") for b, o in slots]
        seen = set()
        for b, o in slots:
            for a in self.aliases(o):
                if (b, a) not in taken and (b, a) not in seen:  # a slot's own window watches it already
                    seen.add((b, a))
                    wins.append((b, a - GUARD, a - GUARD + self.win, "alias"))
        wins.sort()
        for b, lo, hi, kind in wins:
            assert 0 <= lo and hi <= self.sizes[b], f"{kind} window [{lo}, {hi}) of {self.names[b]} leaves the allocation"
        self.windows = wins
        regions, slot_hi = [], {}
        for b, lo, hi, kind in wins:
            if kind == "slot":
                assert merge or lo >= slot_hi.get(b, 0), \
                    f"slot windows overlap in {self.names[b]}: [{lo}, {hi}) starts below {slot_hi[b]}"
                slot_hi[b] = hi
            if regions and regions[-1][0] == b and lo < regions[-1][2]:
                regions[-1][2] = max(regions[-1][2], hi)
            else:
                regions.append([b, lo, hi])
        self.regions = [tuple(r) for r in regions]
        self._starts = [[lo for rb, lo, _ in self.regions if rb == b] for b in range(len(self.sizes))]
        self._first = [sum(1 for rb, _, _ in self.regions if rb < b) for b in range(len(self.sizes))]

    def locate(self, b, o, length):
        """(region index, offset in it) of bytes [o, o + length) of buffer b."""
        r = self._first[b] + bisect.bisect_right(self._starts[b], o) - 1
        rb, lo, hi = self.regions[r]
        assert rb == b and lo <= o and o + length <= hi, (b, o, length, "outside every window")
        return r, o - lo

    def image(self):
        return FarImage(self)


class FarImage:
    """Host model of the windows around one call (or several on the same
    buffers): init / want / loose per region, as strided_image.Image keeps
    them per buffer; `written` counts the shards the call is documented to
    write."""

    def __init__(self, L):
        self.L, self.S = L, L.S
        self.init = [a.copy() for a in L.pristine]
        self.want = [a.copy() for a in L.pristine]
        self.loose = [np.zeros(len(a), dtype=bool) for a in L.pristine]
        self.written = self.slack = 0

    def garbage(self, s, i, rng):
        """Random bytes over round_up(S, 16) bytes of the slot before the call
        (and expected after it until expect_written says otherwise)."""
        r, at = self.L.locate(*self.L.shard_at(s, i), r16(self.S))
        g = rng.integers(0, 256, size=r16(self.S), dtype=np.uint8)
        self.init[r][at:at + len(g)] = g
        self.want[r][at:at + len(g)] = g

    def expect_written(self, s, i, shard=None, length=None):
        """The call writes shard i of stripe s: [0, S) must hold `shard` (the
        pristine one by default), the padding up to round_up(S, 16) is loose,
        everything around it stays.  length: a call that codes only the first
        `length` bytes of the slot."""
        S = self.S if length is None else length
        r, at = self.L.locate(*self.L.shard_at(s, i), r16(self.S))
        self.want[r][at:at + S] = (self.L.shard(s, i) if shard is None else shard)[:S]
        self.loose[r][at + S:at + r16(S)] = True
        self.written += 1
        self.slack += r16(S) - S

    def slot_bytes(self, s, i):
        """The round_up(S, 16) bytes the slot holds before the call."""
        r, at = self.L.locate(*self.L.shard_at(s, i), r16(self.S))
        return self.init[r][at:at + r16(self.S)].copy()

    def flip(self, s, i, off, xor, repaired=False):
        """A wrong byte at offset off of the slot before the call; the call
        leaves it (default) or puts the right one back."""
        r, at = self.L.locate(*self.L.shard_at(s, i), r16(self.S))
        assert 0 <= off < self.S and 0 < xor < 256
        self.init[r][at + off] ^= xor
        if not repaired:
            self.want[r][at + off] ^= xor

    def check(self, read, what=""):
        """read(buffer, offset, length) -> the bytes there after the call."""
        n_loose = sum(int(lo.sum()) for lo in self.loose)
        assert n_loose == self.slack, (what, "loose bytes", n_loose, "written shards", self.written, "want", self.slack)
        for (b, lo, hi), w, loose in zip(self.L.regions, self.want, self.loose):
            g = read(b, lo, hi - lo)
            assert g.shape == w.shape, (what, self.L.names[b], g.shape, w.shape)
            bad = np.flatnonzero((g != w) & ~loose)
            assert bad.size == 0, (f"{what} {self.L.names[b]}: {bad.size} bytes differ in window [{lo}, {hi}), "
                                   f"first offsets {(bad[:8] + lo).tolist()}")

    def upload(self, backend):
        return FarDevice(self, backend)


class NumpyBuffers:
    """The allocation on the host, for the CPU test's engines."""

    def alloc(self, size):
        return np.random.default_rng(size).integers(0, 256, size=size, dtype=np.uint8)  # "uninitialised"

    def write(self, buf, off, data):
        buf[off:off + len(data)] = data

    def read(self, buf, off, length):
        return buf[off:off + length].copy()

    def sums(self, buf, seg):
        full = len(buf) // seg * seg
        out = np.frombuffer(buf[:full], dtype=np.int64).reshape(-1, seg // 8).sum(axis=1).tolist() if full else []
        tail = buf[full:]
        if len(tail):
            words = len(tail) // 8 * 8
            out.append(int(np.frombuffer(tail[:words], dtype=np.int64).sum()) + int(tail[words:].astype(np.int64).sum()))
        return out

    def ptr(self, buf):
        return buf.ctypes.data

    def free(self, bufs):
        pass


class TorchBuffers:
    """The allocation on the GPU: torch.empty, nothing initialises it."""

    def __init__(self, device="cuda"):
        import torch
        self.torch, self.device = torch, device

    def alloc(self, size):
        return self.torch.empty(size, dtype=self.torch.uint8, device=self.device)

    def write(self, buf, off, data):
        buf[off:off + len(data)] = self.torch.from_numpy(np.ascontiguousarray(data)).to(self.device)

    def read(self, buf, off, length):
        return buf[off:off + length].cpu().numpy()

    def sums(self, buf, seg):
        torch = self.torch
        full = buf.numel() // seg * seg
        out = buf[:full].view(torch.int64).view(-1, seg // 8).sum(dim=1).cpu().tolist() if full else []
        tail = buf[full:]
        if tail.numel():
            words = tail.numel() // 8 * 8
            out.append(int(tail[:words].view(torch.int64).sum().item()) + int(tail[words:].to(torch.int64).sum().item()))
        return out

    def ptr(self, buf):
        return buf.data_ptr()

    def free(self, bufs):
        bufs.clear()
        self.torch.cuda.empty_cache()


class FarDevice:
    """The buffers of a FarImage: allocated, the windows written, the segment
    sums taken.  check() is the whole comparison after the call(s)."""

    def __init__(self, img, backend):
        self.img, self.L, self.backend = img, img.L, backend
        self.seg = self.L.wrap // SEGMENTS
        assert self.seg % 8 == 0
        self.bufs = [backend.alloc(size) for size in self.L.sizes]
        self.nbytes = sum(self.L.sizes)
        self._restore()
        self.sums0 = [backend.sums(buf, self.seg) for buf in self.bufs]

    def _restore(self):
        for (b, lo, _), a in zip(self.L.regions, self.img.init):
            self.backend.write(self.bufs[b], lo, a)

    def load(self, img):
        """Another image of the same layout on the same buffers."""
        assert img.L is self.L
        self.img = img
        self._restore()
        self.sums0 = [self.backend.sums(buf, self.seg) for buf in self.bufs]

    @property
    def ptrs(self):
        return [self.backend.ptr(buf) for buf in self.bufs]

    def args(self):
        return self.L.args(self.ptrs)

    def addr(self, s, i):
        """The address of shard i of stripe s."""
        b, o = self.L.shard_at(s, i)
        return self.backend.ptr(self.bufs[b]) + o

    def check(self, what=""):
        """Every window against the model; then the pre-call bytes go back
        into the windows and every segment sum must be what it was: nothing
        outside the windows was written."""
        self.img.check(lambda b, o, length: self.backend.read(self.bufs[b], o, length), what)
        self._restore()
        for name, buf, before in zip(self.L.names, self.bufs, self.sums0):
            after = self.backend.sums(buf, self.seg)
            bad = [q for q, (x, y) in enumerate(zip(before, after)) if x != y]
            assert not bad, f"{what} {name}: segment sums differ outside the windows, segments {bad[:8]} of {self.seg} bytes"

    def free(self):
        self.backend.free(self.bufs)


# -- sampled columns of long shards ---------------------------------------------
def sampled_columns(ncols16, boundary=1 << 27):
    """The 16-byte columns test_bitslice_rec_past_2gib samples, a few more
    around each place: both ends of the shard, both sides of `boundary` (the
    column at 2 GiB) and the ragged end, with +-1 and +-511 / 512 around each."""
    cols = set()
    for c in (0, boundary, ncols16 - 1):
        cols.update(c + d for d in (-513, -512, -511, -2, -1, 0, 1, 2, 511, 512, 513))
    return sorted(c for c in cols if 0 <= c < ncols16)


def column_index(cols):
    """Byte offsets of the 16-byte columns `cols`."""
    return (np.asarray(cols, dtype=np.int64)[:, None] * 16 + np.arange(16, dtype=np.int64)[None, :]).reshape(-1)


def gather_columns(buf, off, cols):
    """The bytes of columns `cols` of the device shard that starts at byte
    `off` of the torch tensor `buf`, on the host."""
    import torch
    idx = torch.from_numpy(column_index(cols) + off).to(buf.device)
    return buf[idx].cpu().numpy()


def oracle_parity_columns(k, n, data_cols):
    """The oracle's parity [m][L] of data columns [k][L]."""
    data_cols = np.ascontiguousarray(data_cols, dtype=np.uint8)
    L = data_cols.shape[1]
    return oracle.encode_batch(oracle.fec_matrix(k, n), k, n, data_cols.reshape(-1), L, 1).reshape(n - k, L)

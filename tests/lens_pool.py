"""Whole-image model for the per-stripe-length scrub of the pointer placement
(rs_verify_ptrs_lens, rs_reconstruct_checked_ptrs_lens; test_gpu_scrub_lens.py).
A plain helper module: no fixtures, and no GPU needed to import it.

A LensPool holds stripes whose shards have a length of their stripe's own, at
random rows of ONE device buffer between guard bands.  Every row has
round_up(S_max, 16) + 32 bytes; stripe s uses the first S_s bytes of its rows,
and the rest of every row holds random bytes that are NOT a continuation of
the codeword: a kernel that compares or reads past a short stripe's length
reports a mismatch instead of faulting, and a write past it shows in the
image.  Payloads are seeded, the parity comes from the oracle.

A LensRun is the host model of calls on one pool: `cur` is what the buffer
holds before a call, `want` what it must hold afterwards, `fb` the verdicts.
The table entries of erased shards name decoy rows -- for a repair distinct
ones, the destinations -- and the erased shards' own rows are overwritten with
random bytes that no entry names.  Expected bytes never come from the engine:
a stripe's codeword is the oracle's Decode of its survivors' bytes as they are
in `cur`, re-encoded by the oracle, over the round_up(S_s, 16) bytes the
kernels move.
"""
import numpy as np

from oracle import oracle
from strided_image import GUARD, r16

CLEAN = 0xFFFFFFFF
SENTINEL = 0x7A7A7A7A
# one column | exactly one 4 KiB block chunk | a chunk plus a column | not a
# multiple of 16 | several chunks | a sub-column | two columns, the second of
# one byte | nothing
MIX = [16, 4096, 4112, 5000, 3 * 4096 + 40, 1, 17, 0]

_MATRIX = {}


def matrix(k, n):
    if (k, n) not in _MATRIX:
        _MATRIX[(k, n)] = oracle.fec_matrix(k, n)
    return _MATRIX[(k, n)]


def deal(mix, stripes, seed, window=0, longest=None):
    """Lengths for `stripes` stripes from a seeded shuffle of `mix`, cycled:
    window w takes the stripes-long piece behind window w - 1's, so
    ceil(len(mix) / stripes) windows use every length.  Neighbours in one
    shuffle differ, so no window of two or more stripes has one length only.
    longest: "first" / "last" moves the longest stripe there."""
    order = [int(x) for x in np.random.default_rng(seed).permutation(mix)]
    lens = [order[(window * stripes + i) % len(order)] for i in range(stripes)]
    if longest is not None:
        at = int(np.argmax(lens))
        to = 0 if longest == "first" else stripes - 1
        lens[at], lens[to] = lens[to], lens[at]
    return lens


def windows(mix, stripes):
    return -(-len(mix) // stripes)


def rebuild_choice(k, n, er_row):
    """Rebuild's survivors: every present data share, then the highest present parity."""
    c = [i for i in range(k) if not er_row[i]]
    for i in range(n - 1, k - 1, -1):
        if len(c) < k and not er_row[i]:
            c.append(i)
    return sorted(c)


def oracle_codeword(k, n, shares):
    """The n shards of the codeword through k shares [(id, bytes)]: the
    oracle's Decode, then its Encode."""
    E = matrix(k, n)
    rc, data = oracle.decode(E, k, n, shares)
    assert rc == 0, rc
    L = len(shares[0][1])
    par = oracle.encode(E, k, n, data) if n > k else b""
    rows = [data[i * L:(i + 1) * L] for i in range(k)] + [par[i * L:(i + 1) * L] for i in range(n - k)]
    return [np.frombuffer(r, dtype=np.uint8) for r in rows]


class LensPool:
    """Stripe s of RS(k, n) has lens[s] bytes per shard.  stripes * n shard rows
    and stripes * m + 8 decoy rows, in a seeded random order."""

    def __init__(self, k, n, lens, seed):
        self.k, self.n, self.m = k, n, n - k
        self.lens = [int(x) for x in lens]
        self.stripes = stripes = len(self.lens)
        self.row_bytes = r16(max(self.lens)) + 32
        self.nrows = stripes * n + stripes * self.m + 8
        rng = np.random.default_rng(seed)
        perm = rng.permutation(self.nrows)
        self.rows = perm[:stripes * n].reshape(stripes, n)  # row of shard i of stripe s
        self.decoys = perm[stripes * n:]
        buf = rng.integers(0, 256, size=GUARD + self.nrows * self.row_bytes + GUARD, dtype=np.uint8)
        E = matrix(k, n)
        self.shards = []  # [stripe] -> (n, S_s)
        for s, S in enumerate(self.lens):
            data = rng.integers(0, 256, size=(k, S), dtype=np.uint8)
            par = np.frombuffer(oracle.encode(E, k, n, data.tobytes()), dtype=np.uint8).reshape(self.m, S) \
                if S and self.m else np.zeros((self.m, S), dtype=np.uint8)
            word = np.concatenate([data, par])
            word.setflags(write=False)
            self.shards.append(word)
            for i in range(n):
                o = self.row_at(self.rows[s, i])
                buf[o:o + S] = word[i]
        buf.setflags(write=False)
        self.pristine = buf

    def row_at(self, row):
        return GUARD + int(row) * self.row_bytes


class LensRun:
    def __init__(self, P, er=None, repair=False, seed=0):
        self.P, self.repair = P, repair
        self.er = np.zeros((P.stripes, P.n), dtype=np.uint8) if er is None else \
            np.asarray(er, dtype=np.uint8).reshape(P.stripes, P.n).copy()
        self.cur = P.pristine.copy()
        self.entry_row = P.rows.copy()  # the row each table entry names
        self.flips = {}                 # stripe -> [(shard, offset)]
        rng = np.random.default_rng(7000 + seed)
        free = [int(d) for d in P.decoys]
        for s, i in zip(*np.nonzero(self.er)):
            o = P.row_at(P.rows[s, i])
            self.cur[o:o + P.row_bytes] = rng.integers(0, 256, size=P.row_bytes, dtype=np.uint8)  # the lost shard
            # verify: any decoy, entries may repeat; repair: a destination of its own
            self.entry_row[s, i] = free.pop() if repair else free[int(rng.integers(len(free)))]
        self.dev = self.table = self.host_table = self.first_bad = None
        self.want = self.fb = None

    # ---- the image before the call
    def at(self, s, i):
        return self.P.row_at(self.P.rows[s, i])

    def present(self, s):
        return [i for i in range(self.P.n) if not self.er[s, i]]

    def survivors(self, s):
        return rebuild_choice(self.P.k, self.P.n, self.er[s])

    def compared(self, s):
        c = set(self.survivors(s))
        return [i for i in self.present(s) if i not in c]

    def flip(self, s, i, off, mask=0x20):
        """XORs mask into byte off of the ROW of present shard i of stripe s;
        off may lie at or beyond the stripe's length."""
        assert mask and not self.er[s, i] and 0 <= off < self.P.row_bytes
        self.cur[self.at(s, i) + off] ^= mask
        self.flips.setdefault(int(s), []).append((int(i), int(off)))

    def expect(self):
        """want and fb from the oracle and the image before the call."""
        P = self.P
        self.want = self.cur.copy()
        self.fb = np.full(P.stripes, CLEAN, dtype=np.uint32)
        for s, S in enumerate(P.lens):
            X = [i for i in range(P.n) if self.er[s, i]]
            if S == 0 or P.m == 0 or not (s in self.flips or (self.repair and X)):
                continue  # nothing there | no parity | stored as coded, nothing to write
            R = r16(S)
            C, U = self.survivors(s), self.compared(s)
            word = oracle_codeword(P.k, P.n, [(i, self.cur[self.at(s, i):self.at(s, i) + R].tobytes()) for i in C])
            for i in U:
                bad = np.flatnonzero(self.cur[self.at(s, i):self.at(s, i) + S] != word[i][:S])
                if bad.size:
                    self.fb[s] = min(int(self.fb[s]), int(bad[0]))
            if self.repair:
                for i in X:
                    o = P.row_at(self.entry_row[s, i])
                    self.want[o:o + R] = word[i]
        return self

    # ---- the device
    def upload(self, torch):
        self.dev = torch.from_numpy(self.cur).cuda()
        self.host_table = (self.dev.data_ptr() + GUARD + self.entry_row.astype(np.int64) * self.P.row_bytes).reshape(-1)
        assert (self.host_table % 16 == 0).all()
        self.table = torch.from_numpy(self.host_table.copy()).cuda()
        self.first_bad = torch.full((self.P.stripes,), SENTINEL, dtype=torch.int32, device="cuda:0")
        return self

    def flags(self):
        return self.er.tobytes()

    def call(self, f, torch=None, erased="own"):
        """The _lens call over the image as it is now (uploads it when torch
        is given); returns first_bad."""
        if torch is not None:
            self.upload(torch)
        P = self.P
        if self.repair:
            f.reconstruct_checked_ptrs_lens(self.table.data_ptr(), P.lens, P.stripes, self.flags(), self.first_bad.data_ptr())
        else:
            f.verify_ptrs_lens(self.table.data_ptr(), P.lens, P.stripes, self.first_bad.data_ptr(),
                               erased=self.flags() if erased == "own" else erased)
        f.sync()
        return self.verdicts()

    def call_by_length(self, f, torch):
        """The only route without the _lens calls: for each distinct non-zero
        length, the equal-length call on a sub-table of the stripes of that
        length.  Returns first_bad, zero-length stripes CLEAN."""
        self.upload(torch)
        P = self.P
        out = np.full(P.stripes, CLEAN, dtype=np.uint32)
        for S in sorted(set(P.lens) - {0}):
            idx = [s for s in range(P.stripes) if P.lens[s] == S]
            sub = torch.from_numpy(self.host_table.reshape(P.stripes, P.n)[idx].reshape(-1).copy()).cuda()
            fb = torch.full((len(idx),), SENTINEL, dtype=torch.int32, device="cuda:0")
            if self.repair:
                f.reconstruct_checked_ptrs(sub.data_ptr(), S, len(idx), self.er[idx].tobytes(), fb.data_ptr())
            else:
                f.verify_ptrs(sub.data_ptr(), S, len(idx), fb.data_ptr(), erased=self.er[idx].tobytes())
            f.sync()
            out[idx] = fb.cpu().numpy().view(np.uint32)
        return out

    def verdicts(self):
        return self.first_bad.cpu().numpy().view(np.uint32)

    def image(self):
        return self.dev.cpu().numpy()

    def check(self, what="", want=None):
        want = self.want if want is None else want
        bad = np.flatnonzero(self.image() != want)
        assert bad.size == 0, f"{what} pool: {bad.size} bytes differ, first offsets {bad[:8].tolist()}"
        assert np.array_equal(self.table.cpu().numpy(), self.host_table), f"{what}: the table changed"

    def run(self, f, torch, what="", erased="own"):
        """expect, call, compare everything."""
        self.expect()
        got = self.call(f, torch, erased=erased)
        assert np.array_equal(got, self.fb), (what, self.P.lens, got.tolist(), self.fb.tolist())
        self.check(what)
        return got

"""Expected-image builder for rs_encode_ptrs, rs_update_ptrs and rs_read_ptrs
(test_gpu_ptrs_io.py; proven on the CPU in test_ptrs_io_model.py).  A plain
helper module: no fixtures, no GPU needed to import it.

A Scene is one flat ARENA of bytes: a strided_image.Pool (random rows, row
padding, decoys, guard bands) followed by the side buffers of a call -- the
src buffers of an update, the dst buffers of a read -- each behind a guard
band of its own.  Everything is random bytes.  An address is an offset into
the arena; an engine adds its base.  The TABLE holds, per (stripe, shard), the
offset of a pool row: the shard's own row, or a DECOY row for every entry a
call must not load, so that a mistake shows as a wrong byte or a changed
decoy, never as a fault.

A Case is a call with the arena and the table before it and the arena it must
leave behind; check() compares the WHOLE arena (pool, padding, decoys, guards,
every side buffer) and the table.  Expected bytes never come from the engine:
parity is the oracle's, over all round_up(S, 16) columns of a row (the calls
code the padding columns too, rsmi.h), an update's parity is the oracle's
encode of the new data, a read's bytes are the arena's before shards were lost.
"""
import numpy as np

from oracle import oracle
from strided_image import GUARD, r16

_MATRIX = {}


def matrix(k, n):
    if (k, n) not in _MATRIX:
        _MATRIX[(k, n)] = oracle.fec_matrix(k, n)
    return _MATRIX[(k, n)]


def parity_of(k, n, cols):
    """The oracle's m parity rows of k data rows: cols [k][W] -> [m][W]."""
    cols = np.ascontiguousarray(cols, dtype=np.uint8)
    if n == k or cols.shape[1] == 0:
        return np.zeros((n - k, cols.shape[1]), dtype=np.uint8)
    out = oracle.encode(matrix(k, n), k, n, cols.tobytes())
    return np.frombuffer(out, dtype=np.uint8).reshape(n - k, cols.shape[1])


class Scene:
    def __init__(self, P, seed):
        self.P, self.k, self.n, self.m, self.S = P, P.k, P.n, P.m, P.S
        self.W = r16(P.S)
        self.rng = np.random.default_rng(seed)
        pool = P.pristine[0].copy()
        # The pool's rows as codewords over all W columns: the oracle's parity
        # of the data rows' padding columns.
        if self.W > self.S:
            for s in range(P.stripes):
                pad = parity_of(self.k, self.n, np.stack([pool[self.at(s, c) + self.S:self.at(s, c) + self.W]
                                                          for c in range(self.k)]))
                for r in range(self.m):
                    pool[self.at(s, self.k + r) + self.S:self.at(s, self.k + r) + self.W] = pad[r]
        self.parts = [pool]
        self.size = len(pool)
        self.pool_len = len(pool)
        self.entry_row = P.rows.copy()  # the row each table entry names

    def at(self, s, i):
        """Arena offset of the real row of shard i of stripe s."""
        return self.P.row_at(self.P.rows[s, i])

    def alloc(self, nbytes):
        """A side buffer of round_up(nbytes, 16) random bytes behind the arena
        so far, a guard band behind it; its offset."""
        off = self.size
        blk = self.rng.integers(0, 256, size=r16(nbytes) + GUARD, dtype=np.uint8)
        self.parts.append(blk)
        self.size += len(blk)
        return off

    def arena(self):
        a = np.concatenate(self.parts)
        self.parts = [a]
        return a

    def decoy(self, s, i):
        self.entry_row[s, i] = self.P.decoys[int(self.rng.integers(len(self.P.decoys)))]

    def table(self):
        return (GUARD + self.entry_row.astype(np.int64) * self.P.row_bytes).reshape(-1)


class Case:
    def __init__(self, sc, op, init, want, **args):
        self.sc, self.op, self.init, self.want, self.args = sc, op, init, want, args
        self.table = sc.table()
        self.stripes = sc.P.stripes

    def run(self, engine):
        """(arena, table) after the call through `engine` (NpEngine's interface)."""
        return getattr(engine, self.op)(self.init.copy(), self.table.copy(), self.sc.S if "length" not in self.args
                                        else self.args["length"], self.stripes,
                                        **{k: v for k, v in self.args.items() if k != "length"})

    def check(self, got, what=""):
        arena, table = got
        assert arena.shape == self.want.shape, (what, arena.shape, self.want.shape)
        bad = np.flatnonzero(arena != self.want)
        assert bad.size == 0, (f"{what} {self.op}: {bad.size} bytes differ, first offsets {bad[:8].tolist()} "
                               f"(pool ends at {self.sc.pool_len})")
        assert np.array_equal(table, self.table), f"{what} {self.op}: the table changed"


def encode_case(P, seed):
    """Every parity row holds garbage over its whole pitch beforehand; after
    the call its first W bytes are the oracle's."""
    sc = Scene(P, seed)
    canon = sc.arena()
    init = canon.copy()
    for s in range(P.stripes):
        for i in range(sc.k, sc.n):
            init[sc.at(s, i):sc.at(s, i) + P.row_bytes] = sc.rng.integers(0, 256, size=P.row_bytes, dtype=np.uint8)
    want = init.copy()
    for s in range(P.stripes):
        for i in range(sc.k, sc.n):
            want[sc.at(s, i):sc.at(s, i) + sc.W] = canon[sc.at(s, i):sc.at(s, i) + sc.W]
    return Case(sc, "encode_ptrs", init, want)


def update_lists(P):
    """{stripe: [changed data shards]}: every third stripe untouched, one
    changed shard in the others, min(k, 3) in the last listed one."""
    listed = {s: [(s * 5 + 1) % P.k] for s in range(P.stripes) if s % 3 != 0 or P.stripes == 1}
    last = max(listed)
    listed[last] = sorted({(last + c * 7) % P.k for c in range(P.k)})[:min(P.k, 3)]
    return listed


def update_case(P, seed, listed=None, sl=None, decoys=True, arena=None, entry_row=None):
    """sl = (offset, length) of a slice update.  The table entries of the
    unchanged data shards of listed stripes and every entry of an unlisted
    stripe name decoys (decoys=False: their own rows).  arena / entry_row: the
    state an earlier call left (the life sequence)."""
    sc = Scene(P, seed)
    listed = update_lists(P) if listed is None else listed
    off, length = sl or (0, P.S)
    W = r16(length)
    assert off % 16 == 0 and off + W <= sc.W
    updates = [(s, c, sc.alloc(W)) for s in sorted(listed) for c in listed[s]]
    init = sc.arena()
    if arena is not None:
        init[:sc.pool_len] = arena[:sc.pool_len]
    if entry_row is not None:
        sc.entry_row = entry_row.copy()
    for s in range(P.stripes):
        for i in range(sc.n):
            if decoys and (s not in listed or (i < sc.k and i not in listed[s])):
                sc.decoy(s, i)
    want = init.copy()
    for s, c, src in updates:
        want[sc.at(s, c) + off:sc.at(s, c) + off + W] = init[src:src + W]
    for s in listed:
        par = parity_of(sc.k, sc.n, np.stack([want[sc.at(s, c) + off:sc.at(s, c) + off + W] for c in range(sc.k)]))
        for r in range(sc.m):
            want[sc.at(s, sc.k + r) + off:sc.at(s, sc.k + r) + off + W] = par[r]
    return Case(sc, "update_ptrs", init, want, length=length, updates=updates, offset=off)


def wanted(sc, er, s, everything):
    """The shards a read of stripe s asks for: its erased shards (all of them,
    or the first), a present data shard and a present parity shard."""
    gone = [i for i in range(sc.n) if er[s, i]]
    ids = gone if everything else gone[:1]
    ids += [i for i in range(sc.k) if not er[s, i]][:1]
    ids += [i for i in range(sc.n - 1, sc.k - 1, -1) if not er[s, i]][:1]
    return sorted(set(ids))


def read_case(P, seed, er, sl=None, overfull=None, arena=None):
    """er [stripes][n]: the erasure flags.  The rows of erased shards are
    overwritten with random bytes and their table entries name decoys.
    overfull: a stripe that gets m + 1 flags and wants present shards only."""
    sc = Scene(P, seed)
    er = np.array(er, dtype=np.uint8)
    off, length = sl or (0, P.S)
    W = r16(length)
    assert off % 16 == 0 and off + W <= sc.W and er.shape == (P.stripes, sc.n)
    if overfull is not None:
        er[overfull] = 0
        er[overfull, sc.rng.choice(sc.n, size=sc.m + 1, replace=False)] = 1
    reads = []
    for s in range(P.stripes):
        if s == overfull:
            ids = [i for i in range(sc.n) if not er[s, i]][:2]
        else:
            ids = wanted(sc, er, s, everything=s % 2 == 0)
        reads += [(s, i, sc.alloc(W)) for i in ids]
    canon = sc.arena()
    if arena is not None:
        canon[:sc.pool_len] = arena[:sc.pool_len]
    init = canon.copy()
    for s, i in zip(*np.nonzero(er)):
        init[sc.at(s, i):sc.at(s, i) + P.row_bytes] = sc.rng.integers(0, 256, size=P.row_bytes, dtype=np.uint8)
        sc.decoy(s, i)
    want = init.copy()
    for s, i, dst in reads:
        want[dst:dst + W] = canon[sc.at(s, i) + off:sc.at(s, i) + off + W]
    return Case(sc, "read_ptrs", init, want, length=length, erased=er, reads=reads, offset=off)


def rebuild_choice(k, n, er_row):
    """Rebuild's survivors: every present data share, then the highest present parity."""
    c = [i for i in range(k) if not er_row[i]]
    for i in range(n - 1, k - 1, -1):
        if len(c) < k and not er_row[i]:
            c.append(i)
    return sorted(c)

"""CPU: the expected-image builder of the pointer-placement I/O calls
(ptrs_io_model.py) against a numpy stand-in engine (np_rs, independent of the
oracle) -- and against stand-ins that each break one rule of rsmi.h, every one
of which the whole-arena comparison has to catch."""
import numpy as np
import pytest

import np_rs
from ptrs_io_model import encode_case, read_case, rebuild_choice, update_case
from strided_image import Pool, fixed_patterns, r16, random_erasures

CODES = [(4, 6), (10, 14), (3, 19), (4, 5), (1, 3), (3, 3)]
SHAPES = [(16, 1), (40, 3), (200, 4)]


class NpEngine:
    """rs_encode_ptrs / rs_update_ptrs / rs_read_ptrs as rsmi.h words them, on
    a numpy arena whose addresses are offsets.  Returns (arena, table)."""

    def __init__(self, k, n):
        self.k, self.n, self.m = k, n, n - k
        self.E = np_rs.fec_matrix(k, n)

    def encode_ptrs(self, arena, table, S, stripes):
        W, t = r16(S), table.reshape(stripes, self.n)
        for s in range(stripes):
            if self.m == 0:
                break
            par = np_rs.apply_rows(self.E[self.k:], np.stack([arena[t[s, c]:t[s, c] + W] for c in range(self.k)]))
            for r in range(self.m):
                self.store(arena, t[s, self.k + r], par[r])
        return arena, table

    def store(self, arena, at, row):
        arena[at:at + len(row)] = row

    def update_ptrs(self, arena, table, S, stripes, updates, offset):
        W, t = r16(S), table.reshape(stripes, self.n)
        o = self.offset(offset)
        for s, c, src in updates:
            old = arena[t[s, c] + o:t[s, c] + o + W].copy()
            new = arena[src:src + W].copy()
            for r in range(self.m):
                at = t[s, self.k + r] + o
                arena[at:at + W] ^= np_rs.MUL[self.E[self.k + r, c], old ^ new]
            arena[t[s, c] + o:t[s, c] + o + W] = new
        return arena, table

    def offset(self, offset):
        return offset

    def read_ptrs(self, arena, table, S, stripes, erased, reads, offset):
        W, t = r16(S), table.reshape(stripes, self.n)
        o = self.offset(offset)
        out = []
        for s, i, dst in reads:
            if not erased[s, i]:
                out.append((dst, arena[t[s, i] + o:t[s, i] + o + W].copy()))
                continue
            surv = rebuild_choice(self.k, self.n, erased[s])
            assert len(surv) == self.k
            inv = np_rs.invert(self.E[surv])
            row = np_rs.matmul(self.E[i:i + 1], inv)
            out.append((dst, np_rs.apply_rows(row, np.stack([arena[t[s, c] + o:t[s, c] + o + W] for c in surv]))[0]))
        for dst, v in out:
            arena[dst:dst + W] = v
        return arena, table


class PastPadding(NpEngine):
    """Writes one byte past round_up(S, 16) of a parity shard."""

    def store(self, arena, at, row):
        arena[at:at + len(row)] = row
        arena[at + len(row)] ^= 0xFF


class TouchesDecoy(NpEngine):
    """Dereferences the table entry of an unchanged data shard of a listed stripe."""

    def update_ptrs(self, arena, table, S, stripes, updates, offset):
        listed = {(s, c) for s, c, _ in updates}
        s = updates[0][0]
        other = next(i for i in range(self.k) if (s, i) not in listed)
        arena[table.reshape(stripes, self.n)[s, other]] ^= 1
        return super().update_ptrs(arena, table, S, stripes, updates, offset)


class WritesUnlisted(NpEngine):
    """Copies the new contents into the slot of a data shard nobody listed too."""

    def update_ptrs(self, arena, table, S, stripes, updates, offset):
        listed = {(s, c) for s, c, _ in updates}
        s, c = next((s, c) for s in range(stripes) for c in range(self.k) if (s, c) not in listed)
        at = table.reshape(stripes, self.n)[s, c]
        arena[at:at + 16] = arena[updates[0][2]:updates[0][2] + 16] ^ 0x5A
        return super().update_ptrs(arena, table, S, stripes, updates, offset)


class IgnoresOffset(NpEngine):
    def offset(self, offset):
        return 0


class WritesPresent(NpEngine):
    """Stores into a present shard's slot during a read."""

    def read_ptrs(self, arena, table, S, stripes, erased, reads, offset):
        s, i = next((s, i) for s, i, _ in reads if not erased[s, i])
        arena[table.reshape(stripes, self.n)[s, i] + offset] ^= 0x80
        return super().read_ptrs(arena, table, S, stripes, erased, reads, offset)


def pool(k, n, S, stripes):
    return Pool(k, n, S, stripes, seed=k * 131 + n * 17 + S + stripes)


def erasures(P, seed):
    if P.m == 0:
        return np.zeros((P.stripes, P.n), dtype=np.uint8)
    fx = fixed_patterns(P.k, P.n)
    rnd = random_erasures(np.random.default_rng(seed), P.stripes, P.n, P.m)
    return np.stack([fx[(s // 2) % len(fx)] if s % 2 == 0 else rnd[s] for s in range(P.stripes)])


def slices(S):
    """The slice to the shard's end and a middle multiple of 16, where S has room."""
    out = [None]
    if S > 16:
        out.append((16, S - 16))
    if S >= 64:
        out.append((16, 32))
    return out


@pytest.mark.parametrize("k,n", CODES)
@pytest.mark.parametrize("S,stripes", SHAPES)
def test_model_agrees_with_stand_in(k, n, S, stripes):
    P, eng = pool(k, n, S, stripes), NpEngine(k, n)
    case = encode_case(P, 1)
    case.check(case.run(eng), "encode")
    for sl in slices(S):
        case = update_case(P, 2, sl=sl)
        case.check(case.run(eng), f"update {sl}")
        case = read_case(P, 3, erasures(P, 5), sl=sl, overfull=1 if stripes >= 3 else None)
        case.check(case.run(eng), f"read {sl}")
    case = read_case(P, 4, erasures(P, 6), overfull=0)
    case.check(case.run(eng), "read, overfull stripe")


def test_update_decoys_cover_every_entry_not_loaded():
    P = pool(4, 6, 40, 4)
    case = update_case(P, 2)
    rows = case.sc.entry_row
    decoys = set(P.decoys.tolist())
    listed = {(s, c) for s, c, _ in case.args["updates"]}
    for s in range(P.stripes):
        for i in range(P.n):
            loaded = (s, i) in listed or (i >= P.k and any(t == s for t, _ in listed))
            assert (rows[s, i] in decoys) == (not loaded), (s, i)


@pytest.mark.parametrize("broken,build", [
    (PastPadding, lambda P: encode_case(P, 1)),
    (TouchesDecoy, lambda P: update_case(P, 2)),
    (WritesUnlisted, lambda P: update_case(P, 2, decoys=False)),
    (IgnoresOffset, lambda P: update_case(P, 2, sl=(16, 16))),
    (IgnoresOffset, lambda P: read_case(P, 3, erasures(P, 5), sl=(16, 16))),
    (WritesPresent, lambda P: read_case(P, 3, erasures(P, 5))),
])
@pytest.mark.parametrize("k,n", [(4, 6), (10, 14), (3, 19)])
def test_comparison_catches_a_broken_engine(k, n, broken, build):
    P = pool(k, n, 40, 4)
    case = build(P)
    case.check(case.run(NpEngine(k, n)), "sound engine")
    with pytest.raises(AssertionError):
        case.check(case.run(broken(k, n)), broken.__name__)

"""CPU: the store-life driver, its scenarios and its ledger, proven without a
GPU (test_gpu_store_life.py runs the same driver against the engine).

Naive is a second host implementation of the method set of
store_model.Model, deliberately plain: every stripe is decoded to its k data
rows by a Gauss-Jordan inverse and every shard is evaluated from them, shard
by shard, with np_rs' table arithmetic; the column decoder is a
Berlekamp-Welch of its own over np_rs' Vandermonde points, one column at a
time.  It shares the Memory plumbing with the model: no addressing, no flag
parsing, no call semantics.  Up to 64 inconsistent columns of a stripe are
decoded one by one; beyond that (whole-shard damage) Berlekamp-Welch runs on
columns until k shards have been right throughout, and their codeword is taken
wherever it lies within the radius, where it is the unique one.

The seven scenarios with k * S > 100,000 run here in the "every" granularity
only, five of them at a reduced S, so their draws differ from the GPU run's:
the ledger conditions proven here are not those of these scenarios as
test_gpu_store_life.py runs them, whose own test_ledger checks them there.

The driver runs with Naive in the engine's place: every scenario must agree,
end in codewords that equal the remembered truth, and satisfy the coverage
ledger.  Then thirteen defects are injected into Naive one at a time, and the
driver must report a mismatch for each in at least one scenario.
"""
import struct

import numpy as np
import pytest

import np_rs
import store_model as sm
from store_model import CLEAN, RS_EINVAL, RS_ENOT_ENOUGH, RS_ETOO_MANY_ERRORS, RS_OK, Refused
from strided_image import r16

SCENARIOS = sm.scenarios()
MUL = np_rs.MUL

MUTANTS = {
    1: "a byte written into a stride gap",
    2: "the pad-to-16 of a present shard written",
    3: "first_bad one too high",
    4: "first_bad not the minimum over shards",
    5: "Rebuild picks the lowest present parity",
    6: "read_stripes regenerates a present shard",
    7: "update_degraded writes the slot of an erased changed shard",
    8: "update_degraded patches an erased parity slot",
    9: "correct_columns works on bytes at offsets >= S",
    10: "the last 16-byte column dropped when ceil(S/16) % 256 == 1",
    11: "one stripe uses the previous call's erasure pattern",
    12: "checked repair fills a slot from the truth",
    13: "rewritten / corrected reported for an erased shard",
}


def solve(A, b):
    """One solution of A x = b over GF(2^8) (free unknowns 0), or None."""
    A = np.concatenate([np.asarray(A, dtype=np.uint8), np.asarray(b, dtype=np.uint8)[:, None]], axis=1)
    rows, cols = A.shape[0], A.shape[1] - 1
    where, r = [], 0
    for c in range(cols):
        piv = next((q for q in range(r, rows) if A[q, c]), None)
        if piv is None:
            continue
        A[[r, piv]] = A[[piv, r]]
        A[r] = MUL[np_rs.ginv(int(A[r, c])), A[r]]
        f = A[:, c].copy()
        f[r] = 0
        A ^= MUL[f[:, None], A[r][None, :]]
        where.append(c)
        r += 1
        if r == rows:
            break
    if A[r:, cols].any():
        return None
    x = np.zeros(cols, dtype=np.uint8)
    x[where] = A[:len(where), cols]
    return x


class Naive(sm.HostEngine):
    def __init__(self, k, n, mem, mutant=0):
        super().__init__(k, n, mem)
        self.E = np_rs.fec_matrix(k, n)
        self.V = np_rs.vandermonde(n, k)
        self.X = [np_rs.point(i) for i in range(n)]
        self.mutant, self.prev, self.truth, self.inverses = mutant, None, None, {}

    # ---- arithmetic ------------------------------------------------------------
    def strided(self, data, dss, parity, pss, pitch):
        def slot(s, i):
            base, stride, j = (data, dss, i) if i < self.k else (parity, pss, i - self.k)
            return base + stride * s + pitch * j
        return slot

    def table(self, tab, stripes):
        entries = struct.unpack(f"<{stripes * self.n}q", bytes(self.mem.view(tab, 8 * stripes * self.n)))
        return lambda s, i: entries[s * self.n + i]

    def flags(self, erased, stripes):
        er = np.array([[1 if erased is not None and erased[s * self.n + i] else 0 for i in range(self.n)]
                       for s in range(stripes)], dtype=np.uint8).reshape(stripes, self.n)
        if self.mutant == 11 and self.prev is not None and self.prev.shape == er.shape:
            er[-1], self.prev = self.prev[-1], er.copy()
        elif erased is not None:
            self.prev = er.copy()
        return er

    def pick(self, er):
        """Rebuild: the present data shards, then parity from the top, each
        erased data slot taking the next one."""
        if int((er != 0).sum()) > self.m:
            raise Refused(RS_ENOT_ENOUGH)
        par = [i for i in range(self.n - 1, self.k - 1, -1) if not er[i]]
        if self.mutant == 5:
            par.reverse()
        return [i if not er[i] else par.pop(0) for i in range(self.k)]

    def data_of(self, slot, s, er, length):
        """The k data rows of the codeword through Rebuild's survivors as stored."""
        ids = self.pick(er)
        vals = np.stack([self.mem.view(slot(s, i), length) for i in ids])
        if ids == list(range(self.k)):
            return ids, vals
        return ids, np_rs.apply_rows(self.inverse(ids), vals)

    def inverse(self, ids):
        if tuple(ids) not in self.inverses:
            self.inverses[tuple(ids)] = np_rs.invert(self.E[list(ids)])
        return self.inverses[tuple(ids)]

    def shard(self, data, i):
        return np_rs.apply_rows(self.E[i:i + 1], data)[0]

    def put(self, addr, v, S):
        R = r16(S)
        if self.mutant == 10 and (R // 16) % 256 == 1:
            R -= 16
        self.mem.view(addr, R)[:] = v[:R]

    def bw(self, ids, y, t):
        """Berlekamp-Welch for one column: the codeword within t of the shares
        y of shards ids, as its values at all n points, or None."""
        r, k = len(ids), self.k
        A = np.zeros((r, k + 2 * t), dtype=np.uint8)
        b = np.zeros(r, dtype=np.uint8)
        for row, (i, yi) in enumerate(zip(ids, y)):
            p = 1
            for q in range(k + t):
                A[row, q] = p
                if q < t:
                    A[row, k + t + q] = MUL[int(yi), p]
                if q == t:
                    b[row] = MUL[int(yi), p]
                p = int(MUL[p, self.X[i]])
        x = solve(A, b)
        if x is None:
            return None
        Q, loc = [int(v) for v in x[:k + t]], [int(v) for v in x[k + t:]] + [1]
        P = [0] * k
        for d in range(k + t - 1, t - 1, -1):
            c = Q[d]
            P[d - t] = c
            for j in range(t + 1):
                Q[d - t + j] ^= int(MUL[c, loc[j]])
        if any(Q):
            return None
        word = np_rs.matmul(self.V, np.array(P, dtype=np.uint8)[:, None])[:, 0]
        return word if int((word[ids] != np.asarray(y)).sum()) <= t else None

    def word(self, slot, s, er, length, cols):
        """The codeword at the columns cols, (present ids, [present][cols]) or
        None: column by column by Berlekamp-Welch; past 64 columns, k shards
        that were right so far are tried on the rest."""
        pres = [i for i in range(self.n) if not er[i]]
        t = (len(pres) - self.k) // 2
        y = np.stack([self.mem.view(slot(s, i), length)[cols] for i in pres])
        out, left, suspects = np.zeros_like(y), list(range(len(cols))), set()
        while left:
            c = left.pop(0)
            w = self.bw(pres, y[:, c], t)
            if w is None:
                return None
            out[:, c] = w[pres]
            suspects |= {j for j in range(len(pres)) if out[j, c] != y[j, c]}
            good = [j for j in range(len(pres)) if j not in suspects][:self.k]
            if len(cols) <= 64 or len(left) < 4 or len(good) < self.k:
                continue
            data = np_rs.apply_rows(self.inverse([pres[j] for j in good]), y[good][:, left])
            cand = np_rs.apply_rows(self.E[pres], data)
            ok = (cand != y[:, left]).sum(axis=0) <= t
            for q, c in enumerate(left):
                if ok[q]:
                    out[:, c] = cand[:, q]
            left = [c for q, c in enumerate(left) if not ok[q]]
        return pres, out

    def first_bad(self, slot, s, er, length, limit):
        """(verdict, the columns below limit at which a compared shard differs)."""
        ids, data = self.data_of(slot, s, er, length)
        fb, cols = CLEAN, set()
        for i in range(self.k, self.n):
            if er[i] or i in ids:
                continue
            bad = np.flatnonzero(self.shard(data, i)[:limit] != self.mem.view(slot(s, i), limit))
            if bad.size:
                fb = int(bad[0]) if self.mutant == 4 else min(fb, int(bad[0]))
                cols |= set(bad.tolist())
        if self.mutant == 3 and fb != CLEAN:
            fb += 1
        return fb, np.array(sorted(cols), dtype=np.int64)

    # ---- the calls ---------------------------------------------------------------
    def _gap(self, slot, s, pitch):
        if self.mutant == 1:
            self.mem.view(slot(s, self.n - 1) + pitch, 1)[:] ^= 0x80

    def encode_stripes(self, data, dss, parity, pss, pitch, S, stripes):
        slot = self.strided(data, dss, parity, pss, pitch)
        for s in range(stripes):
            d = np.stack([self.mem.view(slot(s, c), r16(S)) for c in range(self.k)])
            for i in range(self.k, self.n):
                self.put(slot(s, i), self.shard(d, i), S)
            self._gap(slot, s, pitch)

    def _verify(self, slot, S, stripes, er, first_bad):
        for s in range(stripes):
            self.pick(er[s])
        out = self.mem.view(first_bad, 4 * stripes).view(np.uint32) if S and stripes else []
        for s in range(len(out)):
            out[s] = self.first_bad(slot, s, er[s], S, S)[0]

    def verify_stripes(self, data, dss, parity, pss, pitch, S, stripes, first_bad):
        self._verify(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(None, stripes), first_bad)

    def verify_degraded(self, data, dss, parity, pss, pitch, S, stripes, erased, first_bad):
        self._verify(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes), first_bad)

    def verify_ptrs(self, tab, S, stripes, first_bad, erased=None):
        self._verify(self.table(tab, stripes), S, stripes, self.flags(erased, stripes), first_bad)

    def _rebuild(self, slot, S, stripes, er, first_bad=None, pitch=None):
        for s in range(stripes):
            self.pick(er[s])
        if not S:
            return
        for s in range(stripes):
            if first_bad is not None:
                self.mem.view(first_bad, 4 * stripes).view(np.uint32)[s] = self.first_bad(slot, s, er[s], S, S)[0]
            if not er[s].any():
                continue
            ids, data = self.data_of(slot, s, er[s], r16(S))
            for i in np.flatnonzero(er[s]):
                v = self.shard(data, int(i))
                if self.mutant == 12 and first_bad is not None:
                    v[:S] = self.truth(s, int(i))
                self.put(slot(s, int(i)), v, S)
            if self.mutant == 2 and r16(S) > S:
                self.mem.view(slot(s, ids[0]) + S, r16(S) - S)[:] ^= 0xEE
            if pitch:
                self._gap(slot, s, pitch)

    def reconstruct_stripes(self, data, dss, parity, pss, pitch, S, stripes, erased):
        self._rebuild(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes), pitch=pitch)

    def reconstruct_ptrs(self, tab, S, stripes, erased):
        self._rebuild(self.table(tab, stripes), S, stripes, self.flags(erased, stripes))

    def reconstruct_checked(self, data, dss, parity, pss, pitch, S, stripes, erased, first_bad):
        self._rebuild(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes), first_bad,
                      pitch)

    def reconstruct_checked_ptrs(self, tab, S, stripes, erased, first_bad):
        self._rebuild(self.table(tab, stripes), S, stripes, self.flags(erased, stripes), first_bad)

    def _scrub(self, slot, S, stripes, er, by_column):
        for s in range(stripes):
            self.pick(er[s])
        status = [RS_OK] * stripes
        marks = [0] * (stripes * self.n)
        if by_column and self.m > 16 and S and stripes:
            raise Refused(RS_EINVAL)
        length = r16(S) if by_column and self.mutant == 9 else S
        for s in range(stripes if S and self.m else 0):
            fb, cols = self.first_bad(slot, s, er[s], length, length)
            if fb == CLEAN:
                continue
            if self.mutant == 13 and er[s].any():
                marks[s * self.n + int(np.flatnonzero(er[s])[0])] = 1
            found = self.word(slot, s, er[s], length, cols) if self.m - int(er[s].sum()) >= 2 else None
            if found is None:
                status[s] = RS_ETOO_MANY_ERRORS
                continue
            pres, w = found
            t = (len(pres) - self.k) // 2
            wrong = [i for j, i in enumerate(pres) if (w[j] != self.mem.view(slot(s, i), length)[cols]).any()]
            if not by_column and len(wrong) > t:
                status[s] = RS_ETOO_MANY_ERRORS
                continue
            for j, i in enumerate(pres):
                stored = self.mem.view(slot(s, i), length)
                diff = int((stored[cols] != w[j]).sum())
                if diff:
                    stored[cols] = w[j]
                    marks[s * self.n + i] = diff if by_column else 1
        return status, marks if by_column else bytes(marks)

    def correct_columns(self, data, dss, parity, pss, pitch, S, stripes, erased=None):
        return self._scrub(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes), True)

    def correct_columns_ptrs(self, tab, S, stripes, erased=None):
        return self._scrub(self.table(tab, stripes), S, stripes, self.flags(erased, stripes), True)

    def correct_stripes(self, data, dss, parity, pss, pitch, S, stripes):
        return self._scrub(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(None, stripes), False)

    def correct_degraded(self, data, dss, parity, pss, pitch, S, stripes, erased):
        return self._scrub(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes), False)

    def update_stripes(self, data, dss, parity, pss, pitch, S, stripes, updates):
        self._update(self.strided(data, dss, parity, pss, pitch), S, np.zeros((stripes, self.n), dtype=np.uint8),
                     updates)

    def update_degraded(self, data, dss, parity, pss, pitch, S, stripes, erased, updates):
        self._update(self.strided(data, dss, parity, pss, pitch), S, self.flags(erased, stripes), updates)

    def _update(self, slot, S, er, updates):
        R = r16(S)
        for s, c, _ in updates:
            if er[s, c]:
                self.pick(er[s])
        if not S:
            return
        old = {}
        for s, c, _ in updates:     # the old contents first: the survivors as they were
            if er[s, c]:
                old[(s, c)] = self.shard(self.data_of(slot, s, er[s], R)[1], c)
            else:
                old[(s, c)] = self.mem.view(slot(s, c), R).copy()
        for s, c, src in updates:
            new = self.mem.view(src, R).copy()
            delta = old[(s, c)] ^ new
            for i in range(self.k, self.n):
                if not er[s, i] or self.mutant == 8:
                    self.mem.view(slot(s, i), R)[:] ^= MUL[int(self.E[i, c]), delta]
            if not er[s, c] or self.mutant == 7:
                self.mem.view(slot(s, c), R)[:] = new

    def read_stripes(self, data, dss, parity, pss, pitch, S, stripes, erased, reads):
        slot, er, R = self.strided(data, dss, parity, pss, pitch), self.flags(erased, stripes), r16(S)
        for s, i, _ in reads:
            if er[s, i]:
                self.pick(er[s])
        for s, i, dst in reads if S else []:
            row = er[s].copy()
            if self.mutant == 6 and int(row.sum()) < self.m:
                row[i] = 1
            if row[i]:
                self.mem.view(dst, R)[:] = self.shard(self.data_of(slot, s, row, R)[1], i)
            else:
                self.mem.view(dst, R)[:] = self.mem.view(slot(s, i), R)

    def combine(self, jobs, length):
        R, done = r16(length), []
        for src, dst, coef, acc in jobs if length else []:
            coef = list(bytes(coef))
            for r, d in enumerate(dst):
                v = self.mem.view(d, R).copy() if acc else np.zeros(R, dtype=np.uint8)
                for c, a in enumerate(src):
                    v ^= MUL[coef[r * len(src) + c], self.mem.view(a, R)]
                done.append((d, v))
        for d, v in done:
            self.mem.view(d, R)[:] = v

    def pattern_rows(self, erased):
        er = np.frombuffer(bytes(erased), dtype=np.uint8)
        inv = self.inverse(self.pick(er))
        gone = [i for i in range(self.n) if er[i]]
        rows = [inv[i] if i < self.k else np_rs.matmul(self.E[i:i + 1], inv)[0] for i in gone]
        return b"".join(bytes(r) for r in rows), len(gone)

    def pattern_survivors(self, erased):
        return self.pick(np.frombuffer(bytes(erased), dtype=np.uint8))


# The naive engine is slow where k * S is large: those scenarios run at a
# reduced S here (one that is as ragged), never 16, 17 or 4112, and in the
# "every" granularity only; on the GPU they run as they are.
REDUCED = {12328: 88, 5000: 200, 4096: 256}


def slow(scenario):
    return scenario[1] * scenario[3] > 100000


def run(scenario, gran, mutant=0):
    ident, k, n, S, stripes, placement, seed = scenario
    if slow(scenario):
        S = REDUCED.get(S, S)
    holder = {}

    def make(k, n, names, arrays):
        holder["e"] = Naive(k, n, sm.Memory(names, arrays, bases=[(b + 5) << 40 for b in range(len(arrays))]), mutant)
        return holder["e"]
    d = sm.Driver(make, k, n, S, stripes, placement, seed, gran, ident=("cpu", ident, gran, mutant))
    holder["e"].truth = lambda s, i: d.truth[s, i]
    return d.run()


@pytest.mark.parametrize("scenario,gran",
                         [(x, g) for x in SCENARIOS for g in ("every", "async") if g == "every" or not slow(x)],
                         ids=lambda v: v[0] if isinstance(v, tuple) else v)
def test_agreement_invariants_and_ledger(scenario, gran):
    """The naive engine and the model agree on every byte of every scenario;
    Driver.finish() has checked the codeword invariants (every [0, S) the
    remembered truth, np_rs' re-encoding of the data the stored parity); the
    ledger's conditions hold."""
    ident, k, n, _, stripes, placement, _ = scenario
    d = run(scenario, gran)
    assert not d.er.any()
    sm.check_ledger(("cpu", ident, gran, 0), k, n, stripes, placement == "ptrs")


def test_scenarios_cover_the_sizes_and_codes():
    assert {x[3] for x in SCENARIOS} == set(sm.SIZES)
    for shapes in sm.FIXED.values():
        assert len(shapes) == 2 and any(S % 16 for S, _, _ in shapes)
    assert all(1 <= x[4] <= 6 for x in SCENARIOS)
    drawn = [x for x in SCENARIOS if x[0].startswith("seed")]
    assert len(drawn) == 6 and all(1 <= x[1] <= 72 and 1 <= x[2] - x[1] <= 20 for x in drawn)


# The scenarios a mutant is tried on, cheapest first; it is caught when the
# driver reports a mismatch for any of them.
MUTANT_SCENARIOS = [x for x in SCENARIOS if x[1] <= 13 and x[3] <= 5000]


@pytest.mark.parametrize("mutant", sorted(MUTANTS),
                         ids=[f"{q}-{MUTANTS[q].replace(' ', '_')}" for q in sorted(MUTANTS)])
def test_mutant_is_caught(mutant):
    caught = []
    for scenario in MUTANT_SCENARIOS:
        try:
            run(scenario, "every", mutant)
        except sm.Mismatch as x:
            caught.append((scenario[0], str(x)[:200]))
            break
    assert caught, f"mutant {mutant} ({MUTANTS[mutant]}) survived {len(MUTANT_SCENARIOS)} scenarios"

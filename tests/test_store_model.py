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

The scenarios of store_model_io.py (scattered-shard I/O over a per-call table
with decoys, a length per stripe, a checksum table kept through the whole
life) run the same way; for them Naive has the eleven calls they add, its
CRC-32C bit by bit, and fourteen more defects (14 to 27) that those scenarios
must report.  The model's own CRC-32C is pinned to RFC 3720 here.
"""
import struct

import numpy as np
import pytest

import np_rs
import store_model as sm
import store_model_io as io
from store_model import CLEAN, RS_EINVAL, RS_ENOT_ENOUGH, RS_ETOO_MANY_ERRORS, RS_OK, Refused
from strided_image import r16

SCENARIOS = sm.scenarios()
IO_SCENARIOS = io.scenarios_io()
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
    # the scenarios of store_model_io.py
    14: "a checksum covers the pad up to 16",
    15: "the checksum of the last, ragged sector taken over a full sector",
    16: "the checksum compute writes the row of an erased shard",
    17: "the checksum check reports the highest bad sector",
    18: "the checksum check writes a verdict other than clean for an erased shard",
    19: "correct_crc32c regenerates from survivors chosen for X, not X + B",
    20: "correct_crc32c skips the second check",
    21: "update_ptrs ignores offset for the parity slots",
    22: "update_ptrs reads an unlisted data entry",
    23: "read_ptrs writes the slot the table names, not dst",
    24: "a _lens call treats stripe s at the length of stripe s - 1",
    25: "a _lens call compares bytes in [L, round_up(L, 16))",
    26: "a zero-length stripe gets first_bad 0",
    27: "shard_lens read after the call returned",
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
        self.pending = []

    # ---- arithmetic ------------------------------------------------------------
    def strided(self, data, dss, parity, pss, pitch):
        def slot(s, i):
            base, stride, j = (data, dss, i) if i < self.k else (parity, pss, i - self.k)
            return base + stride * s + pitch * j
        slot.table = False
        return slot

    def table(self, tab, stripes):
        entries = struct.unpack(f"<{stripes * self.n}q", bytes(self.mem.view(tab, 8 * stripes * self.n)))
        self.flush()

        def slot(s, i, offset=0):
            return entries[s * self.n + i] + offset
        slot.table = True
        return slot

    def flags(self, erased, stripes):
        self.flush()
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
        """The codeword at the columns cols, (present ids, [present][cols],
        the columns without one within the radius, which keep their bytes):
        column by column by Berlekamp-Welch; past 64 columns, k shards that
        were right so far are tried on the rest."""
        pres = [i for i in range(self.n) if not er[i]]
        t = (len(pres) - self.k) // 2
        y = np.stack([self.mem.view(slot(s, i), length)[cols] for i in pres])
        out, left, suspects, lost = np.zeros_like(y), list(range(len(cols))), set(), []
        while left:
            c = left.pop(0)
            w = self.bw(pres, y[:, c], t)
            if w is None:
                out[:, c] = y[:, c]
                lost.append(c)
                continue
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
        return pres, out, lost

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
            if found is None or (found[2] and not by_column):
                status[s] = RS_ETOO_MANY_ERRORS
                continue
            pres, w, lost = found
            if lost:    # left alone while the others are corrected
                status[s] = RS_ETOO_MANY_ERRORS
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
        self._read(self.strided(data, dss, parity, pss, pitch), S, self.flags(erased, stripes), reads)

    def _read(self, slot, S, er, reads):
        R = r16(S)
        for s, i, _ in reads:
            if er[s, i]:
                self.pick(er[s])
        for s, i, dst in reads if S else []:
            row = er[s].copy()
            if self.mutant == 6 and int(row.sum()) < self.m:
                row[i] = 1
            if row[i]:
                if self.mutant == 23 and slot.table:
                    dst = slot(s, i)
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

    # ---- scattered-shard I/O -----------------------------------------------------
    def moved(self, at, offset, parity_too=True):
        def slot(s, i):
            return at(s, i) + (offset if i < self.k or parity_too else 0)
        slot.table = True
        return slot

    def encode_ptrs(self, tab, S, stripes):
        slot = self.table(tab, stripes)
        for s in range(stripes if self.m and S else 0):
            d = np.stack([self.mem.view(slot(s, c), r16(S)) for c in range(self.k)])
            for i in range(self.k, self.n):
                self.put(slot(s, i), self.shard(d, i), S)

    def update_ptrs(self, tab, S, stripes, updates, offset=0):
        slot = self.moved(self.table(tab, stripes), offset, self.mutant != 21)
        self._update(slot, S, np.zeros((stripes, self.n), dtype=np.uint8), updates)
        if self.mutant == 22 and S:     # the parity once more, from all k data entries of the table
            for s in sorted({s for s, _, _ in updates}):
                d = np.stack([self.mem.view(slot(s, c), r16(S)) for c in range(self.k)])
                for i in range(self.k, self.n):
                    self.put(slot(s, i), self.shard(d, i), S)

    def read_ptrs(self, tab, S, stripes, erased, reads, offset=0):
        self._read(self.moved(self.table(tab, stripes), offset), S, self.flags(erased, stripes), reads)

    # ---- a length per stripe -----------------------------------------------------
    def flush(self):
        todo, self.pending = self.pending, []
        for fn in todo:
            fn()

    def sync(self):
        self.flush()

    def snapshot(self):
        self.flush()
        return super().snapshot()

    def poke(self, buf, off, data):
        self.flush()
        super().poke(buf, off, data)

    def xor(self, buf, off, data):
        self.flush()
        super().xor(buf, off, data)

    def lens_of(self, tab, shard_lens, stripes, erased):
        er, at = self.flags(erased, stripes), self.table(tab, stripes)
        for s in range(stripes):
            self.pick(er[s])
        lens = [int(shard_lens[s]) for s in range(stripes)]
        if self.mutant == 24:
            lens = lens[:1] + lens[:-1]
        return lens, er, at

    def alone(self, at, s):
        def slot(_, i):
            return at(s, i)
        slot.table = True
        return slot

    def empty(self, first_bad, s):
        self.mem.view(first_bad + 4 * s, 4).view(np.uint32)[0] = 0 if self.mutant == 26 else CLEAN

    def verify_ptrs_lens(self, tab, shard_lens, stripes, first_bad, erased=None):
        if self.mutant == 27:
            # the work happens when the stream gets to it, and reads the lengths
            # then: lengths no call accepts leave everything unwritten
            self.flags(erased, stripes)
            flags = None if erased is None else bytes(erased)

            def later():
                if all(int(x) < 1 << 32 for x in shard_lens):
                    self.mutant = 0
                    self.verify_ptrs_lens(tab, shard_lens, stripes, first_bad, flags)
                    self.mutant = 27
            self.pending.append(later)
            return
        lens, er, at = self.lens_of(tab, shard_lens, stripes, erased)
        for s in range(stripes if any(lens) else 0):
            if not lens[s]:
                self.empty(first_bad, s)
                continue
            limit = r16(lens[s]) if self.mutant == 25 else lens[s]
            self.mem.view(first_bad + 4 * s, 4).view(np.uint32)[0] = self.first_bad(at, s, er[s], limit, limit)[0]

    def reconstruct_checked_ptrs_lens(self, tab, shard_lens, stripes, erased, first_bad):
        lens, er, at = self.lens_of(tab, shard_lens, stripes, erased)
        for s in range(stripes if any(lens) else 0):
            if lens[s]:
                self._rebuild(self.alone(at, s), lens[s], 1, er[s:s + 1], first_bad + 4 * s)
            else:
                self.empty(first_bad, s)

    def correct_columns_ptrs_lens(self, tab, shard_lens, stripes, erased=None):
        lens, er, at = self.lens_of(tab, shard_lens, stripes, erased)
        status, marks = [], []
        for s in range(stripes):
            st, mk = self._scrub(self.alone(at, s), lens[s] if self.m else 0, 1, er[s:s + 1], True)
            status += st
            marks += mk
        return status, marks

    # ---- sector checksums --------------------------------------------------------
    CRCS = {}

    def crc(self, message):
        """CRC-32C bit by bit: the message's bits, lowest first, through the
        reflected polynomial."""
        key = bytes(message)
        if key not in self.CRCS:
            if len(self.CRCS) > 4096:
                self.CRCS.clear()
            c = 0xFFFFFFFF
            for byte in key:
                c ^= byte
                for _ in range(8):
                    c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
            self.CRCS[key] = c ^ 0xFFFFFFFF
        return self.CRCS[key]

    def sums(self, addr, S, sector):
        out = []
        for lo in range(0, S, sector):
            hi = min(lo + sector, S)
            if hi == S and self.mutant == 14:
                hi = min(lo + sector, r16(S))
            if hi == S and self.mutant == 15:
                hi = min(lo + sector, r16(S) + 32)
            out.append(self.crc(self.mem.view(addr + lo, hi - lo)))
        return out

    def entries(self, crcs, x, crc_pitch, count):
        return self.mem.view(crcs + 4 * x * crc_pitch, 4 * count).view(np.uint32)

    def crc_store(self, slot, S, stripes, er, sector, crcs, crc_pitch):
        for s in range(stripes if S else 0):
            for i in range(self.n):
                if not er[s, i] or self.mutant == 16:
                    c = self.sums(slot(s, i), S, sector)
                    self.entries(crcs, s * self.n + i, crc_pitch, len(c))[:] = c

    def bad_sectors(self, addr, S, sector, crcs, x, crc_pitch):
        c = self.sums(addr, S, sector)
        return [j for j, (a, b) in enumerate(zip(c, self.entries(crcs, x, crc_pitch, len(c)))) if a != int(b)]

    def crc_check(self, slot, S, stripes, er, sector, crcs, crc_pitch, first_bad):
        out = self.mem.view(first_bad, 4 * stripes * self.n).view(np.uint32) if S and stripes else []
        for x in range(len(out)):
            s, i = divmod(x, self.n)
            if er[s, i]:
                out[x] = 0 if self.mutant == 18 else CLEAN
                continue
            bad = self.bad_sectors(slot(s, i), S, sector, crcs, x, crc_pitch)
            out[x] = CLEAN if not bad else bad[-1] if self.mutant == 17 else bad[0]

    def crc32c_stripes(self, data, dss, parity, pss, pitch, S, stripes, sector, crcs, crc_pitch, erased=None):
        self.crc_store(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes), sector,
                       crcs, crc_pitch)

    def crc32c_ptrs(self, tab, S, stripes, sector, crcs, crc_pitch, erased=None):
        self.crc_store(self.table(tab, stripes), S, stripes, self.flags(erased, stripes), sector, crcs, crc_pitch)

    def crc32c_check_stripes(self, data, dss, parity, pss, pitch, S, stripes, sector, crcs, crc_pitch, first_bad,
                             erased=None):
        self.crc_check(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes), sector,
                       crcs, crc_pitch, first_bad)

    def crc32c_check_ptrs(self, tab, S, stripes, sector, crcs, crc_pitch, first_bad, erased=None):
        self.crc_check(self.table(tab, stripes), S, stripes, self.flags(erased, stripes), sector, crcs, crc_pitch,
                       first_bad)

    def correct_crc32c(self, data, dss, parity, pss, pitch, S, stripes, sector, crcs, crc_pitch, erased=None):
        slot, er = self.strided(data, dss, parity, pss, pitch), self.flags(erased, stripes)
        status, rewritten = [RS_OK] * stripes, [0] * (stripes * self.n)
        bad = {s: [i for i in range(self.n) if not er[s, i] and
                   self.bad_sectors(slot(s, i), S, sector, crcs, s * self.n + i, crc_pitch)]
               for s in range(stripes if S else 0)}
        if any(b and int(er[s].sum()) > self.m for s, b in bad.items()):
            raise Refused(RS_ENOT_ENOUGH)
        for s, b in bad.items():
            if not b:
                continue
            if int(er[s].sum()) + len(b) > self.m:
                status[s] = RS_ETOO_MANY_ERRORS
                continue
            gone = er[s].copy()
            if self.mutant != 19:
                gone[b] = 1
            data_rows = self.data_of(slot, s, gone, r16(S))[1]
            for i in b:
                self.put(slot(s, i), self.shard(data_rows, i), S)
                rewritten[s * self.n + i] = 1
            if self.mutant != 20 and any(self.bad_sectors(slot(s, i), S, sector, crcs, s * self.n + i, crc_pitch)
                                         for i in b):
                status[s] = RS_ETOO_MANY_ERRORS
        return status, bytes(rewritten)


# The naive engine is slow where k * S is large: those scenarios run at a
# reduced S here (one that is as ragged), never 16, 17 or 4112, and in the
# "every" granularity only; on the GPU they run as they are.
REDUCED = {12328: 88, 5000: 200, 4096: 256}


def slow(scenario):
    return scenario[1] * scenario[3] > 100000


def run(scenario, gran, mutant=0):
    ident, k, n, S = scenario[:4]
    if slow(scenario):
        S = REDUCED.get(S, S)
    holder = {}

    def make(k, n, names, arrays):
        holder["e"] = Naive(k, n, sm.Memory(names, arrays, bases=[(b + 5) << 40 for b in range(len(arrays))]), mutant)
        return holder["e"]
    d = io.driver(make, scenario, gran, ("cpu", ident, gran, mutant), S=S)
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


@pytest.mark.parametrize("scenario,gran",
                         [(x, g) for x in IO_SCENARIOS for g in ("every", "async") if g == "every" or not slow(x)],
                         ids=lambda v: v[0] if isinstance(v, tuple) else v)
def test_io_agreement_invariants_and_ledger(scenario, gran):
    """The same for the scenarios of store_model_io.py.  Agreement of the
    checksum verdicts with "differs from what was written" (asserted by the
    driver at every crc_check and crc_repair) also proves that the committed
    seeds meet no CRC collision; the ledger bounds the stripes the repair by
    checksum had to leave out."""
    d = run(scenario, gran)
    assert not d.er.any()
    full = scenario if not slow(scenario) else scenario[:3] + (REDUCED.get(scenario[3], scenario[3]),) + scenario[4:]
    io.check_ledger_io(("cpu", scenario[0], gran, 0), full)


def test_model_crc32c_is_rfc3720():
    """The model's CRC-32C is its own; pinned to the RFC's check value, the
    empty message, and the project's host reference on random lengths."""
    import rsmi
    assert sm.crc32c(b"123456789") == 0xE3069283
    assert sm.crc32c(b"") == 0
    rng = np.random.default_rng(32)
    msgs = [rng.integers(0, 256, size=int(x), dtype=np.uint8).tobytes()
            for x in [0, 1, 70000] + list(rng.integers(0, 70001, size=13))]
    rows = np.zeros((len(msgs), 70000), dtype=np.uint8)
    for r, x in enumerate(msgs):
        rows[r, :len(x)] = np.frombuffer(x, dtype=np.uint8)
    assert sm.crc32c_rows(rows, [len(x) for x in msgs]).tolist() == list(rsmi.crc32c_host(msgs))
    assert Naive.crc(Naive, b"123456789") == 0xE3069283 and Naive.crc(Naive, b"") == 0


def test_io_scenarios_cover_the_shapes():
    shapes = {(x[3], x[7]) for x in IO_SCENARIOS}
    assert {(17, 512), (16, 512), (4112, 4096), (5000, 512), (12328, 4096), (4096, 65536)} <= shapes
    lens = [x[8] for x in IO_SCENARIOS if x[5] == "ptrs_lens" and not x[0].startswith("io-seed")]
    assert any(0 in L[1:-1] and all(L[j - 1] and L[j + 1] for j in range(1, len(L) - 1) if not L[j]) for L in lens)
    assert any(len(set(L)) == 1 for L in lens)
    assert any(L[0] == max(L) > max(L[1:]) for L in lens) and any(L[-1] == max(L) > max(L[:-1]) for L in lens)
    assert all(x[2] - x[1] <= 16 for x in IO_SCENARIOS if x[5] == "ptrs_lens")
    assert len([x for x in IO_SCENARIOS if x[0].startswith("io-seed")]) == 4
    assert not {x[0] for x in IO_SCENARIOS} & {x[0] for x in SCENARIOS}


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
IO_MUTANT_SCENARIOS = sorted([x for x in IO_SCENARIOS if x[1] <= 13 and x[3] <= 5000], key=lambda x: x[1] * x[3] * x[4])


@pytest.mark.parametrize("mutant", sorted(MUTANTS),
                         ids=[f"{q}-{MUTANTS[q].replace(' ', '_')}" for q in sorted(MUTANTS)])
def test_mutant_is_caught(mutant):
    caught = []
    tried = MUTANT_SCENARIOS if mutant <= 13 else IO_MUTANT_SCENARIOS
    for scenario in tried:
        try:
            run(scenario, "async" if mutant == 27 else "every", mutant)
        except sm.Mismatch as x:
            caught.append((scenario[0], str(x)[:200]))
            break
    print(caught)
    assert caught, f"mutant {mutant} ({MUTANTS[mutant]}) survived {len(tried)} scenarios"

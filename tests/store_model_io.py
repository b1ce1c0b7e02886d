"""The store-life scenarios for scattered-shard I/O, a length per stripe and
sector checksums: store_model.Driver with the calls of those three features
in the place of the routes it takes (test_gpu_store_life.py on the GPU,
test_store_model.py on the CPU).  A plain helper module: no fixtures, no GPU
needed to import it.  The scenarios, seeds and draws of store_model.py are not
touched: what is here stands beside them.

Placement "ptrs_io" is the Pool of placement "ptrs" with rs_encode_ptrs,
rs_update_ptrs and rs_read_ptrs for encode, plain update and read (and for the
first pass of a degraded update).  The last two are given a second table,
"table_io", that is built for every call: each entry the header says is never
loaded names a decoy row of the pool, so a wrong load or store shows as wrong
bytes in the whole-image comparison and never as a fault.

Placement "ptrs_lens" is "ptrs_io" with a shard length per stripe, L[s] <= S:
verify, checked repair and column scrub go through the three _lens calls (the
lengths in a ctypes array that is overwritten with 0xFF.. as soon as a call has
returned, before anything synchronises); every call without such a form goes
once per run of consecutive stripes of one non-zero length, over the sub-table
tab + first * n * 8.  Every third _lens call is issued per group of equal
lengths instead, so that the equal-length pass-through and an all-empty call
happen in the middle of a mixed life.

Every scenario here keeps a checksum table the way a store would: after each
op that legitimately changes stored shards the compute call runs with `erased`
set to the real flags plus every present shard that differs from the
remembered truth (the one place where the truth picks arguments; no expected
byte comes from it), so those rows keep what they had.
"""
import ctypes

import numpy as np

import store_model as sm
from oracle import oracle
from store_model import CLEAN, GUARD, RS_ETOO_MANY_ERRORS, RS_OK

NCFB = 48                           # rows of checksum verdicts, used in turn
POISON = ctypes.c_size_t(-1).value


class IoScene(sm.Scene):
    """A Scene with the checksum table (guard words, crc_pitch = nsec + 3,
    every word seeded garbage), rows for the checksum verdicts and, in the
    pointer placements, the per-call table."""

    def __init__(self, k, n, S, stripes, placement, seed, sector):
        super().__init__(k, n, S, stripes, placement, seed)
        rng = np.random.default_rng(seed + 99)
        self.sector, self.nsec = sector, -(-S // sector)
        self.crc_pitch = self.nsec + 3
        if self.ptrs:
            self.TABIO = self.add("table_io", np.zeros(stripes * n * 8, dtype=np.uint8))
        self.CRC = self.add("crc", rng.integers(0, 256, size=2 * GUARD + stripes * n * self.crc_pitch * 4, dtype=np.uint8))
        self.CFB = self.add("crc_first_bad", rng.integers(0, 256, size=2 * GUARD + NCFB * stripes * n * 4, dtype=np.uint8))

    def add(self, name, array):
        self.names.append(name)
        self.init.append(array)
        return len(self.init) - 1

    def where(self, name, off):
        if name == "crc":
            q = (off - GUARD) // 4
            row, j = divmod(q, self.crc_pitch)
            inside = 0 <= q < self.stripes * self.n * self.crc_pitch
            return f"checksum of {divmod(row, self.n)} sector {j} of {self.nsec}" if inside else "guard"
        if name == "crc_first_bad":
            q = (off - GUARD) // 4
            row, x = divmod(q, self.stripes * self.n)
            return f"checksum verdict row {row} shard {divmod(x, self.n)}" if 0 <= row < NCFB else "guard"
        if name == "table_io":
            return f"table_io entry {off // 8}"
        return super().where(name, off)


class IoDriver(sm.Driver):
    """store_model.Driver with the engine calls of the three features in the
    place of its own (the call_* hooks), the checksum table kept after every
    op that changes shards, the op kinds "crc_check" and "crc_repair", and two
    more blocks in the skeleton.  sector: the sector size of the scenario's
    checksums; lens: a shard length per stripe (placement "ptrs_lens")."""

    def __init__(self, make_engine, k, n, S, stripes, placement, seed, gran, sector, lens=None, walk=sm.WALK,
                 ident=None):
        self.sector, self.lens = sector, lens
        super().__init__(make_engine, k, n, S, stripes, placement, seed, gran, walk, ident)
        self.io = placement in ("ptrs_io", "ptrs_lens")
        self.by_lens = placement == "ptrs_lens"
        self.rng2 = np.random.default_rng(seed + 4242)      # decoys
        self.ncfb = self.nlens = 0

    def make_scene(self):
        return IoScene(self.k, self.n, self.S, self.stripes, self.placement, self.seed, self.sector)

    def lengths(self):
        return [self.S] * self.stripes if self.lens is None else [min(int(x), self.S) for x in self.lens]

    # ---- plumbing --------------------------------------------------------------
    def runs(self):
        """(first, count, length) of every run of consecutive stripes of one
        non-zero length."""
        out, s = [], 0
        while s < self.stripes:
            e = s
            while e < self.stripes and self.L[e] == self.L[s]:
                e += 1
            if self.L[s]:
                out.append((s, e - s, self.L[s]))
            s = e
        return out

    def tab(self, e, first=0, io=False):
        return e.adr(self.scene.TABIO if io else self.scene.TAB, first * self.n * 8)

    def sub(self, er, first, count, none=True):
        part = np.ascontiguousarray(er[first:first + count])
        return None if none and not part.any() else part.tobytes()

    def table_io(self, decoy):
        """The per-call table: the entries `decoy` marks name decoy rows of the
        pool (valid, guard-banded addresses), the others their shards' rows."""
        G = self.scene.G
        rows = G.rows.copy()
        rows[decoy] = self.rng2.choice(G.decoys, size=int(decoy.sum()))
        for e in (self.model, self.engine):
            tab = e.bases[0] + GUARD + rows.astype(np.int64) * G.row_bytes
            e.poke(self.scene.TABIO, 0, np.ascontiguousarray(tab.reshape(-1)).view(np.uint8))
        self.ledger["decoys"] += int(decoy.sum())

    def within(self, s, w, er_row, shards_only):
        """Also inside what the checksums repair: |X + B| <= m."""
        return super().within(s, w, er_row, shards_only) and \
            int(er_row.sum()) + int(w.any(axis=1).sum()) <= self.m

    def fit(self, s, chosen, w):
        had = w.any(axis=1)
        room = self.m - self.e(s) - int(had.sum())
        new = [i for i in chosen if not had[i]][:max(0, room)]
        return [i for i in chosen if had[i] or i in new]

    def slice_stripe(self, order):
        """The slice update goes to the longest stripe that can take one."""
        return max(reversed(order), key=lambda s: self.L[s])

    def slice_read(self, reads):
        """The slice read goes to the longest stripe that is read at all."""
        if not self.by_lens:
            return super().slice_read(reads)
        if reads:
            longest = max((s for s, _ in reads), key=lambda s: self.L[s])
            sl = self.slice_of(self.L[longest])
            if sl:
                self.read([x for x in reads if x[0] == longest][:4], *sl)

    def kinds(self):
        return super().kinds() + ("crc_check", "crc_repair")

    def op_other(self, kind):
        if kind == "crc_check":
            self.op_crc_check()
        else:
            self.op_crc_repair()
        return True

    # ---- scattered-shard I/O ---------------------------------------------------------
    def call_encode(self):
        if not self.io:
            return super().call_encode()
        for first, count, L in self.runs():
            self.both("encode_ptrs", lambda e: e.encode_ptrs(self.tab(e, first), L, count))
        self.ledger["encode_ptrs"] += 1

    def call_update(self, listed, ups, offs, o, l, er):
        """rs_update_ptrs for the stripes without flags; one with flags takes
        the header's two passes: "rs_read_ptrs regenerates the old contents
        into scratch ..., then rs_combine applies the deltas to the present
        parity, whose addresses the caller names"."""
        if not self.io:
            return super().call_update(listed, ups, offs, o, l, er)
        R, src = self.scene.ROWS, dict(zip(ups, offs))
        plain = {s: cs for s, cs in listed.items() if er is None or not er[s].any()}
        if plain:
            decoy = np.ones((self.stripes, self.n), dtype=bool)
            for s, cs in plain.items():
                decoy[s, cs] = False
                decoy[s, self.k:] = False
            self.table_io(decoy)
            for first, count, L in self.runs():
                u = [(s, c) for s, c in ups if s in plain and first <= s < first + count]
                if u and L > o:
                    self.both("update_ptrs", lambda e: e.update_ptrs(
                        self.tab(e, first, io=True), min(l, L - o), count,
                        [(s - first, c, e.adr(R, src[(s, c)])) for s, c in u], offset=o))
                    self.ledger["update_ptrs"] += 1
                    self.ledger["update_ptrs_offset"] += o > 0
        for first, count, L in self.runs():
            part = {s: cs for s, cs in listed.items() if s not in plain and first <= s < first + count}
            if part and L > o:
                self.ledger["update_two_pass"] += 1
                self.update_by_combine(part, src, o, min(l, L - o), er)

    def regen_old(self, gone, tmp, o, l, er):
        R = self.scene.ROWS
        first, count, _ = next(r for r in self.runs() if r[0] <= gone[0][0] < r[0] + r[1])
        self.table_io(er != 0)
        self.both("read_ptrs(old contents)", lambda e: e.read_ptrs(
            self.tab(e, first, io=True), l, count, self.sub(er, first, count, none=False),
            [(s - first, c, e.adr(R, tmp[(s, c)])) for s, c in gone], offset=o))
        self.ledger["read_ptrs"] += 1
        self.ledger["read_regenerated"] += len(gone)

    def call_read(self, reads, offs, o, l):
        if not self.io:
            return super().call_read(reads, offs, o, l)
        R = self.scene.ROWS
        self.table_io(self.er != 0)
        for first, count, L in self.runs():
            part = [(s, i, off) for (s, i), off in zip(reads, offs) if first <= s < first + count]
            if part and L > o:
                self.both("read_ptrs", lambda e: e.read_ptrs(
                    self.tab(e, first, io=True), min(l, L - o), count, self.sub(self.er, first, count, none=False),
                    [(s - first, i, e.adr(R, off)) for s, i, off in part], offset=o))
                self.ledger["read_ptrs"] += 1
                self.ledger["read_ptrs_offset"] += o > 0
                self.ledger["read_regenerated"] += sum(int(self.er[s, i]) for s, i, _ in part)

    def rows_again(self, reads, offs):
        for first, count, L in self.runs():
            part = [((s, i), off) for (s, i), off in zip(reads, offs) if first <= s < first + count]
            if part:
                self.by_rows([x for x, _ in part], [off for _, off in part], 0, L, "combine(decode rows)")

    def call_reconstruct(self, fl):
        if not self.by_lens:
            return super().call_reconstruct(fl)
        er = np.frombuffer(fl, dtype=np.uint8).reshape(self.stripes, self.n)
        for first, count, L in self.runs():
            if er[first:first + count].any():
                self.both("reconstruct_ptrs", lambda e: e.reconstruct_ptrs(
                    self.tab(e, first), L, count, self.sub(er, first, count, none=False)))

    # ---- a length per stripe -----------------------------------------------------
    def groups(self):
        """The stripes of a _lens call: all of them, or, every third call, one
        call per group of consecutive equal lengths (empty stripes a group of
        their own)."""
        self.nlens += 1
        if self.nlens % 3:
            return [(0, self.stripes)]
        out, s = [], 0
        while s < self.stripes:
            e = s
            while e < self.stripes and self.L[e] == self.L[s]:
                e += 1
            out.append((s, e - s))
            s = e
        return out

    def lens_call(self, name, first, count, call, sync=False):
        """One _lens call: shard_lens is a ctypes array that is overwritten as
        soon as the call has returned ("is not retained")."""
        L = self.L[first:first + count]
        self.ledger["lens_equal" if len(set(L)) == 1 and L[0] else "lens_mixed" if len(set(L)) > 1 else
                    "lens_empty"] += 1
        self.ledger["lens_zero_" + name] += sum(1 for x in L if not x)

        def fn(e):
            arr = (ctypes.c_size_t * count)(*L)
            try:
                return call(e, arr)
            finally:
                for j in range(count):
                    arr[j] = POISON
        return self.both(name, fn, sync=sync)

    def call_verify(self, er, off):
        if not self.by_lens:
            return super().call_verify(er, off)
        for first, count in self.groups():
            self.lens_call("verify_ptrs_lens", first, count, lambda e, arr: e.verify_ptrs_lens(
                self.tab(e, first), arr, count, e.adr(self.scene.FB, off + 4 * first),
                erased=self.sub(er, first, count)))

    def call_checked(self, fl, off):
        if not self.by_lens:
            return super().call_checked(fl, off)
        er = np.frombuffer(fl, dtype=np.uint8).reshape(self.stripes, self.n)
        for first, count in self.groups():
            self.lens_call("reconstruct_checked_ptrs_lens", first, count,
                           lambda e, arr: e.reconstruct_checked_ptrs_lens(
                               self.tab(e, first), arr, count, self.sub(er, first, count, none=False),
                               e.adr(self.scene.FB, off + 4 * first)))

    def verdicts(self, off):
        """A call whose lengths are all 0 writes nothing: those stripes are clean."""
        fb = super().verdicts(off)
        fb[np.array([s for s in range(self.stripes) if not self.L[s]], dtype=int)] = CLEAN
        return fb

    def call_columns(self, fl):
        if not self.by_lens:
            return super().call_columns(fl)
        er = np.zeros((self.stripes, self.n), dtype=np.uint8) if fl is None else \
            np.frombuffer(fl, dtype=np.uint8).reshape(self.stripes, self.n)
        status, corrected = [], []
        for first, count in self.groups():
            res = self.lens_call("correct_columns_ptrs_lens", first, count,
                                 lambda e, arr: e.correct_columns_ptrs_lens(
                                     self.tab(e, first), arr, count, erased=self.sub(er, first, count)), sync=True)
            if res[0] != "ok":
                return res
            status += res[1][0]
            corrected += res[1][1]
        return ["ok", [status, corrected]]

    # ---- the ops that change stored shards: the checksums follow ---------------------
    def op_encode(self):
        super().op_encode()
        self.crc_update()

    def op_update(self, listed, sl=None, er=None):
        combines = sum(v for name, v in self.ledger.items() if name.startswith("call combine("))
        done = super().op_update(listed, sl, er)
        if er is None and self.io:
            self.ledger["plain_by_combine"] += sum(
                v for name, v in self.ledger.items() if name.startswith("call combine(")) - combines
        self.crc_update()
        return done

    def op_checked(self):
        fb = super().op_checked()
        self.crc_update()
        return fb

    def op_reconstruct(self):
        done = super().op_reconstruct()
        if done:
            self.crc_update()
        return done

    def op_columns(self, unrepairable=True):
        res = super().op_columns(unrepairable)
        self.crc_update()
        return res

    def op_shards(self):
        """Where the pointer placement has no codeword scrub left (m > 16),
        the checksums repair."""
        if self.ptrs and self.m > 16:
            return self.op_crc_repair()
        res = super().op_shards()
        if res is not None and not self.ptrs:
            self.crc_update()
        return res

    # ---- sector checksums --------------------------------------------------------
    def crc_calls(self, name, er, first_bad=None):
        """One checksum call on the strided placements, one per run of lengths
        on the pointer placements: "crcs[(s * n + i) * crc_pitch + j]", the
        sub-table's rows starting at stripe `first`."""
        sc, n = self.scene, self.n
        if not self.ptrs:
            def call(e):
                extra = () if first_bad is None else (e.adr(sc.CFB, first_bad),)
                return getattr(e, name + "_stripes")(*self.sargs(e), sc.sector, e.adr(sc.CRC, GUARD), sc.crc_pitch,
                                                     *extra, erased=self.sub(er, 0, self.stripes))
            self.both(name + "_stripes", call)
            return
        for first, count, L in self.runs():
            def call(e):
                extra = () if first_bad is None else (e.adr(sc.CFB, first_bad + first * n * 4),)
                return getattr(e, name + "_ptrs")(self.tab(e, first), L, count, sc.sector,
                                                  e.adr(sc.CRC, GUARD + first * n * sc.crc_pitch * 4), sc.crc_pitch,
                                                  *extra, erased=self.sub(er, first, count))
            self.both(name + "_ptrs", call)

    def differs(self):
        return np.stack([self.wrong(s).any(axis=1) for s in range(self.stripes)])

    def crc_update(self):
        self.crc_calls("crc32c", self.er | self.differs().astype(np.uint8))
        self.ledger["crc_update"] += 1

    def crc_check(self, er=None):
        """The check call with the real flags; the verdicts [stripes][n] (of
        the model: the checkpoint compares the engine's with them)."""
        off = GUARD + (self.ncfb % NCFB) * self.stripes * self.n * 4
        self.ncfb += 1
        self.crc_calls("crc32c_check", self.er if er is None else er, first_bad=off)
        v = self.model.mem.bufs[self.scene.CFB][off:off + 4 * self.stripes * self.n].view(np.uint32).copy()
        v = v.reshape(self.stripes, self.n)
        v[np.array([s for s in range(self.stripes) if not self.L[s]], dtype=int)] = CLEAN
        return v

    def op_crc_check(self):
        """The end-to-end sentence: a present shard's verdict is clean if and
        only if its [0, L) is what was written."""
        v, d = self.crc_check(), self.differs()
        for s in range(self.stripes):
            for i in range(self.n):
                want = bool(d[s, i]) and not self.er[s, i]
                assert (v[s, i] != CLEAN) == want, (self.what(), s, i, int(v[s, i]), want)
        self.ledger["crc_check"] += 1
        self.ledger["crc_flagged"] += int((v != CLEAN).sum())
        return v

    def op_crc_repair(self, expect_left=()):
        """Repair by checksum.  Strided: rs_correct_crc32c.  Pointer
        placements, the header's recipe: check, first_bad "Copied to the host
        and reduced to non-zero / zero (clean), it is an `erased` array", the
        checked repair with X + B, check again; a stripe with |X + B| > m is
        left out.  Afterwards every stripe that was not left out is the truth."""
        d = self.differs()
        B = [[i for i in range(self.n) if d[s, i] and not self.er[s, i]] for s in range(self.stripes)]
        left = [s for s in range(self.stripes) if B[s] and self.e(s) + len(B[s]) > self.m]
        assert set(left) == set(expect_left), (self.what(), left, expect_left)
        if not self.ptrs:
            sc = self.scene
            res = self.both("correct_crc32c", lambda e: e.correct_crc32c(
                *self.sargs(e), sc.sector, e.adr(sc.CRC, GUARD), sc.crc_pitch,
                erased=self.sub(self.er, 0, self.stripes)), sync=True)
            assert res[0] == "ok", (self.what(), res)
            status, rewritten = res[1]
            for s in range(self.stripes):
                assert [i for i in range(self.n) if rewritten[s * self.n + i]] == ([] if s in left else B[s]), \
                    (self.what(), s, rewritten)
                if s in left:
                    assert status[s] == RS_ETOO_MANY_ERRORS, (self.what(), s, status)
                elif not B[s]:
                    assert status[s] == RS_OK, (self.what(), s, status)
        else:
            v = self.crc_check()
            self.checkpoint()       # a store reads the verdicts back here
            flags = self.er | (v != CLEAN).astype(np.uint8)
            assert all([i for i in range(self.n) if v[s, i] != CLEAN] == B[s] for s in range(self.stripes)), \
                (self.what(), v.tolist(), B)
            flags[np.array(left, dtype=int)] = 0
            if flags.any():
                self.call_checked(flags.tobytes(), self.fbrow())
                self.settle()
        for s in range(self.stripes):
            if s not in left:
                assert not self.wrong(s).any(), (self.what(), s)
        self.crc_update()
        if self.ptrs:
            v = self.crc_check()
            assert all((v[s] == CLEAN).all() for s in range(self.stripes) if s not in left), (self.what(), v.tolist())
        self.ledger["crc_repair"] += 1
        if not expect_left:
            self.ledger["crc_seen"] += sum(1 for s in range(self.stripes) if B[s])
            self.ledger["crc_left_out"] += len(left)
        self.ledger["crc_beyond"] += sum(1 for s in range(self.stripes) if s not in left and len(B[s]) > self.m // 2)
        return True

    # ---- the skeleton's two blocks -------------------------------------------------
    def beyond_the_radius(self):
        """floor(m / 2) + 1 whole shards of the first stripe that has bytes are
        wrong: one more than any codeword scrub promises to repair.  The
        verify sees an inconsistent stripe, the column scrub (where the code
        has one, m <= 16) gives it up, the checksums flag exactly those shards,
        and the repair by checksum restores them."""
        if self.m < 3:
            return
        s = next(s for s in range(self.stripes) if self.L[s])
        assert not self.er.any()
        had = self.wrong(s).any(axis=1)
        new = [int(i) for i in self.rng.permutation(self.n) if not had[i]][:self.m // 2 + 1 - int(had.sum())]
        for i in [int(i) for i in np.flatnonzero(had)] + new:     # every byte of these shards is wrong
            b, off = self.scene.at(s, i)
            mask = self.rng.integers(1, 256, size=self.L[s], dtype=np.uint8)
            self.host("xor", b, off, np.where(self.wrong(s)[i, :self.L[s]], 0, mask).astype(np.uint8))
        w = self.wrong(s)[:, :self.L[s]]
        assert int(w.all(axis=1).sum()) == int(w.any(axis=1).sum()) == self.m // 2 + 1
        assert self.op_verify()[s] != CLEAN, self.what()
        if self.m <= 16:
            # The column scrub must give the stripe up: RS_ETOO_MANY_ERRORS, "a
            # column beyond the radius ... is left alone".  With an odd m no
            # codeword lies within floor(m / 2) of any column (two codewords
            # differ in m + 1 places), so nothing is written.  With an even m
            # a column may land on another codeword, whose bytes the scrub
            # then writes: the model says which (the oracle, column by
            # column), counts and bytes are compared like any other, and those
            # columns are put back by host writes, because their damage is
            # wider than what the checksums repair.
            before = [self.stored(s, i).copy() for i in range(self.n)]
            self.model.beyond = True
            try:
                res = self.call_columns(None)
            finally:
                self.model.beyond = False
            assert res[0] == "ok" and res[1][0][s] == RS_ETOO_MANY_ERRORS, (self.what(), res)
            landed = [i for i in range(self.n) if not np.array_equal(before[i], self.stored(s, i))]
            assert bool(landed) == any(res[1][1][s * self.n:(s + 1) * self.n]) and not (landed and self.m % 2), \
                (self.what(), landed, res)
            for i in landed:
                b, off = self.scene.at(s, i)
                self.host("poke", b, off, before[i][:self.L[s]])
            self.crc_update()       # another stripe's damage of step 13 may have been repaired
            self.ledger["scrub_gave_up"] += 1
            self.ledger["landed_elsewhere"] += len(landed)
        v = self.op_crc_check()
        assert int((v[s] != CLEAN).sum()) == self.m // 2 + 1, (self.what(), v[s].tolist())
        self.op_crc_repair()
        assert self.clean(s), self.what()
        self.ledger["beyond_radius"] += 1

    def other_data(self):
        """A stripe is overwritten with a valid codeword of other data (a stale
        shard set, a lost update): the codeword check says clean, the
        checksums flag all n shards, and the repair by checksum answers
        RS_ETOO_MANY_ERRORS with nothing written.  Then, on the strided
        placements, one stored checksum is wrong: the shard is regenerated to
        the bytes it had, and the second check still fails."""
        if self.m < 1:
            return
        assert not self.er.any() and all(self.clean(s) for s in range(self.stripes))
        s = max(range(self.stripes), key=lambda s: (self.L[s], s))
        L, E = self.L[s], self.model.E
        saved = [self.stored(s, i)[:L].copy() for i in range(self.n)]
        while True:
            data = self.rng.integers(0, 256, size=(self.k, L), dtype=np.uint8)
            word = list(data) + oracle.matmul_stripe(np.ascontiguousarray(E[self.k:]), [r.copy() for r in data])
            if all((w != t).any() for w, t in zip(word, saved)):
                break
        for i, w in enumerate(word):
            b, off = self.scene.at(s, i)
            self.host("poke", b, off, np.ascontiguousarray(w))
        assert (self.op_verify() == CLEAN).all(), self.what()
        v = self.op_crc_check()
        assert (v[s] != CLEAN).all(), (self.what(), v[s].tolist())
        self.op_crc_repair(expect_left=(s,))
        for i, w in enumerate(saved):
            b, off = self.scene.at(s, i)
            self.host("poke", b, off, w)
        self.ledger["other_data"] += 1
        if self.ptrs:
            return
        sc, i = self.scene, int(self.rng.integers(self.n))
        entry = (sc.CRC, GUARD + (s * self.n + i) * sc.crc_pitch * 4, np.array([1], dtype=np.uint8))
        self.host("xor", *entry)
        res = self.both("correct_crc32c", lambda e: e.correct_crc32c(
            *self.sargs(e), sc.sector, e.adr(sc.CRC, GUARD), sc.crc_pitch), sync=True)
        want = bytearray(self.stripes * self.n)
        want[s * self.n + i] = 1
        assert res == ["ok", [[RS_ETOO_MANY_ERRORS if x == s else RS_OK for x in range(self.stripes)], list(want)]], \
            (self.what(), res)
        self.host("xor", *entry)
        self.ledger["crc_second_check"] += 1


# =============================================================================
# The scenarios
# =============================================================================
# (k, n, S, stripes, placement, sector, lens).  Codes that select every twin:
# (10,14) and (4,6) the K-specialised kernels; (64,80) the bit-sliced pointer
# encode and the K64 read; (12,40) runtime k with row groups of 16 and the
# update's copy commit (m > 16: no column scrub, the checksums repair); (5,9)
# runtime k below one load batch; (1,3), (4,5), (3,3) k = 1, m = 1, m = 0.
# The sector shapes: one partial sector (S = 17 and 16 with 512), a second
# sector of 16 bytes (4112 with 4096), ten sectors and a ragged tail (5000 with
# 512), 12328 with 4096, 4096 with 65536.  The lengths: an empty stripe between
# two that have bytes, all equal (the pass-through), the longest first, the
# longest last.
FIXED_IO = [
    (10, 14, 17, 4, "ptrs_io", 512, None),
    (10, 14, 4112, 3, "split", 4096, None),
    (10, 14, 4112, 4, "ptrs_lens", 4096, (4112, 0, 17, 17)),
    (4, 6, 16, 3, "ptrs_io", 512, None),
    (4, 6, 5000, 2, "joined", 512, None),
    (4, 6, 5000, 5, "ptrs_lens", 512, (1, 16, 16, 0, 5000)),
    (64, 80, 17, 2, "ptrs_io", 512, None),
    (64, 80, 4096, 3, "ptrs_lens", 512, (17, 0, 4096)),
    (12, 40, 4112, 2, "ptrs_io", 4096, None),
    (5, 9, 12328, 2, "ptrs_io", 4096, None),
    (5, 9, 4096, 3, "ptrs_lens", 65536, (4096, 4096, 4096)),
    (13, 18, 5000, 3, "split", 512, None),
    (1, 3, 5000, 4, "ptrs_io", 512, None),
    (4, 5, 17, 4, "ptrs_lens", 512, (17, 16, 0, 16)),
    (3, 3, 4112, 3, "ptrs_io", 4096, None),
]
LENGTHS = (0, 1, 16, 17, 4096, 4112, 5000)


def scenarios_io():
    """[(id, k, n, S, stripes, placement, seed, sector, lens)]: the fixed ones
    and four seeded ones (seeds 21..24)."""
    out = []
    for j, (k, n, S, stripes, placement, sector, lens) in enumerate(FIXED_IO):
        out.append((f"io-rs{k}_{n}-S{S}x{stripes}-{placement}-sec{sector}", k, n, S, stripes, placement,
                    5000 + 100 * k + n + j, sector, lens))
    for seed in range(21, 25):
        rng = np.random.default_rng(8000 + seed)
        k = int(rng.integers(1, 33))
        n = k + int(rng.integers(1, 13))
        S = sm.SIZES[int(rng.integers(len(sm.SIZES)))]
        stripes = int(rng.integers(3, 6))
        placement = ("ptrs_io", "ptrs_lens", "joined", "ptrs_lens")[seed - 21]
        sector = (512, 4096, 65536)[int(rng.integers(3))]
        lens = None
        if placement == "ptrs_lens":
            lens = [int(x) for x in rng.choice([x for x in LENGTHS if x <= S] + [S], size=stripes)]
            lens[int(rng.integers(stripes))] = S
        if k * S > 65536:       # a large code keeps the case quick with one column, or a ragged second one
            small = 17 if S % 16 else 16
            lens = None if lens is None else [small if x == S else min(x, small) for x in lens]
            S = small
        out.append((f"io-seed{seed}-rs{k}_{n}-S{S}x{stripes}-{placement}-sec{sector}", k, n, S, stripes, placement,
                    seed, sector, lens))
    return out


def driver(make_engine, scenario, gran, ident, S=None):
    """The driver of a scenario of store_model.scenarios() or scenarios_io();
    S: a reduced shard length (the CPU proof of the large ones)."""
    _, k, n, S0, stripes, placement, seed = scenario[:7]
    S = S0 if S is None else S
    if len(scenario) == 7:
        return sm.Driver(make_engine, k, n, S, stripes, placement, seed, gran, ident=ident)
    return IoDriver(make_engine, k, n, S, stripes, placement, seed, gran, scenario[7], scenario[8], ident=ident)


def check_ledger_io(ident, scenario):
    """store_model.check_ledger for a scenario of scenarios_io(), and what the
    new walk exists for."""
    _, k, n, S, stripes, placement, _, sector, lens = scenario
    led, m, ptrs = sm.LEDGER[ident], n - k, placement in sm.PTRS
    sm.check_ledger(ident, k, n, stripes, ptrs)
    what = (ident, dict(led))
    assert led["crc_check"] > 0 and led["crc_repair"] > 0 and led["crc_update"] > 0, what
    if placement in ("ptrs_io", "ptrs_lens"):
        assert led["call combine(encode)"] == led["call combine(read)"] == led["plain_by_combine"] == 0, what
        assert led["encode_ptrs"] > 0 or m == 0, what
        assert led["update_ptrs"] > 0 and led["read_ptrs"] > 0 and led["decoys"] > 0, what
        if m:
            assert led["read_regenerated"] > 0, what
        if max(lens or [S]) > 16:
            assert led["update_ptrs_offset"] > 0 and led["read_ptrs_offset"] > 0, what
    if placement == "ptrs_lens":
        names = ["verify_ptrs_lens", "reconstruct_checked_ptrs_lens", "correct_columns_ptrs_lens"]
        assert led["lens_equal"] > 0, what
        if len(set(lens)) > 1:
            assert led["lens_mixed"] > 0, what
        if 0 in lens:
            assert all(led["lens_zero_" + x] > 0 for x in names), what
    if m >= 3:
        assert led["beyond_radius"] > 0 and led["crc_beyond"] > 0, what
        assert led["scrub_gave_up"] > 0 or m > 16, what
    if m >= 1:
        assert led["other_data"] > 0, what
        assert led["crc_second_check"] > 0 or ptrs, what
    assert 2 * led["crc_left_out"] <= led["crc_seen"], what

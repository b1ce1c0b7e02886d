"""Whole-image model of rs_correct_columns_ptrs_lens -- the column scrub of the
pointer placement for stripes that each have a shard length of their own
(test_gpu_column_lens.py; proved on the CPU by test_lens_columns_model.py).
A plain helper module: no fixtures, and no GPU needed to import it.

A ColumnRun is the host model of one call on a lens_pool.LensPool: `cur` is
the image before the call, `want` the image that must result, `status` and
`counts` what the call must report per stripe and per shard.  Table entries of
erased shards name decoy rows -- valid memory that no test looks for a
codeword in -- and the erased shards' own rows hold random bytes that no entry
names: nothing a call can do reaches an invalid address.

Expected bytes never come from the engine.  The model knows every byte it
damaged.  A damaged column below its stripe's length with errors within the
radius floor((r - k) / 2) must return to the pool's pristine bytes, whose
parity is the oracle's.  One with more errors takes the oracle's per-column
decode_correct: on an error code the column stays and the stripe fails,
otherwise the column becomes the codeword the oracle found.  Damage at or
beyond a stripe's length is no part of a codeword: it stays and is not counted.
A stripe with r - k < 2 that is inconsistent fails and stays as it is.
"""
import numpy as np

from lens_pool import CLEAN, matrix
from oracle import oracle
from strided_image import GUARD

OK, TOO_MANY = 0, -16  # RS_OK, RS_ETOO_MANY_ERRORS (include/rsmi.h)
STATUS_SENTINEL = 0x5B5B5B5B
COUNT_SENTINEL = 0xA5A5A5A5


def oracle_column(k, n, shares):
    """The oracle's Correct on one byte column: shares = [(number, byte)].
    (status, the n bytes of the codeword it found, or None)."""
    E = matrix(k, n)
    rc, data = oracle.decode_correct(E, k, n, [(i, bytes([b])) for i, b in shares])
    if rc != 0:
        return rc, None
    return rc, list(data) + list(oracle.encode(E, k, n, data))


def special_offsets(S):
    """The first and the last byte and both sides of every 4096 boundary."""
    offs = [0, S - 1]
    for b in range(4096, S, 4096):
        offs += [b - 1, b]
    return list(dict.fromkeys(o for o in offs if 0 <= o < S))


class ColumnRun:
    def __init__(self, P, er=None, seed=0):
        self.P = P
        self.er = np.zeros((P.stripes, P.n), dtype=np.uint8) if er is None else \
            np.asarray(er, dtype=np.uint8).reshape(P.stripes, P.n).copy()
        self.base = P.pristine.copy()   # the pool with the lost shards' rows overwritten: no damage yet
        self.entry_row = P.rows.copy()  # the row each table entry names
        rng = np.random.default_rng(8100 + seed)
        for s, i in zip(*np.nonzero(self.er)):
            o = P.row_at(P.rows[s, i])
            self.base[o:o + P.row_bytes] = rng.integers(0, 256, size=P.row_bytes, dtype=np.uint8)  # the lost shard
            self.entry_row[s, i] = P.decoys[int(rng.integers(len(P.decoys)))]  # entries may repeat: never loaded
        self.cur = self.base.copy()
        self.touched = {}               # stripe -> offsets (of the row) that hold damage
        self.want = self.status = self.counts = None
        self.dev = self.table = self.host_table = None

    # ---- the image before the call
    def at(self, s, i):
        return self.P.row_at(self.P.rows[s, i])

    def present(self, s):
        return [i for i in range(self.P.n) if not self.er[s, i]]

    def radius(self, s):
        return max(len(self.present(s)) - self.P.k, 0) // 2

    def flags(self):
        return self.er.tobytes() if self.er.any() else None

    def flip(self, s, i, off, mask=0x20):
        """XORs mask into byte off of the ROW of present shard i of stripe s;
        off may lie at or beyond the stripe's length."""
        assert mask and not self.er[s, i] and 0 <= off < self.P.row_bytes
        self.cur[self.at(s, i) + off] ^= mask
        self.touched.setdefault(int(s), set()).add(int(off))

    def scatter(self, s, rng, extra=5, weight=None):
        """Damage of stripe s within its radius: at the special offsets and a
        few random ones, 1 .. radius flips (the first column exactly at the
        radius; weight: every column) in distinct present shards, the shards
        rotating from column to column."""
        S, present, radius = self.P.lens[s], self.present(s), self.radius(s)
        if S == 0 or radius == 0:
            return
        special = special_offsets(S)
        rest = [int(o) for o in rng.permutation(S)[:extra + len(special)] if int(o) not in special][:extra]
        at = int(rng.integers(len(present)))
        for c, off in enumerate(special + rest):
            w = weight or (radius if c == 0 else int(rng.integers(1, radius + 1)))
            for j in range(w):
                self.flip(s, present[(at + j) % len(present)], off, int(rng.integers(1, 256)))
            at += w

    def column(self, s, off):
        return [(i, int(self.cur[self.at(s, i) + off])) for i in self.present(s)]

    def expect(self):
        """want, status and counts from the damage, the pristine pool and the oracle."""
        P = self.P
        self.want = self.cur.copy()
        self.status = [OK] * P.stripes
        self.counts = np.zeros((P.stripes, P.n), dtype=np.int64)
        for s, offs in sorted(self.touched.items()):
            S, present = P.lens[s], self.present(s)
            if len(present) == P.k:
                continue  # nothing to compare (m erasures, or no parity): any bytes are a codeword
            wrong = {}  # offset below S -> the present shards whose byte is not the pristine one
            for off in sorted(o for o in offs if o < S):
                bad = [i for i in present if self.cur[self.at(s, i) + off] != P.pristine[self.at(s, i) + off]]
                # up to r - k wrong bytes are never another codeword: the stripe is inconsistent
                assert len(bad) <= len(present) - P.k, "the model places at most r - k errors in a column"
                if bad:
                    wrong[off] = bad
            if not wrong:
                continue  # clean below its length: not a job, unwritten
            if len(present) - P.k < 2:
                self.status[s] = TOO_MANY  # seen, not locatable: unwritten
                continue
            for off, bad in wrong.items():
                if len(bad) <= self.radius(s):
                    word = [int(P.pristine[self.at(s, i) + off]) for i in range(P.n)]
                else:
                    rc, word = oracle_column(P.k, P.n, self.column(s, off))
                    if rc != 0:
                        self.status[s] = TOO_MANY
                        continue
                for i in present:
                    o = self.at(s, i) + off
                    self.counts[s, i] += int(self.want[o] != word[i])
                    self.want[o] = word[i]
        return self

    def jobs(self):
        """The stripes the column launch must cover (after expect)."""
        return [s for s in range(self.P.stripes)
                if self.counts[s].sum() > 0 or (self.status[s] == TOO_MANY and len(self.present(s)) - self.P.k >= 2)]

    # ---- the device
    def upload(self, torch):
        self.dev = torch.from_numpy(self.cur).cuda()
        self.host_table = (self.dev.data_ptr() + GUARD + self.entry_row.astype(np.int64) * self.P.row_bytes).reshape(-1)
        assert (self.host_table % 16 == 0).all()
        self.table = torch.from_numpy(self.host_table.copy()).cuda()
        return self.table.data_ptr()

    def call(self, f, torch=None):
        """The _lens call over the image as it is now (uploads it when torch is
        given); returns (status, counts[stripes][n])."""
        if torch is not None:
            self.upload(torch)
        P = self.P
        st, cnt = f.correct_columns_ptrs_lens(self.table.data_ptr(), P.lens, P.stripes, erased=self.flags())
        return st, np.asarray(cnt, dtype=np.int64).reshape(P.stripes, P.n)

    def call_by_length(self, f, torch):
        """The only route without the call: for each distinct non-zero length,
        correct_columns_ptrs on a sub-table of the stripes of that length."""
        self.upload(torch)
        P = self.P
        st, cnt = [OK] * P.stripes, np.zeros((P.stripes, P.n), dtype=np.int64)
        for S in sorted(set(P.lens) - {0}):
            idx = [s for s in range(P.stripes) if P.lens[s] == S]
            sub = torch.from_numpy(self.host_table.reshape(P.stripes, P.n)[idx].reshape(-1).copy()).cuda()
            er = self.er[idx]
            st_s, cnt_s = f.correct_columns_ptrs(sub.data_ptr(), S, len(idx), erased=er.tobytes() if er.any() else None)
            for j, s in enumerate(idx):
                st[s] = st_s[j]
            cnt[idx] = np.asarray(cnt_s, dtype=np.int64).reshape(len(idx), P.n)
        return st, cnt

    def verify(self, f, torch):
        """first_bad of verify_ptrs_lens over the device image as it is now."""
        fb = torch.full((self.P.stripes,), 0x7A7A7A7A, dtype=torch.int32, device="cuda:0")
        f.verify_ptrs_lens(self.table.data_ptr(), self.P.lens, self.P.stripes, fb.data_ptr(), erased=self.flags())
        f.sync()
        return fb.cpu().numpy().view(np.uint32)

    def image(self):
        return self.dev.cpu().numpy()

    def check(self, what="", want=None):
        want = self.want if want is None else want
        bad = np.flatnonzero(self.image() != want)
        assert bad.size == 0, f"{what} pool: {bad.size} bytes differ, first offsets {bad[:8].tolist()}"
        assert np.array_equal(self.table.cpu().numpy(), self.host_table), f"{what}: the table changed"

    def run(self, f, torch, what=""):
        """expect, call, compare everything; returns (status, counts)."""
        self.expect()
        st, cnt = self.call(f, torch)
        assert st == self.status, (what, self.P.lens, st, self.status)
        self.check(what)
        assert np.array_equal(cnt, self.counts), (what, self.P.lens, np.argwhere(cnt != self.counts)[:8].tolist())
        return st, cnt


__all__ = ["CLEAN", "OK", "TOO_MANY", "ColumnRun", "oracle_column", "special_offsets"]

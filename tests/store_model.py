"""A byte-exact host model of the device-resident API, and the driver that
runs an engine and the model through the same seeded life of a store
(test_gpu_store_life.py on the GPU; test_store_model.py proves the driver on
the CPU with a second, naive host engine).  A plain helper module: no
fixtures, no GPU needed to import it.

Memory holds the bytes of every device buffer of a scenario at addresses, so
the Model's methods take exactly what the rsmi.FEC binding takes: the fake
addresses of a Memory here, device pointers on the GPU.  Every call is applied
to the bytes that are stored, as include/rsmi.h words it; the sentence that is
implemented stands next to the code.  The Driver keeps a remembered truth (the
codeword every stripe is meant to hold) to choose the next op and for the
final checks only; no expected byte comes from it.

Padding follows strided_image.Image: bytes [S, round_up(S, 16)) of a shard or
row a call writes are `loose` -- not compared, and adopted from the engine at
the next comparison so that every later "untouched" check stays strict.
Everything else is compared exactly at every checkpoint: guards, pitch
padding, stride gaps, decoy rows, erased slots after a garbage fill, the
first_bad rows, and in pointer mode the address table.

The Model also has the scattered-shard I/O calls, the calls with a length per
stripe and the sector checksums; the scenarios that use them, and the driver
that overrides this one's call_* hooks for them, are in store_model_io.py.
"""
import collections
import ctypes

import numpy as np

import np_rs
from oracle import oracle
from strided_image import GUARD, Layout, Pool, fixed_patterns, r16

CLEAN = 0xFFFFFFFF
RS_OK, RS_ENOT_ENOUGH, RS_EINVAL, RS_ETOO_MANY_ERRORS = 0, -3, -8, -16


class Refused(Exception):
    """A call the header refuses with nothing launched or written."""

    def __init__(self, code):
        super().__init__(code)
        self.code = code


class Memory:
    """Device buffers as host bytes: buffer b lies at [bases[b], bases[b] + len)."""

    def __init__(self, names, arrays, bases=None):
        self.names = list(names)
        self.bufs = [np.array(a, dtype=np.uint8) for a in arrays]
        self.bases = list(bases) if bases is not None else [(b + 1) << 32 for b in range(len(self.bufs))]
        self.loose = [np.zeros(len(a), dtype=bool) for a in self.bufs]

    def find(self, addr, length):
        for b, (base, a) in enumerate(zip(self.bases, self.bufs)):
            if base <= addr and addr + length <= base + len(a):
                return b, addr - base
        raise AssertionError(f"address {addr:#x}+{length} is in no buffer")

    def view(self, addr, length):
        b, o = self.find(addr, length)
        return self.bufs[b][o:o + length]

    def wrote(self, addr, S):
        """A call wrote round_up(S, 16) bytes at addr: its pad is loose."""
        b, o = self.find(addr, r16(S))
        self.loose[b][o + S:o + r16(S)] = True


def survivors(er_row, k, n):
    """rsmi.h, rs_pattern_survivors: "slot i holds shard i if it is present,
    otherwise the highest-numbered remaining parity (Rebuild's choice)".
    None for more than m erasures."""
    ids, p = [], n - 1
    for i in range(k):
        if not er_row[i]:
            ids.append(i)
            continue
        while p >= k and er_row[p]:
            p -= 1
        if p < k:
            return None
        ids.append(p)
        p -= 1
    return ids if int(np.sum(np.asarray(er_row) != 0)) <= n - k else None


def _crc_table():
    t = np.arange(256, dtype=np.uint32)
    for _ in range(8):
        t = np.where(t & 1, (t >> 1) ^ np.uint32(0x82F63B78), t >> 1).astype(np.uint32)
    return t


_CRC_TABLE = _crc_table()
_CRC_MEMO = {}


def crc32c_rows(rows, lens=None):
    """CRC-32C as RFC 3720 defines it (reflected polynomial 0x82F63B78, initial
    value 0xFFFFFFFF, final XOR 0xFFFFFFFF), byte by byte through the table,
    of the first lens[r] bytes of every row of `rows` [N][W] at once."""
    rows = np.asarray(rows, dtype=np.uint8)
    lens = np.full(len(rows), rows.shape[1]) if lens is None else np.asarray(lens)
    c = np.full(len(rows), 0xFFFFFFFF, dtype=np.uint32)
    for j in range(int(lens.max(initial=0))):
        nxt = _CRC_TABLE[(c ^ rows[:, j]) & 0xFF] ^ (c >> 8)
        c = np.where(j < lens, nxt, c)
    return c ^ np.uint32(0xFFFFFFFF)


def crc32c(message):
    return int(crc32c_rows(np.frombuffer(bytes(message), dtype=np.uint8)[None, :])[0])


def crc32c_sectors(shards, sector):
    """The checksums of the ceil(S / sector) sectors of every shard of a list
    of equally long shards, the last sector over what is left: [uint32[nsec]].
    All sectors go through the table side by side; a shard's result is
    remembered by its content (most shards do not change between two calls)."""
    keys = [(bytes(x), sector) for x in shards]
    out = {key: _CRC_MEMO[key] for key in keys if key in _CRC_MEMO}
    todo = list(dict.fromkeys(key for key in keys if key not in out))
    if todo:
        if len(_CRC_MEMO) > 2048:
            _CRC_MEMO.clear()
        S = len(todo[0][0])
        nsec, W = -(-S // sector), min(sector, S)
        rows = np.zeros((len(todo) * nsec, W), dtype=np.uint8)
        for r, (content, _) in enumerate(todo):
            for j in range(nsec):
                part = np.frombuffer(content, dtype=np.uint8)[j * sector:(j + 1) * sector]
                rows[r * nsec + j, :len(part)] = part
        sums = crc32c_rows(rows, [min(sector, S - j * sector) for j in range(nsec)] * len(todo))
        for r, key in enumerate(todo):
            _CRC_MEMO[key] = out[key] = sums[r * nsec:(r + 1) * nsec]
    return [out[key] for key in keys]


class HostEngine:
    """What the Model and the naive engine of test_store_model.py share: the
    Memory and the host-side writes of the driver.  No addressing, no flag
    parsing, no call semantics."""

    def __init__(self, k, n, mem):
        self.k, self.n, self.m, self.mem = k, n, n - k, mem
        self.bases = mem.bases

    def adr(self, buf, off):
        return self.bases[buf] + off

    def poke(self, buf, off, data):
        self.mem.bufs[buf][off:off + len(data)] = data
        self.mem.loose[buf][off:off + len(data)] = False

    def xor(self, buf, off, data):
        self.mem.bufs[buf][off:off + len(data)] ^= data

    def sync(self):
        pass

    def snapshot(self):
        return self.mem.bufs


class Model(HostEngine):
    """The byte-exact model.  One method per call, with the binding's arguments."""

    def __init__(self, k, n, mem):
        super().__init__(k, n, mem)
        self.E = oracle.fec_matrix(k, n)
        self._D = {}
        self.beyond = False     # columns beyond the decoding radius are expected (_codeword)

    # ---- addressing ----------------------------------------------------------
    def strided(self, data, dss, parity, pss, pitch):
        """rsmi.h: "Stripe s, shard i lives at data + s * data_stripe_stride +
        i * shard_pitch (i < k), parity + s * parity_stripe_stride + (i - k) *
        shard_pitch (i >= k)"."""
        k = self.k
        return lambda s, i: data + s * dss + i * pitch if i < k else parity + s * pss + (i - k) * pitch

    def table(self, tab, stripes):
        """rsmi.h: "shard i of stripe s is read (survivor) or written (erased)
        at shard_ptrs[s * n + i]"."""
        t = self.mem.view(tab, stripes * self.n * 8).view(np.int64)
        n = self.n
        return lambda s, i: int(t[s * n + i])

    def flags(self, erased, stripes):
        if erased is None:
            return np.zeros((stripes, self.n), dtype=np.uint8)
        return np.frombuffer(bytes(erased), dtype=np.uint8).reshape(stripes, self.n)

    # ---- decode rows ---------------------------------------------------------
    def decode_matrix(self, er_row):
        """(ids, D): D[x] is the combination of Rebuild's k survivors (in slot
        order, ids) that gives shard x: E . inv(E[ids])."""
        key = bytes(np.asarray(er_row, dtype=np.uint8) != 0)
        if key not in self._D:
            ids = survivors(er_row, self.k, self.n)
            if ids is None:
                raise Refused(RS_ENOT_ENOUGH)
            if ids == list(range(self.k)):
                D = self.E
            else:
                inv = np_rs.invert(self.E[ids])
                assert inv is not None
                D = np_rs.matmul(self.E, inv)
            self._D[key] = (ids, D)
        return self._D[key]

    def _apply(self, D, targets, slot, s, ids, length):
        if not targets:
            return []
        return oracle.matmul_stripe(np.ascontiguousarray(D[targets]), [self.mem.view(slot(s, i), length) for i in ids])

    def _enough(self, er, rows=None):
        """"A stripe with more than m erasures -> RS_ENOT_ENOUGH (nothing is launched)"."""
        for s in (range(len(er)) if rows is None else rows):
            if int((er[s] != 0).sum()) > self.m:
                raise Refused(RS_ENOT_ENOUGH)

    def _check(self, slot, s, er_row, S):
        """rs_verify_degraded: "the lowest byte offset o < shard_len at which
        the PRESENT shards of stripe s do not lie on one codeword, or
        RS_VERIFY_CLEAN.  For a stripe with e erasures the k survivors Rebuild
        chooses recompute the other m - e present shards, which are compared
        with the stored ones ... A stripe with exactly m erasures has no
        redundancy left: RS_VERIFY_CLEAN."  Returns (first_bad, the offsets
        below S at which any compared shard differs)."""
        ids, D = self.decode_matrix(er_row)
        comp = [i for i in range(self.n) if not er_row[i] and i not in ids]
        bad = np.zeros(S, dtype=bool)
        for i, c in zip(comp, self._apply(D, comp, slot, s, ids, S)):
            bad |= c != self.mem.view(slot(s, i), S)
        cols = np.flatnonzero(bad)
        return (int(cols[0]) if cols.size else CLEAN), cols

    def _codeword(self, slot, s, er_row, S, cols, failed=None):
        """rs_correct_columns: "a codeword lies within Hamming distance
        floor((r - k) / 2) of y: it is unique".  The oracle's Correct over the
        columns `cols` of the present shards; (present ids, their codeword
        bytes at those columns).  The model is given no column beyond the
        radius ("may ... land on another codeword"), unless the caller passes
        a list for them: then "a column beyond the radius ... is left alone
        while the others are corrected", the oracle deciding column by column
        which those are, and their positions in cols are appended to it
        (_columns does so only while `beyond` is set, which the one step that
        damages a stripe past the radius on purpose does: anywhere else such a
        column is a damage plan gone wrong and is reported as that)."""
        pres = [i for i in range(self.n) if not er_row[i]]
        t = (len(pres) - self.k) // 2
        y = np.stack([self.mem.view(slot(s, i), S)[cols] for i in pres])
        word, todo, suspects, tried, step = np.empty_like(y), np.arange(len(cols)), set(), None, 8
        while todo.size:
            # the oracle's Berlekamp-Welch, a few columns at a time ...
            head, todo = todo[:step], todo[step:]
            rc, data = (1, None) if step > 8 else oracle.decode_correct(
                self.E, self.k, self.n, [(i, y[j, head].tobytes()) for j, i in enumerate(pres)])
            if rc != 0 and failed is not None:
                data = np.zeros((self.k, len(head)), dtype=np.uint8)
                lost = []
                for q, c in enumerate(head):     # one of them is beyond the radius: which
                    rc1, d1 = self._decode_column(pres, y[:, c])
                    if rc1 != 0:
                        lost.append(q)
                    else:
                        data[:, q] = d1
                step = 64 if len(lost) == len(head) else 8   # a run of them: no more calls for eight at once
                if step == 64:
                    word[:, head] = y[:, head]
                    failed += [int(c) for c in head]
                    continue
                data = data.tobytes()
            else:
                assert rc == 0, ("the model was given a column beyond the decoding radius", rc)
                lost = []
            d = np.frombuffer(data, dtype=np.uint8).reshape(self.k, len(head))
            word[:, head] = np.stack(oracle.matmul_stripe(np.ascontiguousarray(self.E[pres]), [r.copy() for r in d]))
            if lost:
                word[:, head[lost]] = y[:, head[lost]]
                failed += [int(c) for c in head[lost]]
            suspects |= {j for j in range(len(pres)) if (word[j, head] != y[j, head]).any()}
            good = [j for j in range(len(pres)) if j not in suspects][:self.k]
            if not todo.size or len(good) < self.k:
                continue
            # ... and for the rest the codeword through k shards that were right
            # so far, wherever it lies within the radius: there it is the
            # unique one.  The columns where it does not go round again.
            key = tuple(pres[j] for j in good) + (-1,) + tuple(pres)
            if key == tried:    # the columns left have been held against this codeword already
                continue
            tried = key
            if key not in self._D:
                self._D[key] = np_rs.matmul(self.E[pres], np_rs.invert(self.E[[pres[j] for j in good]]))
            cand = np.stack(oracle.matmul_stripe(self._D[key], [y[j, todo].copy() for j in good]))
            ok = (cand != y[:, todo]).sum(axis=0) <= t
            word[:, todo[ok]] = cand[:, ok]
            todo = todo[~ok]
        return pres, word

    def _decode_column(self, pres, column):
        """oracle.decode_correct for one column of the shards pres, through
        call arrays that are built once per set of present shards."""
        key = ("column",) + tuple(pres)
        if key not in self._D:
            col, out = np.empty(len(pres), dtype=np.uint8), np.zeros(self.k, dtype=np.uint8)
            nums = (ctypes.c_int * len(pres))(*pres)
            ptrs = (ctypes.c_void_p * len(pres))(*[col.ctypes.data + j for j in range(len(pres))])
            self._D[key] = (col, out, nums, ptrs, np.ascontiguousarray(self.E))
        col, out, nums, ptrs, E = self._D[key]
        col[:] = column
        rc = oracle.lib().orc_decode_correct(E.ctypes.data, self.k, self.n, ctypes.addressof(nums),
                                             ctypes.addressof(ptrs), len(pres), 1, out.ctypes.data)
        return rc, out.copy()

    def _fb(self, first_bad, stripes):
        return self.mem.view(first_bad, 4 * stripes).view(np.uint32)

    # ---- encode / verify / reconstruct -----------------------------------------
    def _encode(self, slot, S, stripes):
        R = r16(S)
        for s in range(stripes):
            par = self._apply(self.E, list(range(self.k, self.n)), slot, s, range(self.k), R)
            for t, p in enumerate(par):
                self.mem.view(slot(s, self.k + t), R)[:] = p
                self.mem.wrote(slot(s, self.k + t), S)

    def encode_stripes(self, data, dss, parity, pss, pitch, S, stripes):
        """"rs_encode_stripes: parity of every stripe"; "bytes between
        shard_len and the next multiple of 16 are coded too"."""
        self._encode(self.strided(data, dss, parity, pss, pitch), S, stripes)

    def _verify(self, slot, S, stripes, er, first_bad):
        self._enough(er)
        if S == 0 or stripes == 0:
            return
        fb = self._fb(first_bad, stripes)
        for s in range(stripes):
            fb[s] = self._check(slot, s, er[s], S)[0]

    def verify_stripes(self, data, dss, parity, pss, pitch, S, stripes, first_bad):
        """"with no flag set at all the call is rs_verify_stripes"."""
        self._verify(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(None, stripes), first_bad)

    def verify_degraded(self, data, dss, parity, pss, pitch, S, stripes, erased, first_bad):
        self._verify(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes), first_bad)

    def verify_ptrs(self, tab, S, stripes, first_bad, erased=None):
        """"rs_verify_ptrs is rs_verify_degraded ... on that placement"."""
        self._verify(self.table(tab, stripes), S, stripes, self.flags(erased, stripes), first_bad)

    def _reconstruct(self, slot, S, stripes, er, first_bad=None):
        """"Every erased shard, data or parity, is regenerated in place from k
        survivors chosen like infectious Rebuild".  Checked repair: "the slot
        of every erased shard holds the round_up(shard_len, 16) bytes
        rs_reconstruct_stripes would have written there, bit for bit, whether
        or not the stripe's check passes"; "first_bad[s] is what
        rs_verify_degraded would have written for the stripes as they were
        before the call"."""
        self._enough(er)
        if S == 0 or stripes == 0:
            return
        R = r16(S)
        for s in range(stripes):
            if first_bad is not None:
                self._fb(first_bad, stripes)[s] = self._check(slot, s, er[s], S)[0]
            X = [i for i in range(self.n) if er[s, i]]
            ids, D = self.decode_matrix(er[s])
            for i, v in zip(X, self._apply(D, X, slot, s, ids, R)):
                self.mem.view(slot(s, i), R)[:] = v
                self.mem.wrote(slot(s, i), S)

    def reconstruct_stripes(self, data, dss, parity, pss, pitch, S, stripes, erased):
        self._reconstruct(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes))

    def reconstruct_ptrs(self, tab, S, stripes, erased):
        self._reconstruct(self.table(tab, stripes), S, stripes, self.flags(erased, stripes))

    def reconstruct_checked(self, data, dss, parity, pss, pitch, S, stripes, erased, first_bad):
        self._reconstruct(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes),
                          first_bad)

    def reconstruct_checked_ptrs(self, tab, S, stripes, erased, first_bad):
        self._reconstruct(self.table(tab, stripes), S, stripes, self.flags(erased, stripes), first_bad)

    # ---- scrub ---------------------------------------------------------------
    def _columns(self, slot, S, stripes, er):
        """rs_correct_columns: "exactly the bytes that differ from it are
        overwritten with its values"; "corrected[s*n + i] = the bytes of shard
        i of stripe s that the call changed; 0 for erased shards and clean
        stripes"; "Never read for comparison and never written: the slots of
        erased shards, bytes at offsets >= shard_len"; "An inconsistent stripe
        with r - k < 2 ends RS_ETOO_MANY_ERRORS unwritten"; "Codes with m > 16
        -> RS_EINVAL"."""
        self._enough(er)
        status, corrected = [RS_OK] * stripes, [0] * (stripes * self.n)
        if S == 0 or stripes == 0 or self.m == 0:
            return status, corrected
        if self.m > 16:
            raise Refused(RS_EINVAL)
        for s in range(stripes):
            fb, cols = self._check(slot, s, er[s], S)
            if fb == CLEAN:
                continue
            if self.m - int((er[s] != 0).sum()) < 2:
                status[s] = RS_ETOO_MANY_ERRORS
                continue
            failed = [] if self.beyond else None
            pres, word = self._codeword(slot, s, er[s], S, cols, failed)
            if failed:
                status[s] = RS_ETOO_MANY_ERRORS
            for i, w in zip(pres, word):
                stored = self.mem.view(slot(s, i), S)
                diff = stored[cols] != w
                stored[cols[diff]] = w[diff]
                corrected[s * self.n + i] = int(diff.sum())
        return status, corrected

    def correct_columns(self, data, dss, parity, pss, pitch, S, stripes, erased=None):
        return self._columns(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes))

    def correct_columns_ptrs(self, tab, S, stripes, erased=None):
        return self._columns(self.table(tab, stripes), S, stripes, self.flags(erased, stripes))

    def _shards(self, slot, S, stripes, er):
        """rs_correct_degraded: "Repairs every stripe with e erasures in which
        at most floor((m - e) / 2) present shards hold wrong bytes ... by
        regenerating the located shards in place.  The erased shards are NOT
        filled in"; "rewritten is set for located shards only, never for erased
        ones.  An inconsistent stripe with m - e < 2 ends RS_ETOO_MANY_ERRORS
        with nothing in it written."""
        self._enough(er)
        status, rewritten = [RS_OK] * stripes, bytearray(stripes * self.n)
        if S == 0 or stripes == 0:
            return status, bytes(rewritten)
        for s in range(stripes):
            fb, cols = self._check(slot, s, er[s], S)
            if fb == CLEAN:
                continue
            t = (self.m - int((er[s] != 0).sum())) // 2
            if t < 1:
                status[s] = RS_ETOO_MANY_ERRORS
                continue
            pres, word = self._codeword(slot, s, er[s], S, cols)
            located = [(i, w) for i, w in zip(pres, word) if (self.mem.view(slot(s, i), S)[cols] != w).any()]
            assert len(located) <= t, "the model was given more wrong shards than the shard scrub repairs"
            for i, w in located:
                self.mem.view(slot(s, i), S)[cols] = w
                self.mem.wrote(slot(s, i), S)
                rewritten[s * self.n + i] = 1
        return status, bytes(rewritten)

    def correct_stripes(self, data, dss, parity, pss, pitch, S, stripes):
        """"with no flag set it is rs_correct_stripes"."""
        return self._shards(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(None, stripes))

    def correct_degraded(self, data, dss, parity, pss, pitch, S, stripes, erased):
        return self._shards(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes))

    # ---- update / read / combine -------------------------------------------------
    def update_stripes(self, data, dss, parity, pss, pitch, S, stripes, updates):
        self.update_degraded(data, dss, parity, pss, pitch, S, stripes, bytes(stripes * self.n), updates)

    def update_degraded(self, data, dss, parity, pss, pitch, S, stripes, erased, updates):
        """"every PRESENT parity shard r becomes parity[r] ^= sum_{c in U}
        E[k + r][c] * (old_c ^ new_c).  For c in U_p old_c is read from the
        shard's slot, which then takes the new contents.  For c in U_x old_c
        is regenerated from the k survivors Rebuild chooses for X, read in
        their state before the call ...; the slot of c is NOT written";
        "Stripes and shards not listed are neither read nor written"; src
        holds "round_up(shard_len, 16) readable bytes, all of which are coded
        and committed"; "A listed stripe with more than m erasures whose
        changed shards are all present is served"."""
        self._update(self.strided(data, dss, parity, pss, pitch), S, self.flags(erased, stripes), updates)

    def _update(self, slot, S, er, updates):
        R = r16(S)
        by = collections.OrderedDict()
        for s, c, src in updates:
            by.setdefault(int(s), []).append((int(c), src))
        for s, ch in by.items():
            if any(er[s, c] for c, _ in ch):
                self._enough(er, [s])
        if S == 0:
            return
        writes = []
        for s, ch in by.items():
            gone = [c for c, _ in ch if er[s, c]]
            old = {}
            if gone:
                ids, D = self.decode_matrix(er[s])
                old = dict(zip(gone, self._apply(D, gone, slot, s, ids, R)))
            delta = []
            for c, src in ch:
                new = self.mem.view(src, R).copy()
                delta.append(new ^ (old[c] if c in old else self.mem.view(slot(s, c), R)))
                if c not in old:
                    writes.append((slot(s, c), new))
            coef = np.ascontiguousarray(self.E[self.k:][:, [c for c, _ in ch]])
            for r, p in enumerate(oracle.matmul_stripe(coef, delta) if self.m else []):
                if not er[s, self.k + r]:
                    writes.append((slot(s, self.k + r), self.mem.view(slot(s, self.k + r), R) ^ p))
        for addr, v in writes:
            self.mem.view(addr, R)[:] = v
            self.mem.wrote(addr, S)

    def read_stripes(self, data, dss, parity, pss, pitch, S, stripes, erased, reads):
        """"a shard that is not erased is copied; an erased one is computed
        from the k survivors Rebuild chooses for the stripe's erasure set";
        "round_up(shard_len, 16) bytes of dst are written; those past
        shard_len are unspecified"."""
        self._read(self.strided(data, dss, parity, pss, pitch), S, self.flags(erased, stripes), reads)

    def _read(self, slot, S, er, reads):
        R = r16(S)
        for s, i, _ in reads:
            if er[s, i]:
                self._enough(er, [s])
        if S == 0:
            return
        for s, i, dst in reads:
            if er[s, i]:
                ids, D = self.decode_matrix(er[s])
                v = self._apply(D, [i], slot, s, ids, R)[0]
            else:
                v = self.mem.view(slot(s, i), R).copy()
            self.mem.view(dst, R)[:] = v
            self.mem.wrote(dst, S)

    def combine(self, jobs, length):
        """"dst[r] = sum_c coef[r * nsrc + c] * src[c] (accumulate == 0), dst[r]
        ^= ... (accumulate == 1)"; "round_up(len, 16) bytes of every src are
        read and of every dst are written, those past len being unspecified"."""
        R = r16(length)
        if length == 0:
            return
        outs = []
        for src, dst, coef, acc in jobs:
            c = np.frombuffer(bytes(coef), dtype=np.uint8).reshape(len(dst), len(src))
            v = oracle.matmul_stripe(np.ascontiguousarray(c), [self.mem.view(a, R).copy() for a in src])
            outs += [(d, x ^ self.mem.view(d, R) if acc else x) for d, x in zip(dst, v)]
        for d, x in outs:
            self.mem.view(d, R)[:] = x
            self.mem.wrote(d, length)

    def pattern_rows(self, erased):
        """"row t (t < *count) is the combination of the k survivors (Rebuild's
        choice) that regenerates the t-th erased shard in increasing id order"."""
        er = np.frombuffer(bytes(erased), dtype=np.uint8)
        ids, D = self.decode_matrix(er)
        X = [i for i in range(self.n) if er[i]]
        return bytes(np.ascontiguousarray(D[X]).reshape(-1)) if X else b"", len(X)

    def pattern_survivors(self, erased):
        ids = survivors(np.frombuffer(bytes(erased), dtype=np.uint8), self.k, self.n)
        if ids is None:
            raise Refused(RS_ENOT_ENOUGH)
        return ids

    # ---- scattered-shard I/O -----------------------------------------------------
    def encode_ptrs(self, tab, S, stripes):
        """"rs_encode_ptrs is rs_encode_stripes on that placement: parity shard
        r of stripe s is written at shard_ptrs[s * n + k + r], and its
        round_up(shard_len, 16) bytes are bit for bit what rs_encode_stripes
        writes for the same data"; "m == 0: RS_OK"."""
        if self.m and S:
            self._encode(self.table(tab, stripes), S, stripes)

    def update_ptrs(self, tab, S, stripes, updates, offset=0):
        """"the call works on bytes [shard_offset, shard_offset + shard_len) of
        every slot it touches, and src holds the slice's new bytes from its
        start"; "Only the table entries of a listed stripe's changed shards
        and of its m parity shards are loaded" (the table is read entry by
        entry, as each is needed)."""
        at = self.table(tab, stripes)
        self._update(lambda s, i: at(s, i) + offset, S, self.flags(None, stripes), updates)

    def read_ptrs(self, tab, S, stripes, erased, reads, offset=0):
        """"A present wanted shard is copied; an erased one is computed from
        the k survivors Rebuild chooses"; "Nothing named by the table is
        written, and the table entries of erased shards are never loaded";
        "bytes [shard_offset, shard_offset + shard_len) of the slots are read
        and dst receives the slice from its start"."""
        at = self.table(tab, stripes)
        self._read(lambda s, i: at(s, i) + offset, S, self.flags(erased, stripes), reads)

    # ---- a length per stripe -----------------------------------------------------
    def _each(self, tab, shard_lens, stripes, erased):
        """"Stripe s is treated exactly as the equal-length call would treat it
        if it were called on that stripe alone with shard_len = shard_lens[s]";
        "RS_ENOT_ENOUGH when any stripe has more than m erasures", a stripe
        without bytes included, before anything is written.  The lengths are
        copied at once: "is not retained".  Yields (s, its length, its slot
        function as stripe 0, its flags)."""
        lens, er, at = [int(x) for x in shard_lens], self.flags(erased, stripes), self.table(tab, stripes)
        assert len(lens) == stripes
        self._enough(er)
        return [(s, lens[s], (lambda s: lambda _, i: at(s, i))(s), er[s:s + 1]) for s in range(stripes)]

    def verify_ptrs_lens(self, tab, shard_lens, stripes, first_bad, erased=None):
        """"a stripe with shard_lens[s] == 0 ... reads nothing, writes nothing,
        gets RS_VERIFY_CLEAN"; "RS_OK with nothing written for stripes == 0 or
        when every length is 0"."""
        each = self._each(tab, shard_lens, stripes, erased)
        if not any(L for _, L, _, _ in each):
            return
        for s, L, slot, er in each:
            if L:
                self._verify(slot, L, 1, er, first_bad + 4 * s)
            else:
                self._fb(first_bad + 4 * s, 1)[0] = CLEAN

    def reconstruct_checked_ptrs_lens(self, tab, shard_lens, stripes, erased, first_bad):
        each = self._each(tab, shard_lens, stripes, erased)
        if not any(L for _, L, _, _ in each):
            return
        for s, L, slot, er in each:
            if L:
                self._reconstruct(slot, L, 1, er, first_bad + 4 * s)
            else:
                self._fb(first_bad + 4 * s, 1)[0] = CLEAN

    def correct_columns_ptrs_lens(self, tab, shard_lens, stripes, erased=None):
        """"m > 16" -> RS_EINVAL; "a stripe with shard_lens[s] == 0 ... ends
        RS_OK with zero corrected"."""
        each = self._each(tab, shard_lens, stripes, erased)
        status, corrected = [RS_OK] * stripes, [0] * (stripes * self.n)
        if self.m == 0 or not any(L for _, L, _, _ in each):
            return status, corrected
        if self.m > 16:
            raise Refused(RS_EINVAL)
        for s, L, slot, er in each:
            if L:
                st, co = self._columns(slot, L, 1, er)
                status[s], corrected[s * self.n:(s + 1) * self.n] = st[0], co
        return status, corrected

    # ---- sector checksums --------------------------------------------------------
    def _sums(self, slot, S, stripes, er, sector):
        """"the checksum of sector j covers the bytes [j * sector_len, min((j +
        1) * sector_len, shard_len)) and nothing else -- never the padding up
        to 16 or the pitch gap"; "The slots of erased shards are never
        dereferenced".  {(s, i): uint32[nsec]} of the present shards."""
        ids = [(s, i) for s in range(stripes) for i in range(self.n) if not er[s, i]]
        return dict(zip(ids, crc32c_sectors([self.mem.view(slot(s, i), S) for s, i in ids], sector)))

    def _crcs(self, crcs, stripes, crc_pitch):
        return self.mem.view(crcs, 4 * stripes * self.n * crc_pitch).view(np.uint32).reshape(stripes * self.n, crc_pitch)

    def _crc_store(self, slot, S, stripes, er, sector, crcs, crc_pitch):
        """"computes and stores the checksums of every present shard; the
        entries of erased shards are left as they are"; "entries between nsec
        and crc_pitch are never read or written"."""
        if S == 0 or stripes == 0:
            return
        tab = self._crcs(crcs, stripes, crc_pitch)
        for (s, i), c in self._sums(slot, S, stripes, er, sector).items():
            tab[s * self.n + i, :len(c)] = c

    def _crc_check(self, slot, S, stripes, er, sector, crcs, crc_pitch, first_bad):
        """"first_bad ... gets, at [s * n + i], the lowest sector index of
        shard i of stripe s whose bytes do not match the stored checksum, or
        RS_VERIFY_CLEAN; an erased shard gets RS_VERIFY_CLEAN.  Writes nothing
        but first_bad"."""
        if S == 0 or stripes == 0:
            return
        tab, fb = self._crcs(crcs, stripes, crc_pitch), self._fb(first_bad, stripes * self.n)
        fb[:] = CLEAN
        for (s, i), c in self._sums(slot, S, stripes, er, sector).items():
            bad = np.flatnonzero(tab[s * self.n + i, :len(c)] != c)
            if bad.size:
                fb[s * self.n + i] = int(bad[0])

    def crc32c_stripes(self, data, dss, parity, pss, pitch, S, stripes, sector, crcs, crc_pitch, erased=None):
        self._crc_store(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes), sector,
                        crcs, crc_pitch)

    def crc32c_ptrs(self, tab, S, stripes, sector, crcs, crc_pitch, erased=None):
        self._crc_store(self.table(tab, stripes), S, stripes, self.flags(erased, stripes), sector, crcs, crc_pitch)

    def crc32c_check_stripes(self, data, dss, parity, pss, pitch, S, stripes, sector, crcs, crc_pitch, first_bad,
                             erased=None):
        self._crc_check(self.strided(data, dss, parity, pss, pitch), S, stripes, self.flags(erased, stripes), sector,
                        crcs, crc_pitch, first_bad)

    def crc32c_check_ptrs(self, tab, S, stripes, sector, crcs, crc_pitch, first_bad, erased=None):
        self._crc_check(self.table(tab, stripes), S, stripes, self.flags(erased, stripes), sector, crcs, crc_pitch,
                        first_bad)

    def correct_crc32c(self, data, dss, parity, pss, pitch, S, stripes, sector, crcs, crc_pitch, erased=None):
        """The header's steps: "1. every present shard is checked; B(s) is the
        set of present shards of stripe s with a mismatching sector, X(s) its
        erased shards; 2. B empty: the stripe is RS_OK and untouched (a clean
        stripe with more than m erasures too); 3. |X + B| > m: the stripe is
        RS_ETOO_MANY_ERRORS and nothing in it is written; 4. otherwise every
        shard of B is regenerated in place, whole, from the k survivors
        Rebuild chooses for X + B ...; the slots of X are neither read nor
        written; 5. the regenerated shards are checked against their stored
        checksums again ...; one that still mismatches makes its stripe
        RS_ETOO_MANY_ERRORS".  "RS_ENOT_ENOUGH, with nothing written, when a
        stripe with more than m erasures also has a mismatch.  Checksums are
        never written by this call"."""
        slot, er = self.strided(data, dss, parity, pss, pitch), self.flags(erased, stripes)
        status, rewritten = [RS_OK] * stripes, bytearray(stripes * self.n)
        if S == 0 or stripes == 0:
            return status, bytes(rewritten)
        tab, R = self._crcs(crcs, stripes, crc_pitch), r16(S)
        B = [[] for _ in range(stripes)]
        for (s, i), c in self._sums(slot, S, stripes, er, sector).items():
            if (tab[s * self.n + i, :len(c)] != c).any():
                B[s].append(i)
        for s in range(stripes):
            if B[s] and int((er[s] != 0).sum()) > self.m:
                raise Refused(RS_ENOT_ENOUGH)
        for s in range(stripes):
            if not B[s]:
                continue
            known = er[s].copy()
            known[B[s]] = 1
            if int((known != 0).sum()) > self.m:
                status[s] = RS_ETOO_MANY_ERRORS
                continue
            ids, D = self.decode_matrix(known)
            for i, v in zip(B[s], self._apply(D, B[s], slot, s, ids, R)):
                self.mem.view(slot(s, i), R)[:] = v
                self.mem.wrote(slot(s, i), S)
                rewritten[s * self.n + i] = 1
                c = crc32c_sectors([v[:S]], sector)[0]
                if (tab[s * self.n + i, :len(c)] != c).any():
                    status[s] = RS_ETOO_MANY_ERRORS
        return status, bytes(rewritten)


# =============================================================================
# The scenario: geometry, driver, ledger
# =============================================================================
PTRS = ("ptrs", "ptrs_io", "ptrs_lens")      # the placements with an address table
KINDS = ("update", "update_degraded", "read", "lose", "damage", "verify", "checked", "columns", "shards",
         "reconstruct")
NROWS = 64        # rows of the source / destination pool
NFB = 96          # first_bad rows: every verdict of a run keeps its own
WALK = 12
LEDGER = {}       # scenario id -> Counter of op kinds and damaged stripes


def defined_kinds(k, n, ptrs=False):
    """The op kinds the header defines for a code and a placement: with m == 0
    there is nothing to lose, damage, regenerate or scrub shard by shard, and
    the pointer placement has no shard-level scrub."""
    if n == k:
        return ("update", "update_degraded", "read", "verify", "checked", "columns")
    return tuple(x for x in KINDS if not (ptrs and x == "shards"))


def random_code(seed):
    """The seeded random codes: 1 <= k <= 72, 1 <= m <= 20."""
    rng = np.random.default_rng(9000 + seed)
    k = int(rng.integers(1, 73))
    return k, k + int(rng.integers(1, 21))


class Mismatch(AssertionError):
    pass


class Scene:
    """The buffers of a scenario: the stripes (a strided_image.Layout or
    Pool), a pool of source / destination rows, the first_bad rows, and in
    pointer mode the address table.  All of it seeded random bytes."""

    def __init__(self, k, n, S, stripes, placement, seed):
        self.k, self.n, self.S, self.stripes, self.placement = k, n, S, stripes, placement
        self.ptrs = placement in PTRS
        self.G = Pool(k, n, S, stripes, seed) if self.ptrs else Layout(k, n, S, stripes, seed, placement)
        self.pitch = r16(S) + 32
        rng = np.random.default_rng(seed + 77)
        self.names = ["pool"] if self.ptrs else list(self.G.names)
        self.init = [b.copy() for b in self.G.pristine]
        self.ROWS = len(self.init)
        self.names.append("rows")
        self.init.append(rng.integers(0, 256, size=GUARD + NROWS * self.pitch + GUARD, dtype=np.uint8))
        self.FB = len(self.init)
        self.names.append("first_bad")
        self.init.append(rng.integers(0, 256, size=GUARD + NFB * stripes * 4 + GUARD, dtype=np.uint8))
        if self.ptrs:
            self.TAB = len(self.init)
            self.names.append("table")
            self.init.append(np.zeros(stripes * n * 8, dtype=np.uint8))
        for s in range(stripes):    # the parity slots hold garbage before the encode
            for i in range(k, n):
                b, o = self.at(s, i)
                self.init[b][o:o + self.pitch] = rng.integers(0, 256, size=self.pitch, dtype=np.uint8)

    def at(self, s, i):
        if self.ptrs:
            return 0, self.G.row_at(self.G.rows[s, i])
        return self.G.shard_at(s, i)

    def table_bytes(self, bases):
        return np.ascontiguousarray(self.G.table(bases[0]).reshape(-1)).view(np.uint8)

    def where(self, name, off):
        """A buffer offset as (stripe, shard, offset) or what else lies there."""
        if name == "first_bad":
            q = (off - GUARD) // 4
            inside = 0 <= q < NFB * self.stripes
            return f"first_bad row {q // self.stripes} stripe {q % self.stripes}" if inside else "guard"
        if name == "rows":
            q, r = divmod(off - GUARD, self.pitch)
            return f"row {q} +{r}" if 0 <= q < NROWS else "guard"
        if name == "table":
            return f"table entry {off // 8}"
        b = self.names.index(name)
        for s in range(self.stripes):
            for i in range(self.n):
                bb, o = self.at(s, i)
                if bb == b and o <= off < o + self.pitch:
                    d = off - o
                    if d < self.S:
                        return (s, i, d)
                    return f"pad of {(s, i)}" if d < r16(self.S) else f"pitch padding of {(s, i)}"
        return "gap/guard/decoy"


def _norm(v):
    if isinstance(v, (bytes, bytearray)):
        return list(v)
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, (tuple, list)):
        return [_norm(x) for x in v]
    return v


class Driver:
    """Runs one scenario on an engine and on the model, op by op."""

    def __init__(self, make_engine, k, n, S, stripes, placement, seed, gran, walk=WALK, ident=None):
        assert gran in ("every", "async")
        self.k, self.n, self.m, self.S, self.stripes = k, n, n - k, S, stripes
        self.placement, self.seed, self.gran, self.walk = placement, seed, gran, walk
        self.scene = self.make_scene()
        self.ptrs = self.scene.ptrs
        self.L = self.lengths()
        self.model = Model(k, n, Memory(self.scene.names, self.scene.init))
        self.engine = make_engine(k, n, self.scene.names, self.scene.init)
        self.rng = np.random.default_rng(seed)
        self.truth = np.concatenate([self.scene.G.payload, self.scene.G.ref], axis=1).copy()
        self.er = np.zeros((stripes, n), dtype=np.uint8)
        self.op, self.opname, self.nfb, self.nrow, self.in_skeleton = 0, "start", 0, 0, False
        self.ledger = LEDGER.setdefault(ident or (k, n, S, stripes, placement, seed, gran), collections.Counter())
        self.ledger.clear()
        if self.ptrs:
            for e in (self.model, self.engine):
                e.poke(self.scene.TAB, 0, self.scene.table_bytes(e.bases))
                if hasattr(self.scene, "TABIO"):
                    e.poke(self.scene.TABIO, 0, self.scene.table_bytes(e.bases))

    # ---- plumbing --------------------------------------------------------------
    def make_scene(self):
        return Scene(self.k, self.n, self.S, self.stripes, self.placement, self.seed)

    def lengths(self):
        """The shard length of every stripe: S, but for the placement with a
        length per stripe."""
        return [self.S] * self.stripes

    def what(self):
        return (f"seed {self.seed} RS({self.k},{self.n}) S={self.S} x{self.stripes} {self.placement} "
                f"{self.gran}, op {self.op} {self.opname}")

    def both(self, name, fn, sync=False):
        """One engine call on the model and on the engine; what it returns (or
        the code it is refused with) is compared at once."""
        self.op += 1
        self.opname = name
        self.ledger["call " + name] += 1
        res = []
        for e in (self.model, self.engine):
            try:
                res.append(["ok", _norm(fn(e))])
            except Exception as x:  # Refused, rsmi.RSError
                if not hasattr(x, "code"):
                    raise
                res.append(["refused", x.code])
        if res[0] != res[1]:
            raise Mismatch(f"{self.what()}: returned {str(res[1])[:400]}, the model says {str(res[0])[:400]}")
        if self.gran == "every" or sync:
            self.checkpoint()
        return res[0]

    def host(self, how, buf, off, data):
        for e in (self.model, self.engine):
            getattr(e, how)(buf, off, data)

    def checkpoint(self):
        self.engine.sync()
        got, mem = self.engine.snapshot(), self.model.mem
        for b, (name, g) in enumerate(zip(mem.names, got)):
            w, lo = mem.bufs[b], mem.loose[b]
            if name == "table":
                assert np.array_equal(w, self.scene.table_bytes(self.model.bases))
                w = self.scene.table_bytes(self.engine.bases)
            if name == "table_io":      # addresses in the pool: compared as offsets into it
                w = (w.view(np.int64) - self.model.bases[0] + self.engine.bases[0]).view(np.uint8)
            bad = np.flatnonzero((g != w) & ~lo)
            if bad.size:
                first = [(int(o), self.scene.where(name, int(o)), int(g[o]), int(w[o])) for o in bad[:8]]
                raise Mismatch(f"{self.what()}: buffer {name}: {bad.size} bytes differ; "
                               f"(offset, where, engine, model) {first}")
            if name not in ("table", "table_io"):
                w[lo] = g[lo]
                lo[:] = False

    def sargs(self, e, o=0, S=None):
        a = self.scene.G.args(e.bases)
        return (a[0] + o, a[1], a[2] + o, a[3], a[4], self.S if S is None else S, a[6])

    def targs(self, e):
        return (e.adr(self.scene.TAB, 0), self.S, self.stripes)

    def slot(self, e, s, i, o=0):
        b, off = self.scene.at(s, i)
        return e.adr(b, off + o)

    def fbrow(self):
        assert self.nfb < NFB
        self.nfb += 1
        return GUARD + (self.nfb - 1) * self.stripes * 4

    def verdicts(self, off):
        return self.model.mem.bufs[self.scene.FB][off:off + 4 * self.stripes].view(np.uint32).copy()

    def rows(self, count):
        """`count` distinct rows of the pool (offsets in the rows buffer)."""
        assert count <= NROWS
        out = [GUARD + ((self.nrow + j) % NROWS) * self.scene.pitch for j in range(count)]
        self.nrow = (self.nrow + count) % NROWS
        return out

    def stored(self, s, i):
        b, o = self.scene.at(s, i)
        return self.model.mem.bufs[b][o:o + self.S]

    def e(self, s):
        return int(self.er[s].sum())

    def t(self, s):
        return (self.m - self.e(s)) // 2

    def wrong(self, s, er_row=None):
        er_row = self.er[s] if er_row is None else er_row
        w, L = np.zeros((self.n, self.S), dtype=bool), self.L[s]
        for i in range(self.n):
            if not er_row[i]:
                w[i, :L] = self.stored(s, i)[:L] != self.truth[s, i, :L]
        return w

    def clean(self, s):
        return not self.wrong(s).any()

    def within(self, s, w, er_row, shards_only):
        """Does damage w leave stripe s inside what the header promises to
        repair: every column within floor((r - k) / 2), and, where only the
        shard-level scrub serves the code, no more wrong shards than that."""
        t = (self.m - int(er_row.sum())) // 2
        return int(w.sum(axis=0).max(initial=0)) <= t and (not shards_only or int(w.any(axis=1).sum()) <= t)

    def retruth(self, s):
        if self.m:
            par = oracle.matmul_stripe(np.ascontiguousarray(self.model.E[self.k:]),
                                       [np.ascontiguousarray(self.truth[s, c]) for c in range(self.k)])
            self.truth[s, self.k:] = np.stack(par)

    def flags(self):
        return self.er.tobytes()

    # ---- the ops -------------------------------------------------------------
    def op_encode(self):
        if self.m == 0:
            return
        self.call_encode()

    def call_encode(self):
        if not self.ptrs:
            self.both("encode_stripes", lambda e: e.encode_stripes(*self.sargs(e)))
            return
        coef = self.model.E[self.k:].tobytes()
        self.both("combine(encode)", lambda e: e.combine(
            [([self.slot(e, s, c) for c in range(self.k)], [self.slot(e, s, i) for i in range(self.k, self.n)], coef, 0)
             for s in range(self.stripes)], self.S))

    def op_verify(self, er=None):
        er = self.er if er is None else er
        off = self.fbrow()
        self.call_verify(er, off)
        self.ledger["verify"] += 1
        return self.verdicts(off)

    def call_verify(self, er, off):
        fl = er.tobytes()
        if self.ptrs:
            self.both("verify_ptrs", lambda e: e.verify_ptrs(*self.targs(e), e.adr(self.scene.FB, off),
                                                             erased=fl if er.any() else None))
        elif er.any():
            self.both("verify_degraded", lambda e: e.verify_degraded(*self.sargs(e), fl, e.adr(self.scene.FB, off)))
        else:
            self.both("verify_stripes", lambda e: e.verify_stripes(*self.sargs(e), e.adr(self.scene.FB, off)))

    def fresh_rows(self, count):
        offs = self.rows(count)
        for o in offs:
            self.host("poke", self.scene.ROWS, o, self.rng.integers(0, 256, size=r16(self.S), dtype=np.uint8))
        return offs

    def slice_of(self, S=None):
        """(o, l) of a slice: o = 16, l up to the shard's end or a multiple of 16."""
        S = self.S if S is None else S
        if S <= 16:
            return None
        if S < 48 or self.rng.integers(2):
            return 16, S - 16
        return 16, 16 * int(self.rng.integers(1, (S - 16) // 16 + 1))

    def op_update(self, listed, sl=None, er=None):
        """listed: {stripe: [data shards]}; er: the flags of a degraded update."""
        o, l = sl or (0, self.S)
        ups = [(s, c) for s, cs in listed.items() for c in cs]
        if not ups:
            return False
        offs = self.fresh_rows(len(ups))
        kind = "update" if er is None else "update_degraded"
        R = self.scene.ROWS
        self.call_update(listed, ups, offs, o, l, er)
        for (s, c), off in zip(ups, offs):
            ll = min(l, self.L[s] - o)
            self.truth[s, c, o:o + ll] = self.model.mem.bufs[R][off:off + ll]
        for s in listed:
            self.retruth(s)
        self.ledger[kind] += 1
        if er is not None:
            self.ledger["absorbed"] += sum(int(er[s, c]) for s, c in ups)
            self.ledger["over_m"] += sum(int(er[s].sum()) > self.m for s in listed)
        return True

    def call_update(self, listed, ups, offs, o, l, er):
        fl = None if er is None else er.tobytes()
        R = self.scene.ROWS
        if not self.ptrs:
            def call(e):
                u = [(s, c, e.adr(R, off)) for (s, c), off in zip(ups, offs)]
                if er is None:
                    return e.update_stripes(*self.sargs(e, o, l), u)
                return e.update_degraded(*self.sargs(e, o, l), fl, u)
            self.both("update_stripes" if er is None else "update_degraded", call)
        else:
            self.update_by_combine(listed, dict(zip(ups, offs)), o, l, self.er if er is None else er)

    def update_by_combine(self, listed, src, o, l, er):
        """The pointer placement has no update call: rs_combine's "data holder
        turns old and new contents of a shard into the m parity deltas
        E[k + r][shard] * (old ^ new) and the parity holder accumulates them",
        the old contents of an erased changed shard coming from its decode row
        (rs_pattern_rows, rs_pattern_survivors) first."""
        gone = [(s, c) for s, cs in listed.items() for c in cs if er[s, c]]
        tmp = dict(zip(gone, self.rows(len(gone))))
        if gone:
            self.regen_old(gone, tmp, o, l, er)
        self.deltas_by_combine(listed, src, tmp, o, l, er)

    def regen_old(self, gone, tmp, o, l, er):
        R = self.scene.ROWS

        def regen(e):
            jobs = []
            for s, c in gone:
                rows, cnt = e.pattern_rows(er[s].tobytes())
                ids = e.pattern_survivors(er[s].tobytes())
                rk = int(er[s, :c].sum())
                jobs.append(([self.slot(e, s, i, o) for i in ids], [e.adr(R, tmp[(s, c)])],
                             rows[rk * self.k:(rk + 1) * self.k], 0))
            return e.combine(jobs, l)
        self.both("combine(old contents)", regen)

    def deltas_by_combine(self, listed, src, tmp, o, l, er):
        R, E = self.scene.ROWS, self.model.E

        def delta(e):
            jobs = []
            for s, cs in listed.items():
                par = [r for r in range(self.m) if not er[s, self.k + r]]
                if not par:
                    continue
                srcs, coef = [], np.zeros((len(par), 2 * len(cs)), dtype=np.uint8)
                for j, c in enumerate(cs):
                    srcs += [e.adr(R, tmp[(s, c)]) if er[s, c] else self.slot(e, s, c, o), e.adr(R, src[(s, c)])]
                    coef[:, 2 * j] = coef[:, 2 * j + 1] = E[[self.k + r for r in par], c]
                jobs.append((srcs, [self.slot(e, s, self.k + r, o) for r in par], coef.tobytes(), 1))
            return e.combine(jobs, l) if jobs else None
        self.both("combine(parity deltas)", delta)
        commit = [(s, c) for s, cs in listed.items() for c in cs if not er[s, c]]
        if commit:
            self.both("combine(commit)", lambda e: e.combine(
                [([e.adr(R, src[(s, c)])], [self.slot(e, s, c, o)], b"\1", 0) for s, c in commit], l))

    def undamaged(self, s):
        w = self.wrong(s).any(axis=1)
        return [c for c in range(self.k) if self.L[s] and not self.er[s, c] and not w[c]]

    def op_update_plain(self):
        """Some stripes untouched, some with one shard, one with min(k, 3)
        shards, then one slice update."""
        cand = [s for s in range(self.stripes) if self.e(s) == 0 and self.undamaged(s)]
        if not cand:
            return False
        order = [cand[j] for j in self.rng.permutation(len(cand))]
        listed = {}
        for j, s in enumerate(order[:max(1, len(order) - max(1, len(order) // 3))]):
            ok = self.undamaged(s)
            cnt = min(self.k, 3, len(ok)) if j == 0 else 1
            listed[s] = sorted(int(c) for c in self.rng.choice(ok, size=cnt, replace=False))
        self.op_update(listed)
        s = self.slice_stripe(order)
        sl = self.slice_of(self.L[s])
        if sl:
            self.op_update({s: [int(self.rng.choice(self.undamaged(s)))]}, sl=sl)
        return True

    def slice_stripe(self, order):
        return order[-1]

    def op_update_degraded(self):
        """Changed shards present and erased, an erased parity among the
        flags, and one stripe with more than m flags whose changed shards are
        all present (the extra flags name unchanged data shards, which the
        call neither reads nor writes)."""
        er, listed = self.er.copy(), {}
        # the stripes that can take more than m flags: one changed shard that is
        # present, and enough other present data shards to flag (the pointer
        # placement's combine form has no flags)
        can = [s for s in range(self.stripes) if not self.ptrs and self.undamaged(s) and
               self.k - 1 - int(self.er[s, :self.k].sum()) >= self.m + 1 - self.e(s)]
        over = can[int(self.rng.integers(len(can)))] if can else None
        keep = int(self.rng.integers(self.stripes))
        for s in range(self.stripes):
            ok = self.undamaged(s)
            gone = [c for c in range(self.k) if self.er[s, c]] if self.clean(s) and self.e(s) <= self.m else []
            if s == over or not self.L[s]:
                gone = []
            elif s != keep and not gone and not self.rng.integers(3):
                continue    # an unlisted stripe
            cs = ([int(self.rng.choice(ok))] if ok else []) + ([int(self.rng.choice(gone))] if gone else [])
            if cs:
                listed[s] = sorted(cs)
        if not listed:
            return False
        if over is not None:
            spare = [c for c in range(self.k) if c not in listed[over] and not er[over, c]]
            er[over, spare[:self.m + 1 - self.e(over)]] = 1
        return self.op_update(listed, er=er)

    def op_lose(self, want):
        """want: {stripe: flags to add}; the slots are overwritten with garbage
        over their whole pitch.  Flags that would leave damage beyond what the
        header promises to repair are not taken."""
        done = 0
        for s, add in want.items():
            new = self.er[s] | add
            if int(new.sum()) > self.m or not self.within(s, self.wrong(s, new), new, self.shards_only()):
                continue
            for i in np.flatnonzero(new & ~self.er[s].astype(bool)):
                b, o = self.scene.at(s, int(i))
                self.host("poke", b, o, self.rng.integers(0, 256, size=self.scene.pitch, dtype=np.uint8))
                done += 1
            self.er[s] = new
        self.op += 1
        self.opname = "lose"
        self.ledger["lose"] += 1
        if self.gran == "every":
            self.checkpoint()
        return done

    def regarbage(self):
        for s, i in zip(*np.nonzero(self.er)):
            b, o = self.scene.at(int(s), int(i))
            self.host("poke", b, o, self.rng.integers(0, 256, size=self.scene.pitch, dtype=np.uint8))

    def skeleton_sets(self, fewer=False):
        """0, 1 ... m - 1 and m erasures over the stripes, rows of
        strided_image.fixed_patterns among them."""
        k, n, m = self.k, self.n, self.m
        fixed = fixed_patterns(k, n)
        want = {}
        for s in range(self.stripes):
            row = np.zeros(n, dtype=np.uint8)
            if s % 6 == 0:       # a data and a parity shard, and redundancy left
                ids = ([int(self.rng.integers(k))] + [k + int(self.rng.integers(m))] * (m >= 4))[:max(0, m - 2)]
                if m == 1:
                    ids = []
                row[ids] = 1
            elif s % 6 == 1:     # m erasures, a data shard among them
                if m:
                    row[int(self.rng.integers(k))] = 1
                    row[self.rng.choice(np.flatnonzero(row == 0), size=m - 1, replace=False)] = 1
            elif s % 6 == 2:
                pass
            elif s % 6 in (3, 5):
                row = fixed[int(self.rng.integers(len(fixed)))].copy()
                if fewer and int(row.sum()) > max(0, m - 2):
                    row[np.flatnonzero(row)[max(0, m - 2):]] = 0
            else:
                cnt = max(0, m - 2) if fewer else max(0, m - 1)
                row[self.rng.choice(n, size=cnt, replace=False)] = 1
            want[s] = row
        return want

    def op_read(self):
        """Present and erased shards mixed, then one slice read.  Damaged
        present shards are always among them."""
        reads = []
        for s in range(self.stripes):
            if not self.L[s]:
                continue
            gone = [int(i) for i in np.flatnonzero(self.er[s])] if self.e(s) <= self.m else []
            bad = [int(i) for i in np.flatnonzero(self.wrong(s).any(axis=1))]
            pres = [int(i) for i in np.flatnonzero(self.er[s] == 0)]
            take = set(gone[:2] + gone[-1:] + bad[:2])
            if pres:
                take.add(int(self.rng.choice(pres)))
            reads += [(s, i) for i in sorted(take)]
        reads = reads[:NROWS // 2]
        got = self.read(reads, 0, self.S)
        self.slice_read(reads)
        self.ledger["read"] += 1
        return got

    def slice_read(self, reads):
        sl = self.slice_of()
        if sl:
            self.read(reads[:4], *sl)

    def read(self, reads, o, l):
        offs = self.rows(len(reads))
        self.call_read(reads, offs, o, l)
        return [(s, i, off) for (s, i), off in zip(reads, offs) if self.er[s, i]]

    def call_read(self, reads, offs, o, l):
        R, fl = self.scene.ROWS, self.flags()
        if not self.ptrs:
            self.both("read_stripes", lambda e: e.read_stripes(
                *self.sargs(e, o, l), fl, [(s, i, e.adr(R, off)) for (s, i), off in zip(reads, offs)]))
        else:
            self.by_rows(reads, offs, o, l, "combine(read)")

    def by_rows(self, reads, offs, o, l, name):
        """rs_combine's decode-row form: "a holder of some survivors of a
        stripe multiplies them by their columns of a decode row
        (rs_pattern_rows, rs_pattern_survivors)"; a present shard is a copy."""
        R = self.scene.ROWS

        def call(e):
            jobs = []
            for (s, i), off in zip(reads, offs):
                if not self.er[s, i]:
                    jobs.append(([self.slot(e, s, i, o)], [e.adr(R, off)], b"\1", 0))
                    continue
                rows, cnt = e.pattern_rows(self.er[s].tobytes())
                ids = e.pattern_survivors(self.er[s].tobytes())
                rk = int(self.er[s, :i].sum())
                jobs.append(([self.slot(e, s, x, o) for x in ids], [e.adr(R, off)],
                             rows[rk * self.k:(rk + 1) * self.k], 0))
            return e.combine(jobs, l)
        self.both(name, call)

    def op_patterns(self, regenerated):
        """rs_pattern_rows + rs_pattern_survivors + combine: the same shards
        again, which must equal what the degraded read gave."""
        if not regenerated:
            return
        for s in sorted({s for s, _, _ in regenerated}):
            fl = self.er[s].tobytes()
            self.both("pattern_rows", lambda e: (lambda r: [list(r[0][:r[1] * self.k]), r[1]])(e.pattern_rows(fl)))
            self.both("pattern_survivors", lambda e: list(e.pattern_survivors(fl)))
        reads = [(s, i) for s, i, _ in regenerated]
        offs = self.rows(len(reads))
        self.rows_again(reads, offs)
        rows = self.model.mem.bufs[self.scene.ROWS]
        for (s, i, a), b in zip(regenerated, offs):
            assert np.array_equal(rows[a:a + self.L[s]], rows[b:b + self.L[s]]), (self.what(), s, i)
        self.ledger["patterns"] += 1

    def rows_again(self, reads, offs):
        self.by_rows(reads, offs, 0, self.S, "combine(decode rows)")

    def fit(self, s, chosen, w):
        """The shards of a scattered damage plan that the scenario can take."""
        return chosen

    def shards_only(self):
        """Where rs_correct_columns refuses the code, only the shard-level scrub repairs."""
        return self.m > 16

    def offsets(self, count, S=None):
        S = self.S if S is None else S
        special = [o for o in dict.fromkeys([0, 15, 16, 4095, 4096, S - 17, S - 1]) if 0 <= o < S]
        pick = [int(special[j]) for j in self.rng.permutation(len(special))[:max(1, count // 2)]]
        pick += [int(x) for x in self.rng.integers(0, S, size=count)]
        return list(dict.fromkeys(pick))[:count]

    def op_damage(self, kind):
        """kind "scattered": at most floor((r - k) / 2) wrong shares in any
        column, several shards touched at different offsets, one column filled
        to the radius, a survivor and a compared shard among them, and a byte
        in the pad, which "is not an error".  kind "whole": at most floor((m -
        e) / 2) shards, arbitrary bytes.  A stripe with r - k < 2 gets none."""
        hit = 0
        for s in range(self.stripes):
            t, er_row, S = self.t(s), self.er[s], self.L[s]
            if t < 1 or self.e(s) > self.m or not S:
                continue
            pres = [int(i) for i in np.flatnonzero(er_row == 0)]
            w = self.wrong(s)
            plan = []   # (shard, offset, mask)
            if kind == "whole":
                room = t - int(w.any(axis=1).sum())
                for i in self.rng.permutation(pres)[:max(0, min(room, 1 + int(self.rng.integers(t))))]:
                    plan.append((int(i), 0, self.rng.integers(0, 256, size=S, dtype=np.uint8)))
            else:
                ids = survivors(er_row, self.k, self.n)
                comp = [i for i in pres if i not in ids]
                room = t - int(w.any(axis=1).sum()) if self.shards_only() else min(len(pres), 2 * t + 1)
                chosen = list(dict.fromkeys([int(self.rng.choice(ids)), int(self.rng.choice(comp))] +
                                            [int(i) for i in self.rng.permutation(pres)]))[:max(0, room)]
                chosen = self.fit(s, chosen, w)
                if chosen:
                    full = self.offsets(1, S)[0]        # one column filled to the radius
                    for i in chosen[:t]:
                        plan.append((i, full, None))
                    for j, i in enumerate(chosen):      # and every shard at offsets of its own
                        for o in self.offsets(1 + j % 3, S):
                            plan.append((i, o, None))
            col = w.sum(axis=0)
            did = False
            for i, o, mask in plan:
                if mask is None:
                    if w[i, o] or col[o] >= t:
                        continue
                    mask = np.array([self.rng.integers(1, 256)], dtype=np.uint8)
                    w[i, o], col[o] = True, col[o] + 1
                b, off = self.scene.at(s, i)
                self.host("xor", b, off + o, mask)
                did = True
            if did and kind != "whole" and r16(S) > S:
                b, off = self.scene.at(s, pres[0])
                self.host("xor", b, off + S + int(self.rng.integers(r16(S) - S)),
                          np.array([0x5A], dtype=np.uint8))
            assert self.within(s, self.wrong(s), er_row, self.shards_only())
            hit += did
        self.op += 1
        self.opname = f"damage({kind})"
        self.ledger["damage"] += 1
        self.ledger["damaged_" + kind] += hit
        self.ledger["skeleton_damage_empty"] += self.in_skeleton and hit == 0
        if self.gran == "every":
            self.checkpoint()
        return hit

    def settle(self, fb=None):
        """After a repair: a stripe that is clean has its slots filled with
        the truth and drops its flags; the others keep them (rsmi.h: "Keep
        that stripe's flags")."""
        for s in range(self.stripes):
            if self.e(s) and self.e(s) <= self.m:
                full = self.wrong(s, np.zeros(self.n, dtype=np.uint8))
                if fb is not None:
                    assert (fb[s] == CLEAN) == (not self.wrong(s).any()), (self.what(), s, fb.tolist())
                if not full.any():
                    self.er[s] = 0

    def op_checked(self):
        off = self.fbrow()
        self.call_checked(self.flags(), off)
        fb = self.verdicts(off)
        self.settle(fb)
        self.ledger["checked"] += 1
        return fb

    def call_checked(self, fl, off):
        if self.ptrs:
            self.both("reconstruct_checked_ptrs",
                      lambda e: e.reconstruct_checked_ptrs(*self.targs(e), fl, e.adr(self.scene.FB, off)))
        else:
            self.both("reconstruct_checked",
                      lambda e: e.reconstruct_checked(*self.sargs(e), fl, e.adr(self.scene.FB, off)))

    def op_reconstruct(self):
        if self.m == 0 or not self.er.any():
            return False
        self.call_reconstruct(self.flags())
        self.settle()
        self.ledger["reconstruct"] += 1
        return True

    def call_reconstruct(self, fl):
        if self.ptrs:
            self.both("reconstruct_ptrs", lambda e: e.reconstruct_ptrs(*self.targs(e), fl))
        else:
            self.both("reconstruct_stripes", lambda e: e.reconstruct_stripes(*self.sargs(e), fl))

    def op_columns(self, unrepairable=True):
        """rs_correct_columns with the flags.  A clean stripe with r - k == 1
        takes the one explicit "inconsistent and unrepairable, must stay
        unwritten" byte around the call.  For m > 16 the call is refused with
        RS_EINVAL and an untouched image."""
        fl = self.flags() if self.er.any() else None
        flip = None
        if unrepairable and self.m <= 16:
            for s in range(self.stripes):
                if self.m - self.e(s) == 1 and self.clean(s) and self.L[s]:
                    i = int(self.rng.choice(np.flatnonzero(self.er[s] == 0)))
                    b, off = self.scene.at(s, i)
                    flip = (s, b, off + self.offsets(1, self.L[s])[0], np.array([self.rng.integers(1, 256)], dtype=np.uint8))
                    self.host("xor", *flip[1:])
                    self.ledger["damage"] += 1
                    break
        res = self.call_columns(fl)
        self.ledger["columns"] += 1
        if self.m > 16:
            assert res == ["refused", RS_EINVAL], (self.what(), res)
            self.ledger["columns_refused"] += 1
            return res
        assert res[0] == "ok", (self.what(), res)
        status = res[1][0]
        if flip:
            assert status[flip[0]] == RS_ETOO_MANY_ERRORS, (self.what(), status)
            self.host("xor", *flip[1:])
            self.ledger["unrepairable"] += 1
            if self.gran == "every":
                self.checkpoint()
        assert all(st == RS_OK for s, st in enumerate(status) if not flip or s != flip[0]), (self.what(), status)
        for s in range(self.stripes):
            assert self.clean(s), (self.what(), s)
        return res

    def call_columns(self, fl):
        if self.ptrs:
            return self.both("correct_columns_ptrs", lambda e: e.correct_columns_ptrs(*self.targs(e), erased=fl),
                             sync=True)
        return self.both("correct_columns", lambda e: e.correct_columns(*self.sargs(e), erased=fl), sync=True)

    def can_shards(self):
        return (self.m > 0 and not self.ptrs and
                all(int(self.wrong(s).any(axis=1).sum()) <= self.t(s) for s in range(self.stripes)))

    def op_shards(self):
        """rs_correct_stripes, or rs_correct_degraded while shards are missing
        (the pointer placement has neither: its column scrub stands in)."""
        if self.ptrs:
            return self.op_columns(unrepairable=False) if 0 < self.m <= 16 else None
        if not self.can_shards():
            self.ledger["skeleton_shards_skipped"] += self.in_skeleton
            return None
        want = sum(int(self.wrong(s).any(axis=1).sum()) for s in range(self.stripes))
        if self.er.any():
            fl = self.flags()
            degraded = sum(int(self.wrong(s).any(axis=1).sum()) for s in range(self.stripes) if self.e(s))
            res = self.both("correct_degraded", lambda e: e.correct_degraded(*self.sargs(e), fl), sync=True)
            self.ledger["correct_degraded"] += 1
            self.ledger["degraded_regenerated"] += degraded     # located shards of stripes with missing ones
        else:
            res = self.both("correct_stripes", lambda e: e.correct_stripes(*self.sargs(e)), sync=True)
            self.ledger["correct_stripes"] += 1
        assert res[0] == "ok" and all(st == RS_OK for st in res[1][0]), (self.what(), res)
        assert sum(1 for x in res[1][1] if x) == want, (self.what(), res[1][1], want)
        for s in range(self.stripes):
            assert self.clean(s), (self.what(), s)
        self.ledger["shards"] += 1
        return res

    def repair_damage(self):
        if self.m > 16 or (self.rng.integers(2) and self.can_shards() and not self.ptrs):
            return self.op_shards()
        return self.op_columns(unrepairable=False)

    # ---- the life of a store -----------------------------------------------------
    def skeleton(self):
        m = self.m
        self.op_encode()                                                    # 1
        assert (self.op_verify() == CLEAN).all(), self.what()
        self.op_update_plain()                                              # 2
        if m:
            self.op_lose(self.skeleton_sets())                              # 3
        regenerated = self.op_read()                                        # 4
        self.op_patterns(regenerated)                                       # 5
        self.op_update_degraded()                                           # 6
        if m >= 2:
            self.op_damage("scattered")                                     # 7
        first = self.op_verify()                                            # 8
        self.regarbage()                                                    # 9
        assert np.array_equal(self.op_verify(), first), self.what()
        self.op_checked()                                                   # 10
        self.op_columns()                                                   # 11
        if m > 16:
            self.op_shards()
        if m:
            fb = self.op_checked()                                          # 12
            assert (fb == CLEAN).all() and not self.er.any(), (self.what(), fb.tolist())
            if m >= 2:
                self.op_damage("whole")                                     # 13
            self.beyond_the_radius()
            self.op_shards()                                                # 14
            self.other_data()
            self.op_lose(self.skeleton_sets(fewer=True))                    # 15
            if m >= 2:
                self.op_damage("whole")
            self.op_shards()
            if not self.er.any():   # nothing is missing: lose one shard of every stripe first
                self.op_lose({s: np.eye(self.n, dtype=np.uint8)[int(self.rng.integers(self.n))]
                              for s in range(self.stripes)})
            self.op_reconstruct()                                           # 16
        self.finish()                                                       # 17

    def beyond_the_radius(self):
        pass

    def other_data(self):
        pass

    def finish(self):
        """All clean, every [0, S) the truth, the stored parity the re-encoded data."""
        if self.er.any():
            self.op_reconstruct()
        assert not self.er.any(), self.what()
        assert (self.op_verify() == CLEAN).all(), self.what()
        self.checkpoint()
        for s in range(self.stripes):
            L = self.L[s]
            data = np.stack([self.stored(s, c)[:L] for c in range(self.k)])
            assert np.array_equal(data, self.truth[s, :self.k, :L]), (self.what(), s)
            if self.m:
                par = np_rs.apply_rows(np_rs.fec_matrix(self.k, self.n)[self.k:], data)
                stored = np.stack([self.stored(s, i)[:L] for i in range(self.k, self.n)])
                assert np.array_equal(par, stored), (self.what(), s)
                assert np.array_equal(par, self.truth[s, self.k:, :L]), (self.what(), s)

    def random_walk(self):
        """WALK further ops, drawn from those whose preconditions hold."""
        kinds = self.kinds()
        done = 0
        while done < self.walk:
            kind = kinds[int(self.rng.integers(len(kinds)))]
            if not self.rng.integers(4) and any(not self.clean(s) for s in range(self.stripes)):
                kind = "read"   # damaged shards are there to be read: "copied, damaged or not"
            if kind == "update":
                ok = self.op_update_plain()
            elif kind == "update_degraded":
                ok = self.op_update_degraded()
            elif kind == "read":
                ok = self.op_read() is not None
            elif kind == "lose":
                add = {}
                for s in range(self.stripes):
                    room = self.m - self.e(s)
                    row = np.zeros(self.n, dtype=np.uint8)
                    if room > 0 and self.rng.integers(3):
                        pres = np.flatnonzero(self.er[s] == 0)
                        row[self.rng.choice(pres, size=int(self.rng.integers(1, room + 1)), replace=False)] = 1
                    add[s] = row
                ok = self.op_lose(add) > 0
            elif kind == "damage":
                ok = self.m >= 2 and not (self.ptrs and self.m > 16) and \
                    self.op_damage("whole" if self.shards_only() or self.rng.integers(2) else "scattered") > 0
            elif kind == "verify":
                ok = self.op_verify() is not None
            elif kind == "checked":
                ok = self.op_checked() is not None
            elif kind == "columns":
                ok = self.op_columns() is not None
            elif kind == "shards":
                ok = self.op_shards() is not None
            elif kind == "reconstruct":
                ok = self.op_reconstruct()
            else:
                ok = self.op_other(kind)
            done += 1 if ok else 0
        # the final repair
        if any(not self.clean(s) for s in range(self.stripes)):
            self.repair_damage()
        self.finish()

    def kinds(self):
        return defined_kinds(self.k, self.n, self.ptrs)

    def run(self):
        self.in_skeleton = True
        self.skeleton()
        self.in_skeleton = False
        self.random_walk()
        return self


# S: one column | a ragged second column | exactly one 4 KiB block chunk | a
# chunk plus one column | not a multiple of 16 | three chunks plus a ragged
# column, the bit-sliced window edge
SIZES = (16, 17, 4096, 4112, 5000, 12328)
# (k, n): two scenarios each, (S, stripes, placement), one S no multiple of 16.
# Codes the column scrub refuses (m > 16) live in the strided placements: the
# pointer placement has no other scrub to repair them with.
FIXED = {
    (10, 14): [(17, 4, "split"), (4112, 3, "ptrs")],           # the specialised kernels
    (4, 6): [(16, 3, "joined"), (5000, 2, "ptrs")],
    (8, 14): [(5000, 3, "split"), (4096, 2, "joined")],
    (64, 80): [(12328, 2, "joined"), (4096, 2, "ptrs")],
    (64, 84): [(17, 3, "split"), (4112, 2, "joined")],         # k = 64 with m > 16: row groups of 16
    (5, 9): [(12328, 2, "ptrs"), (16, 6, "split")],            # runtime k below one load batch
    (13, 18): [(17, 6, "split"), (4096, 2, "ptrs")],           # runtime k = 8 + 5, m = 5
    (9, 26): [(4112, 2, "joined"), (5000, 1, "split")],        # m = 17
    (1, 3): [(5000, 5, "ptrs"), (16, 3, "split")],             # k = 1
    (4, 5): [(17, 4, "split"), (16, 4, "ptrs")],               # m = 1
    (3, 3): [(4112, 3, "joined"), (17, 3, "ptrs")],            # m = 0
}


def scenarios():
    """[(id, k, n, S, stripes, placement, seed)]: the fixed codes and six
    seeded random ones (seeds 1..6), their (k, n) in the id."""
    out = []
    for (k, n), shapes in FIXED.items():
        for j, (S, stripes, placement) in enumerate(shapes):
            out.append((f"rs{k}_{n}-S{S}x{stripes}-{placement}", k, n, S, stripes, placement, 100 * k + n + j))
    for seed in range(1, 7):
        k, n = random_code(seed)
        rng = np.random.default_rng(7000 + seed)
        S = SIZES[(seed - 1) % len(SIZES)]
        stripes = int(rng.integers(2, 4)) if k > 32 else int(rng.integers(2, 7))
        placement = ("split", "joined", "ptrs")[seed % 3] if n - k <= 16 else ("split", "joined")[seed % 2]
        out.append((f"seed{seed}-rs{k}_{n}-S{S}x{stripes}-{placement}", k, n, S, stripes, placement, seed))
    return out


def check_ledger(ident, k, n, stripes, ptrs):
    """Every op kind the header defines for the code ran, the refusal of
    rs_correct_columns counted for m > 16, and every damage step damaged at
    least one stripe where m >= 2."""
    led, m = LEDGER[ident], n - k
    for kind in defined_kinds(k, n, ptrs):
        assert led[kind] > 0, (ident, kind, dict(led))
    if m > 16:
        assert led["columns_refused"] == led["columns"] > 0, (ident, dict(led))
    if m >= 2:
        assert led["damaged_scattered"] > 0 and led["damaged_whole"] > 0, (ident, dict(led))
        assert led["skeleton_damage_empty"] == 0, (ident, dict(led))
    if m == 1:
        assert led["unrepairable"] > 0, (ident, dict(led))
    # step 6: an erased changed shard is absorbed wherever a stripe loses a data
    # shard (the first stripe for m >= 3, the second for any m), and a stripe
    # with more than m flags is served wherever one present changed shard leaves
    # m + 1 - e spare data shards to flag: k >= m + 2 for the first stripe.  The
    # pointer placement's combine form has no flags.
    if m >= 3 or (m >= 1 and stripes >= 2):
        assert led["absorbed"] > 0, (ident, dict(led))
    if not ptrs and k >= m + 2:
        assert led["over_m"] > 0, (ident, dict(led))
    # steps 14 and 15: both shard-level scrubs ran and none was skipped; with
    # m >= 3 the first stripe of step 15 is degraded, damaged and repairable
    if not ptrs and m >= 1:
        assert led["correct_stripes"] > 0 and led["skeleton_shards_skipped"] == 0, (ident, dict(led))
    if not ptrs and m >= 3:
        assert led["correct_degraded"] > 0 and led["degraded_regenerated"] > 0, (ident, dict(led))

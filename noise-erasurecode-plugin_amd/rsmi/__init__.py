"""ctypes binding of the MI355X Reed-Solomon engine (include/rsmi.h).

Mirrors the github.com/vivint/infectious API the reference plugin calls
(/root/reference/main.go:24 import, :73/:248 NewFEC, :262 Encode, :77 Decode,
:57-69/:254-258 Share + DeepCopy) so Python callers and the tests read like
the plugin.  The shared library lib/librsmi.so is built in-tree by
``__graft_entry__.build()`` (or ``make -C noise-erasurecode-plugin_amd/csrc``);
importing this module without it raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
# RSMI_LIB points at another build of the engine (same-box A/B runs of build variants).
LIB_PATH = os.environ.get("RSMI_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "librsmi.so")

# rs_status codes (include/rsmi.h)
RS_OK = 0
RS_EINVAL_KN = -1
RS_ELEN_NOT_MULTIPLE = -2
RS_ENOT_ENOUGH = -3
RS_EBAD_SHARE_ID = -4
RS_ESINGULAR = -5
RS_ENO_SHARES = -6
RS_ESHARE_LEN = -7
RS_EINVAL = -8
RS_EDEVICE = -9
RS_ENOMEM = -10
RS_ETOO_MANY_ERRORS = -16
RS_VERIFY_CLEAN = 0xFFFFFFFF  # rs_verify_stripes: the stripe is a codeword

# Every symbol include/rsmi.h declares (checked by tests/test_capi_symbols.py).
EXPORTS = (
    "rs_new", "rs_new_on_device", "rs_free", "rs_k", "rs_n", "rs_device",
    "rs_encode_matrix", "rs_strerror", "rs_encode", "rs_decode", "rs_decode_batch", "rs_encode_batch",
    "rs_encode_stripes", "rs_reconstruct_stripes", "rs_reconstruct_ptrs", "rs_pattern_count",
    "rs_verify_ptrs", "rs_correct_columns_ptrs",
    "rs_encode_ptrs", "rs_update_ptrs", "rs_read_ptrs",
    "rs_reconstruct_checked", "rs_reconstruct_checked_ptrs",
    "rs_verify_ptrs_lens", "rs_reconstruct_checked_ptrs_lens", "rs_correct_columns_ptrs_lens",
    "rs_verify_stripes", "rs_correct_stripes", "rs_update_stripes", "rs_read_stripes",
    "rs_verify_degraded", "rs_correct_degraded", "rs_correct_columns", "rs_update_degraded", "rs_combine",
    "rs_combine_lens", "rs_encode_batch_lens", "rs_decode_batch_lens",
    "rs_crc32c_stripes", "rs_crc32c_check_stripes", "rs_crc32c_ptrs", "rs_crc32c_check_ptrs",
    "rs_correct_crc32c", "rs_crc32c_host",
    "rs_pattern_survivors",
    "rs_pattern_evictions",
    "rs_prepare_patterns",
    "rs_pattern_rows",
    "rs_pinned_alloc", "rs_pinned_free", "rs_device_alloc", "rs_device_free",
    "rs_stream_sync", "rs_fill_splitmix", "rs_kernel_name",
    "rs_blake2b_batch", "rs_blake2b_device", "rs_blake2b", "rs_blake2b_host",
    "rs_stat", "rs_arena_new", "rs_arena_alloc", "rs_arena_put", "rs_arena_reset", "rs_arena_used", "rs_arena_free",
    "rs_new_devices", "rs_member_count", "rs_member", "rs_partition",
    "rs_encode_stripes_parts", "rs_reconstruct_stripes_parts", "rs_reconstruct_spread",
)


class StripePart(ctypes.Structure):
    """rs_stripe_part (include/rsmi.h): the stripes one member holds."""

    _fields_ = [("data", ctypes.c_void_p), ("data_stripe_stride", ctypes.c_size_t),
                ("parity", ctypes.c_void_p), ("parity_stripe_stride", ctypes.c_size_t),
                ("stripes", ctypes.c_size_t), ("stream", ctypes.c_void_p)]


class ShardUpdate(ctypes.Structure):
    """rs_shard_update (include/rsmi.h): one changed data shard."""

    _fields_ = [("stripe", ctypes.c_uint64), ("shard", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("src", ctypes.c_void_p)]


def shard_updates(updates: Sequence[tuple]) -> ctypes.Array:
    """The rs_shard_update table of (stripe, shard, src_ptr) tuples."""
    return (ShardUpdate * len(updates))(*[ShardUpdate(s, i, 0, p) for s, i, p in updates])


class ShardRead(ctypes.Structure):
    """rs_shard_read (include/rsmi.h): one wanted shard and where it goes."""

    _fields_ = [("stripe", ctypes.c_uint64), ("shard", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("dst", ctypes.c_void_p)]


def shard_reads(reads: Sequence[tuple]) -> ctypes.Array:
    """The rs_shard_read table of (stripe, shard, dst_ptr) tuples."""
    return (ShardRead * len(reads))(*[ShardRead(s, i, 0, p) for s, i, p in reads])


class CombineJob(ctypes.Structure):
    """rs_combine_job (include/rsmi.h): nout combinations of nsrc buffers."""

    _fields_ = [("src", ctypes.POINTER(ctypes.c_uint64)), ("dst", ctypes.POINTER(ctypes.c_uint64)),
                ("coef", ctypes.POINTER(ctypes.c_uint8)), ("nsrc", ctypes.c_uint32), ("nout", ctypes.c_uint32),
                ("accumulate", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


def combine_jobs(jobs: Sequence[tuple]) -> ctypes.Array:
    """The rs_combine_job table of (src_ptrs, dst_ptrs, coef, accumulate)
    tuples: coef holds len(dst_ptrs) * len(src_ptrs) coefficient bytes, row
    by row.  The table keeps the host arrays its jobs point to alive."""
    arr = (CombineJob * max(len(jobs), 1))()
    keep = []
    for job, (src, dst, coef, accumulate) in zip(arr, jobs):
        coef = bytes(coef)
        if len(coef) != len(src) * len(dst):
            raise RSError(RS_EINVAL, "coef must hold nout*nsrc coefficients")
        hs, hd = (ctypes.c_uint64 * len(src))(*src), (ctypes.c_uint64 * len(dst))(*dst)
        hc = (ctypes.c_uint8 * max(len(coef), 1)).from_buffer_copy(coef or b"\0")
        keep.append((hs, hd, hc))
        job.src, job.dst, job.coef = hs, hd, hc
        job.nsrc, job.nout, job.accumulate = len(src), len(dst), int(accumulate)
    arr._keep = keep
    arr._count = len(jobs)
    return arr


class RSError(Exception):
    """Error from the engine; .code is the rs_status value."""

    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = _lib().rs_strerror(code).decode() if _LIB is not None else str(code)
        super().__init__(f"{what}: {msg} ({code})" if what else f"{msg} ({code})")


class NotEnoughShares(RSError):
    """infectious NotEnoughShares (Rebuild/Correct with fewer than k shares)."""


_LIB: Optional[ctypes.CDLL] = None


def _lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                "(the engine has no CPU fallback)")
        lib = ctypes.CDLL(LIB_PATH)
        vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        u8p = ctypes.POINTER(ctypes.c_uint8)
        sig = {
            "rs_new": (i32, [i32, i32, ctypes.POINTER(vp)]),
            "rs_new_on_device": (i32, [i32, i32, i32, ctypes.POINTER(vp)]),
            "rs_free": (None, [vp]),
            "rs_k": (i32, [vp]),
            "rs_n": (i32, [vp]),
            "rs_device": (i32, [vp]),
            "rs_encode_matrix": (i32, [vp, u8p]),
            "rs_strerror": (ctypes.c_char_p, [i32]),
            "rs_kernel_name": (ctypes.c_char_p, [vp, i32]),
            "rs_encode": (i32, [vp, vp, sz, vp]),
            "rs_decode": (i32, [vp, ctypes.POINTER(i32), ctypes.POINTER(vp), i32, sz, vp]),
            "rs_decode_batch": (i32, [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32),
                                      ctypes.POINTER(vp), sz, ctypes.POINTER(vp), ctypes.POINTER(i32)]),
            "rs_encode_batch": (i32, [vp, i32, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), ctypes.POINTER(i32)]),
            "rs_encode_batch_lens": (i32, [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.POINTER(vp),
                                           ctypes.POINTER(i32)]),
            "rs_decode_batch_lens": (i32, [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(vp),
                                           ctypes.POINTER(sz), ctypes.POINTER(vp), ctypes.POINTER(i32)]),
            "rs_encode_stripes": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp]),
            "rs_reconstruct_stripes": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, vp]),
            "rs_reconstruct_ptrs": (i32, [vp, vp, sz, sz, vp, vp]),
            "rs_verify_ptrs": (i32, [vp, vp, sz, sz, vp, vp, vp]),
            "rs_encode_ptrs": (i32, [vp, vp, sz, sz, vp]),
            "rs_update_ptrs": (i32, [vp, vp, sz, sz, sz, ctypes.POINTER(ShardUpdate), sz, vp]),
            "rs_read_ptrs": (i32, [vp, vp, sz, sz, sz, vp, ctypes.POINTER(ShardRead), sz, vp]),
            "rs_correct_columns_ptrs": (i32, [vp, vp, sz, sz, vp, ctypes.POINTER(i32), vp, vp]),
            "rs_verify_stripes": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, vp]),
            "rs_correct_stripes": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, ctypes.POINTER(i32), vp, vp]),
            "rs_update_stripes": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, ctypes.POINTER(ShardUpdate), sz, vp]),
            "rs_update_degraded": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, ctypes.POINTER(ShardUpdate), sz, vp]),
            "rs_read_stripes": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, ctypes.POINTER(ShardRead), sz, vp]),
            "rs_verify_degraded": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, vp, vp]),
            "rs_correct_degraded": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, ctypes.POINTER(i32), vp, vp]),
            "rs_reconstruct_checked": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, vp, vp]),
            "rs_reconstruct_checked_ptrs": (i32, [vp, vp, sz, sz, vp, vp, vp]),
            "rs_verify_ptrs_lens": (i32, [vp, vp, ctypes.POINTER(sz), sz, vp, vp, vp]),
            "rs_reconstruct_checked_ptrs_lens": (i32, [vp, vp, ctypes.POINTER(sz), sz, vp, vp, vp]),
            "rs_correct_columns_ptrs_lens": (i32, [vp, vp, ctypes.POINTER(sz), sz, vp, ctypes.POINTER(i32), vp, vp]),
            "rs_correct_columns": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, ctypes.POINTER(i32), vp, vp]),
            "rs_crc32c_stripes": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, sz, vp, sz, vp]),
            "rs_crc32c_check_stripes": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, sz, vp, sz, vp, vp]),
            "rs_crc32c_ptrs": (i32, [vp, vp, sz, sz, vp, sz, vp, sz, vp]),
            "rs_crc32c_check_ptrs": (i32, [vp, vp, sz, sz, vp, sz, vp, sz, vp, vp]),
            "rs_correct_crc32c": (i32, [vp, vp, sz, vp, sz, sz, sz, sz, vp, sz, vp, sz, ctypes.POINTER(i32), vp, vp]),
            "rs_crc32c_host": (i32, [i32, ctypes.POINTER(vp), ctypes.POINTER(sz), vp]),
            "rs_combine": (i32, [vp, ctypes.POINTER(CombineJob), sz, sz, vp]),
            "rs_combine_lens": (i32, [vp, ctypes.POINTER(CombineJob), sz, ctypes.POINTER(sz), vp]),
            "rs_pattern_survivors": (i32, [vp, vp, ctypes.POINTER(i32)]),
            "rs_pattern_count": (i32, [vp]),
            "rs_pattern_evictions": (ctypes.c_int64, [vp]),
            "rs_prepare_patterns": (i32, [vp, i32, vp]),
            "rs_pattern_rows": (i32, [vp, vp, vp, ctypes.POINTER(i32)]),
            "rs_pinned_alloc": (vp, [sz]),
            "rs_pinned_free": (None, [vp]),
            "rs_device_alloc": (i32, [vp, sz, ctypes.POINTER(vp)]),
            "rs_device_free": (i32, [vp, vp]),
            "rs_stream_sync": (i32, [vp, vp]),
            "rs_fill_splitmix": (i32, [vp, vp, sz, ctypes.c_uint64, vp]),
            "rs_stat": (ctypes.c_int64, [vp, i32]),
            "rs_arena_new": (vp, [sz]),
            "rs_arena_alloc": (vp, [vp, sz]),
            "rs_arena_put": (vp, [vp, vp, sz]),
            "rs_arena_reset": (None, [vp]),
            "rs_arena_used": (sz, [vp]),
            "rs_arena_free": (None, [vp]),
            "rs_shard_unmarshal_arena": (i32, [vp, sz, vp, vp]),
            "rs_blake2b_batch": (i32, [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(sz), i32, vp]),
            "rs_blake2b_device": (i32, [vp, i32, vp, vp, vp, i32, vp, vp]),
            "rs_blake2b": (i32, [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(sz), i32, vp, ctypes.POINTER(i32)]),
            "rs_blake2b_host": (i32, [i32, ctypes.POINTER(vp), ctypes.POINTER(sz), i32, vp, i32]),
            "rs_new_devices": (i32, [i32, i32, ctypes.POINTER(i32), i32, ctypes.POINTER(vp)]),
            "rs_member_count": (i32, [vp]),
            "rs_member": (vp, [vp, i32]),
            "rs_partition": (i32, [sz, i32, i32, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
            "rs_encode_stripes_parts": (i32, [vp, ctypes.POINTER(StripePart), sz, sz]),
            "rs_reconstruct_stripes_parts": (i32, [vp, ctypes.POINTER(StripePart), sz, sz, vp]),
            "rs_reconstruct_spread": (i32, [vp, vp, vp, sz, sz, vp, vp]),
        }
        for name, (res, args) in sig.items():
            if os.environ.get("RSMI_LIB") and not hasattr(lib, name):
                continue  # an older build selected for an A/B run
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def load() -> ctypes.CDLL:
    """The loaded engine library (raises ImportError if it was not built)."""
    return _lib()


def _check(code: int, what: str) -> None:
    if code == RS_OK:
        return
    if code == RS_ENOT_ENOUGH:
        raise NotEnoughShares(code, what)
    raise RSError(code, what)


@dataclass
class Share:
    """infectious.Share{Number int; Data []byte} (main.go:57-69, :254-258)."""

    Number: int
    Data: bytes

    def DeepCopy(self) -> "Share":
        return Share(self.Number, bytes(self.Data))


def partition(units: int, parts: int, part: int):
    """rs_partition: (first, count) of part `part` of `units` split into
    `parts` contiguous ranges."""
    first, count = ctypes.c_size_t(), ctypes.c_size_t()
    _check(_lib().rs_partition(units, parts, part, ctypes.byref(first), ctypes.byref(count)), "rs_partition")
    return first.value, count.value


class FEC:
    """Handle of an rs_ctx: the engine-side infectious *FEC for (k, n).
    devices=[...] builds a device-set context (rs_new_devices): one member
    per listed GPU, every call spread over them."""

    def __init__(self, k: int, n: int, device: Optional[int] = None,
                 devices: Optional[Sequence[int]] = None, _handle=None):
        lib = _lib()
        self.k = k
        self.n = n
        self._owner = _handle is None
        if _handle is not None:  # a member of a device set: owned by the set
            self._h = ctypes.c_void_p(_handle)
            return
        h = ctypes.c_void_p()
        if devices is not None:
            devs = (ctypes.c_int * max(len(devices), 1))(*devices)
            code = lib.rs_new_devices(k, n, devs, len(devices), ctypes.byref(h))
        elif device is None:
            code = lib.rs_new(k, n, ctypes.byref(h))
        else:
            code = lib.rs_new_on_device(k, n, device, ctypes.byref(h))
        _check(code, f"NewFEC({k}, {n})")
        self._h = h

    # -- device sets (rs_new_devices) --------------------------------------------
    def member_count(self) -> int:
        return _lib().rs_member_count(self._h)

    def member(self, i: int) -> "FEC":
        """Member i (a single-device context owned by the set; self for i = 0
        of a single-device context)."""
        h = _lib().rs_member(self._h, i)
        if not h:
            raise RSError(RS_EINVAL, f"rs_member({i})")
        m = FEC(self.k, self.n, _handle=h)
        m._set = self  # keep the set alive while the member is used
        return m

    def encode_stripes_parts(self, parts: Sequence[tuple], pitch: int, shard_len: int) -> None:
        """rs_encode_stripes_parts: parts[i] = (data_ptr, data_stride,
        parity_ptr, parity_stride, stripes, stream) on member i's device."""
        arr = (StripePart * max(len(parts), 1))(*[StripePart(*p) for p in parts])
        _check(_lib().rs_encode_stripes_parts(self._h, arr, pitch, shard_len), "rs_encode_stripes_parts")

    def reconstruct_stripes_parts(self, parts: Sequence[tuple], pitch: int, shard_len: int,
                                  erased: bytes) -> None:
        arr = (StripePart * max(len(parts), 1))(*[StripePart(*p) for p in parts])
        buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_reconstruct_stripes_parts(self._h, arr, pitch, shard_len,
                                                   ctypes.cast(buf, ctypes.c_void_p)),
               "rs_reconstruct_stripes_parts")

    def reconstruct_spread(self, shard_ptrs: Sequence[int], owner: Sequence[int], shard_len: int,
                           stripes: int, erased: bytes, streams: Optional[Sequence[int]] = None) -> None:
        """rs_reconstruct_spread: shard i of stripe s at device address
        shard_ptrs[s * n + i] on any member's GPU; owner[s] reconstructs."""
        import numpy as np
        if len(erased) != stripes * self.n or len(shard_ptrs) != stripes * self.n or len(owner) != stripes:
            raise RSError(RS_EINVAL, "reconstruct_spread: table sizes")
        tab = np.ascontiguousarray(np.asarray(shard_ptrs, dtype=np.uint64))
        own = np.ascontiguousarray(np.asarray(owner, dtype=np.int32))
        buf = ctypes.c_char_p(bytes(erased))
        st = None
        if streams is not None:
            st = (ctypes.c_void_p * max(len(streams), 1))(*[x or None for x in streams])
        _check(_lib().rs_reconstruct_spread(self._h, tab.ctypes.data, own.ctypes.data, shard_len, stripes,
                                            ctypes.cast(buf, ctypes.c_void_p), st), "rs_reconstruct_spread")

    # -- infectious accessors -------------------------------------------------
    def Required(self) -> int:
        return self.k

    def Total(self) -> int:
        return self.n

    @property
    def handle(self) -> ctypes.c_void_p:
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None):
            if getattr(self, "_owner", True):
                _lib().rs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def kernel_name(self, which: int = 0) -> str:
        """Kernel serving encode (0), reconstruct (1), verify (2), update
        (3), degraded read (4), degraded check (5), combine (6), degraded
        update (7), column scrub (8) or combine_lens of mixed lengths (9);
        10 to 13 the pointer-mode check and column kernels and the repair
        kernels, 14 to 16 the per-stripe-length twins of verify, check and
        repair (verify_ptrs_lens, reconstruct_checked_ptrs_lens), 17 the
        per-job-length twin of the pointer-mode column kernel
        (correct_columns_ptrs_lens), 18 and 19 the sector-checksum kernel
        (crc32c_*) and its pointer-mode twin, 20 to 22 the kernels serving
        encode_ptrs, update_ptrs and read_ptrs: diagnostics."""
        return _lib().rs_kernel_name(self._h, which).decode()

    def matrix(self) -> bytes:
        buf = (ctypes.c_uint8 * (self.n * self.k))()
        _check(_lib().rs_encode_matrix(self._h, buf), "rs_encode_matrix")
        return bytes(buf)

    # -- (*FEC).Encode (main.go:262) ------------------------------------------
    def Encode(self, input: bytes, output: Callable[[Share], None]) -> None:
        """Calls output(Share) for shares 0..n-1 in order; like infectious,
        data shares are views of input and the parity buffer is reused
        between callbacks (callers DeepCopy, main.go:255-258)."""
        data = bytes(input)
        if len(data) % self.k != 0:
            raise RSError(RS_ELEN_NOT_MULTIPLE, "Encode")
        S = len(data) // self.k
        m = self.n - self.k
        parity = bytearray(m * S)
        if S and m:
            src = ctypes.c_char_p(data)
            dst = (ctypes.c_char * len(parity)).from_buffer(parity)
            _check(_lib().rs_encode(self._h, ctypes.cast(src, ctypes.c_void_p), len(data),
                                    ctypes.cast(dst, ctypes.c_void_p)), "Encode")
        view = memoryview(data)
        for i in range(self.k):
            output(Share(i, view[i * S:(i + 1) * S]))
        pv = memoryview(parity)
        for i in range(m):
            output(Share(self.k + i, pv[i * S:(i + 1) * S]))

    def encode_parity(self, input: bytes) -> bytes:
        """Parity shares k..n-1 concatenated (rs_encode)."""
        out: List[bytes] = []
        self.Encode(input, lambda s: out.append(bytes(s.Data)) if s.Number >= self.k else None)
        return b"".join(out)

    # -- (*FEC).Decode (main.go:77) -------------------------------------------
    def Decode(self, dst: Optional[bytearray], shares: List[Share]) -> bytes:
        """Returns the k*S-byte original.  Sorts `shares` in place by Number,
        as infectious does to the caller's slice."""
        cnt = len(shares)
        S = len(shares[0].Data) if cnt else 0
        for s in shares:
            if len(s.Data) != S:
                raise RSError(RS_ESHARE_LEN, "Decode")
        nums = (ctypes.c_int * max(cnt, 1))(*[s.Number for s in shares])
        keep = [bytes(s.Data) for s in shares]
        ptrs = (ctypes.c_void_p * max(cnt, 1))(
            *[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value for b in keep])
        out = bytearray(self.k * S)
        outp = (ctypes.c_char * max(len(out), 1)).from_buffer(out) if out else None
        code = _lib().rs_decode(self._h, nums, ptrs, cnt, S,
                                ctypes.cast(outp, ctypes.c_void_p) if outp is not None else None)
        _check(code, "Decode")
        # mirror the in-place sort
        order = sorted(range(cnt), key=lambda i: (shares[i].Number, i))
        shares[:] = [shares[i] for i in order]
        if dst is not None and len(dst) >= len(out):
            dst[:len(out)] = out
            return bytes(dst[:len(out)])
        return bytes(out)

    def DecodeBatch(self, messages: List[List[Share]]):
        """rs_decode_batch: decode many messages in one GPU pass.  Returns
        (outputs, statuses); outputs[b] is None where statuses[b] != 0."""
        B = len(messages)
        S = len(messages[0][0].Data) if B and messages[0] else 0
        counts = (ctypes.c_int * max(B, 1))(*[len(msg) for msg in messages])
        flat = [s for msg in messages for s in msg]
        for s in flat:
            if len(s.Data) != S:
                raise RSError(RS_ESHARE_LEN, "DecodeBatch")
        nums = (ctypes.c_int * max(len(flat), 1))(*[s.Number for s in flat])
        keep = [bytes(s.Data) for s in flat]
        ptrs = (ctypes.c_void_p * max(len(flat), 1))(
            *[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value for b in keep])
        outs = [bytearray(max(self.k * S, 1)) for _ in range(B)]
        outp = (ctypes.c_void_p * max(B, 1))(
            *[ctypes.addressof((ctypes.c_char * max(len(o), 1)).from_buffer(o)) for o in outs])
        st = (ctypes.c_int * max(B, 1))()
        _lib().rs_decode_batch(self._h, B, counts, nums, ptrs, S, outp, st)
        return ([bytes(o[:self.k * S]) if st[b] == RS_OK else None for b, o in enumerate(outs)],
                [st[b] for b in range(B)])

    def EncodeBatch(self, inputs: List[bytes]):
        """rs_encode_batch: the parity of many equal-length messages in one
        GPU pass (send-side batching).  Returns (parities, statuses);
        parities[b] is the m*S parity bytes (rs_encode's layout) or None where
        statuses[b] != 0."""
        B = len(inputs)
        L = len(inputs[0]) if B else 0
        for x in inputs:
            if len(x) != L:
                raise RSError(RS_EINVAL, "EncodeBatch: messages of unequal length")
        m = self.n - self.k
        P = (L // self.k) * m if L % self.k == 0 else 0
        keep = [bytes(x) for x in inputs]
        ins = (ctypes.c_void_p * max(B, 1))(
            *[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value for b in keep])
        outs = [bytearray(max(P, 1)) for _ in range(B)]
        outp = (ctypes.c_void_p * max(B, 1))(
            *[ctypes.addressof((ctypes.c_char * len(o)).from_buffer(o)) for o in outs])
        st = (ctypes.c_int * max(B, 1))()
        _lib().rs_encode_batch(self._h, B, ins, L, outp, st)
        return ([bytes(o[:P]) if st[b] == RS_OK else None for b, o in enumerate(outs)],
                [st[b] for b in range(B)])

    def EncodeBatchLens(self, inputs: List[bytes]):
        """rs_encode_batch_lens: EncodeBatch for messages of any lengths, in
        one call.  Returns (parities, statuses); a message whose length is no
        multiple of k fails alone."""
        B = len(inputs)
        m = self.n - self.k
        P = [(len(x) // self.k) * m if len(x) % self.k == 0 else 0 for x in inputs]
        keep = [bytes(x) for x in inputs]
        ins = (ctypes.c_void_p * max(B, 1))(
            *[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value for b in keep])
        lens = (ctypes.c_size_t * max(B, 1))(*[len(x) for x in keep])
        outs = [bytearray(max(p, 1)) for p in P]
        outp = (ctypes.c_void_p * max(B, 1))(
            *[ctypes.addressof((ctypes.c_char * len(o)).from_buffer(o)) for o in outs])
        st = (ctypes.c_int * max(B, 1))()
        _lib().rs_encode_batch_lens(self._h, B, ins, lens, outp, st)
        return ([bytes(o[:P[b]]) if st[b] == RS_OK else None for b, o in enumerate(outs)],
                [st[b] for b in range(B)])

    def DecodeBatchLens(self, messages: List[List[Share]]):
        """rs_decode_batch_lens: DecodeBatch for messages of different share
        lengths, in one call; the shares of one message must still agree.
        Sorts each message's list in place by Number, as Decode does.  Returns
        (outputs, statuses); outputs[b] is None where statuses[b] != 0."""
        B = len(messages)
        S = [len(msg[0].Data) if msg else 0 for msg in messages]
        for msg, length in zip(messages, S):
            for s in msg:
                if len(s.Data) != length:
                    raise RSError(RS_ESHARE_LEN, "DecodeBatchLens")
        counts = (ctypes.c_int * max(B, 1))(*[len(msg) for msg in messages])
        flat = [s for msg in messages for s in msg]
        nums = (ctypes.c_int * max(len(flat), 1))(*[s.Number for s in flat])
        keep = [bytes(s.Data) for s in flat]
        ptrs = (ctypes.c_void_p * max(len(flat), 1))(
            *[ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value for b in keep])
        lens = (ctypes.c_size_t * max(B, 1))(*S)
        outs = [bytearray(max(self.k * length, 1)) for length in S]
        outp = (ctypes.c_void_p * max(B, 1))(
            *[ctypes.addressof((ctypes.c_char * max(len(o), 1)).from_buffer(o)) for o in outs])
        st = (ctypes.c_int * max(B, 1))()
        _lib().rs_decode_batch_lens(self._h, B, counts, nums, ptrs, lens, outp, st)
        for msg in messages:  # mirror the in-place sort
            msg.sort(key=lambda s: s.Number)
        return ([bytes(o[:self.k * S[b]]) if st[b] == RS_OK else None for b, o in enumerate(outs)],
                [st[b] for b in range(B)])

    # -- device-resident batched API -------------------------------------------
    def encode_stripes(self, data_ptr: int, data_stride: int, parity_ptr: int,
                       parity_stride: int, pitch: int, shard_len: int, stripes: int,
                       stream: int = 0) -> None:
        _check(_lib().rs_encode_stripes(self._h, data_ptr, data_stride, parity_ptr,
                                        parity_stride, pitch, shard_len, stripes,
                                        stream or None), "rs_encode_stripes")

    def reconstruct_stripes(self, data_ptr: int, data_stride: int, parity_ptr: int,
                            parity_stride: int, pitch: int, shard_len: int, stripes: int,
                            erased: bytes, stream: int = 0) -> None:
        if len(erased) != stripes * self.n:
            raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
        buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_reconstruct_stripes(self._h, data_ptr, data_stride, parity_ptr,
                                             parity_stride, pitch, shard_len, stripes,
                                             ctypes.cast(buf, ctypes.c_void_p), stream or None),
               "rs_reconstruct_stripes")

    def verify_stripes(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                       pitch: int, shard_len: int, stripes: int, first_bad_ptr: int,
                       stream: int = 0) -> None:
        """rs_verify_stripes: first_bad_ptr is a device array of `stripes`
        uint32; entry s receives the lowest byte offset at which stripe s's
        stored parity differs from the recomputed one, or RS_VERIFY_CLEAN.
        Enqueued on stream."""
        _check(_lib().rs_verify_stripes(self._h, data_ptr, data_stride, parity_ptr, parity_stride,
                                        pitch, shard_len, stripes, first_bad_ptr or None,
                                        stream or None), "rs_verify_stripes")

    def correct_stripes(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                        pitch: int, shard_len: int, stripes: int, stream: int = 0):
        """rs_correct_stripes (scrub): (status, rewritten) -- status[s] is
        RS_OK or RS_ETOO_MANY_ERRORS, rewritten[s * n + i] is non-zero where
        shard i of stripe s was regenerated.  Raises only for argument,
        device or memory errors."""
        st = (ctypes.c_int * max(stripes, 1))()
        rw = ctypes.create_string_buffer(max(stripes * self.n, 1))
        rc = _lib().rs_correct_stripes(self._h, data_ptr, data_stride, parity_ptr, parity_stride,
                                       pitch, shard_len, stripes, st,
                                       ctypes.cast(rw, ctypes.c_void_p), stream or None)
        if rc != RS_ETOO_MANY_ERRORS:
            _check(rc, "rs_correct_stripes")
        return [st[s] for s in range(stripes)], rw.raw[:stripes * self.n]

    def verify_degraded(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                        pitch: int, shard_len: int, stripes: int, erased: bytes, first_bad_ptr: int,
                        stream: int = 0) -> None:
        """rs_verify_degraded: verify_stripes for stripes with missing shards
        (erased: stripes * n flags).  first_bad_ptr[s] receives the lowest
        byte offset at which the present shards of stripe s do not lie on one
        codeword, or RS_VERIFY_CLEAN; erased slots are never dereferenced.
        Enqueued on stream."""
        if len(erased) != stripes * self.n:
            raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
        buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_verify_degraded(self._h, data_ptr, data_stride, parity_ptr, parity_stride,
                                         pitch, shard_len, stripes, ctypes.cast(buf, ctypes.c_void_p),
                                         first_bad_ptr or None, stream or None), "rs_verify_degraded")

    def reconstruct_checked(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                            pitch: int, shard_len: int, stripes: int, erased: bytes, first_bad_ptr: int,
                            stream: int = 0) -> None:
        """rs_reconstruct_checked: reconstruct_stripes and verify_degraded in
        one pass (erased: stripes * n flags).  The erased slots are filled in
        and first_bad_ptr[s] receives verify_degraded's verdict on the stripes
        as they were before the call: a stripe that is not RS_VERIFY_CLEAN was
        repaired from survivors that cannot be trusted.  Enqueued on stream."""
        if len(erased) != stripes * self.n:
            raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
        buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_reconstruct_checked(self._h, data_ptr, data_stride, parity_ptr, parity_stride,
                                             pitch, shard_len, stripes, ctypes.cast(buf, ctypes.c_void_p),
                                             first_bad_ptr or None, stream or None), "rs_reconstruct_checked")

    def correct_degraded(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                         pitch: int, shard_len: int, stripes: int, erased: bytes, stream: int = 0):
        """rs_correct_degraded (scrub with missing shards): (status,
        rewritten) as correct_stripes; located shards are regenerated in
        place, erased ones are neither touched nor filled in.  Raises only
        for argument, device or memory errors and for more than m erasures."""
        if len(erased) != stripes * self.n:
            raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
        buf = ctypes.c_char_p(bytes(erased))
        st = (ctypes.c_int * max(stripes, 1))()
        rw = ctypes.create_string_buffer(max(stripes * self.n, 1))
        rc = _lib().rs_correct_degraded(self._h, data_ptr, data_stride, parity_ptr, parity_stride,
                                        pitch, shard_len, stripes, ctypes.cast(buf, ctypes.c_void_p), st,
                                        ctypes.cast(rw, ctypes.c_void_p), stream or None)
        if rc != RS_ETOO_MANY_ERRORS:
            _check(rc, "rs_correct_degraded")
        return [st[s] for s in range(stripes)], rw.raw[:stripes * self.n]

    # -- sector checksums (CRC-32C of stored shards) -----------------------------
    def _flags(self, erased: Optional[bytes], stripes: int):
        if erased is None:
            return None
        if len(erased) != stripes * self.n:
            raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
        return ctypes.c_char_p(bytes(erased))

    def crc32c_stripes(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                       pitch: int, shard_len: int, stripes: int, sector_len: int, crcs_ptr: int,
                       crc_pitch: int, erased: Optional[bytes] = None, stream: int = 0) -> None:
        """rs_crc32c_stripes: the CRC-32C of sector j of shard i of stripe s
        goes to the device uint32 array crcs_ptr[(s * n + i) * crc_pitch + j];
        a sector covers sector_len bytes, the last one what is left below
        shard_len.  Entries of erased shards (erased: stripes * n flags, or
        None) are left as they are.  Enqueued on stream."""
        buf = self._flags(erased, stripes)
        _check(_lib().rs_crc32c_stripes(self._h, data_ptr, data_stride, parity_ptr, parity_stride, pitch,
                                        shard_len, stripes, ctypes.cast(buf, ctypes.c_void_p), sector_len,
                                        crcs_ptr or None, crc_pitch, stream or None), "rs_crc32c_stripes")

    def crc32c_check_stripes(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                             pitch: int, shard_len: int, stripes: int, sector_len: int, crcs_ptr: int,
                             crc_pitch: int, first_bad_ptr: int, erased: Optional[bytes] = None,
                             stream: int = 0) -> None:
        """rs_crc32c_check_stripes: first_bad_ptr is a device array of
        stripes * n uint32; entry s * n + i receives the lowest sector of
        shard i of stripe s that does not match its stored checksum, or
        RS_VERIFY_CLEAN (also for erased shards).  Enqueued on stream."""
        buf = self._flags(erased, stripes)
        _check(_lib().rs_crc32c_check_stripes(self._h, data_ptr, data_stride, parity_ptr, parity_stride, pitch,
                                              shard_len, stripes, ctypes.cast(buf, ctypes.c_void_p), sector_len,
                                              crcs_ptr or None, crc_pitch, first_bad_ptr or None, stream or None),
               "rs_crc32c_check_stripes")

    def crc32c_ptrs(self, shard_ptrs_dev: int, shard_len: int, stripes: int, sector_len: int, crcs_ptr: int,
                    crc_pitch: int, erased: Optional[bytes] = None, stream: int = 0) -> None:
        """rs_crc32c_ptrs: crc32c_stripes for shards at the device addresses
        in the device array shard_ptrs_dev[s * n + i]; entries of erased
        shards are not loaded.  Enqueued on stream."""
        buf = self._flags(erased, stripes)
        _check(_lib().rs_crc32c_ptrs(self._h, shard_ptrs_dev or None, shard_len, stripes,
                                     ctypes.cast(buf, ctypes.c_void_p), sector_len, crcs_ptr or None, crc_pitch,
                                     stream or None), "rs_crc32c_ptrs")

    def crc32c_check_ptrs(self, shard_ptrs_dev: int, shard_len: int, stripes: int, sector_len: int, crcs_ptr: int,
                          crc_pitch: int, first_bad_ptr: int, erased: Optional[bytes] = None,
                          stream: int = 0) -> None:
        """rs_crc32c_check_ptrs: crc32c_check_stripes on the pointer
        placement.  Enqueued on stream."""
        buf = self._flags(erased, stripes)
        _check(_lib().rs_crc32c_check_ptrs(self._h, shard_ptrs_dev or None, shard_len, stripes,
                                           ctypes.cast(buf, ctypes.c_void_p), sector_len, crcs_ptr or None,
                                           crc_pitch, first_bad_ptr or None, stream or None),
               "rs_crc32c_check_ptrs")

    def correct_crc32c(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                       pitch: int, shard_len: int, stripes: int, sector_len: int, crcs_ptr: int,
                       crc_pitch: int, erased: Optional[bytes] = None, stream: int = 0):
        """rs_correct_crc32c (repair by checksum): (status, rewritten) as
        correct_degraded.  Every present shard with a sector that does not
        match its stored checksum is regenerated in place, up to m of them
        per stripe together with the erased ones, and checked again; the
        checksums themselves are never written.  Raises only for argument,
        device or memory errors and for a damaged stripe with more than m
        erasures."""
        buf = self._flags(erased, stripes)
        st = (ctypes.c_int * max(stripes, 1))()
        rw = ctypes.create_string_buffer(max(stripes * self.n, 1))
        rc = _lib().rs_correct_crc32c(self._h, data_ptr, data_stride, parity_ptr, parity_stride, pitch,
                                      shard_len, stripes, ctypes.cast(buf, ctypes.c_void_p), sector_len,
                                      crcs_ptr or None, crc_pitch, st, ctypes.cast(rw, ctypes.c_void_p),
                                      stream or None)
        if rc != RS_ETOO_MANY_ERRORS:
            _check(rc, "rs_correct_crc32c")
        return [st[s] for s in range(stripes)], rw.raw[:stripes * self.n]

    def correct_columns(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                        pitch: int, shard_len: int, stripes: int, erased: Optional[bytes] = None,
                        stream: int = 0):
        """rs_correct_columns (column scrub): every byte column of every
        stripe decoded on its own, so a stripe is repaired whenever each
        column has at most (r - k) // 2 wrong shares among its r present
        ones.  Returns (status, corrected): status[s] is RS_OK or
        RS_ETOO_MANY_ERRORS, corrected[s * n + i] the bytes of shard i of
        stripe s the call changed.  erased: stripes * n flags, or None.
        Raises only for argument, device or memory errors and for more than
        m erasures."""
        buf = None
        if erased is not None:
            if len(erased) != stripes * self.n:
                raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
            buf = ctypes.c_char_p(bytes(erased))
        st = (ctypes.c_int * max(stripes, 1))()
        cnt = (ctypes.c_uint32 * max(stripes * self.n, 1))()
        rc = _lib().rs_correct_columns(self._h, data_ptr, data_stride, parity_ptr, parity_stride,
                                       pitch, shard_len, stripes, ctypes.cast(buf, ctypes.c_void_p), st,
                                       ctypes.cast(cnt, ctypes.c_void_p), stream or None)
        if rc != RS_ETOO_MANY_ERRORS:
            _check(rc, "rs_correct_columns")
        return [st[s] for s in range(stripes)], [cnt[x] for x in range(stripes * self.n)]

    def update_stripes(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                       pitch: int, shard_len: int, stripes: int, updates: Sequence[tuple],
                       stream: int = 0) -> None:
        """rs_update_stripes: updates is a sequence of (stripe, shard,
        src_ptr); data shard `shard` of stripe `stripe` takes the contents at
        the device address src_ptr and the stripe's stored parity is patched
        in place from old ^ new.  A caller that repeats a large list passes
        the table shard_updates() built from it instead.  Enqueued on stream."""
        arr = updates if isinstance(updates, ctypes.Array) else shard_updates(updates)
        _check(_lib().rs_update_stripes(self._h, data_ptr, data_stride, parity_ptr or None, parity_stride,
                                        pitch, shard_len, stripes, arr, len(updates), stream or None),
               "rs_update_stripes")

    def update_degraded(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                        pitch: int, shard_len: int, stripes: int, erased: bytes, updates: Sequence[tuple],
                        stream: int = 0) -> None:
        """rs_update_degraded: update_stripes for stripes with missing shards
        (erased: stripes * n flags).  Present parity shards are patched in
        place; a present changed shard takes its new contents; an erased one
        is left alone -- its old contents are regenerated from the stripe's
        survivors for the patch and its new ones live in the parity until
        reconstruct_stripes with the same flags produces them.  Erased slots
        are never dereferenced.  Enqueued on stream."""
        if len(erased) != stripes * self.n:
            raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
        arr = updates if isinstance(updates, ctypes.Array) else shard_updates(updates)
        buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_update_degraded(self._h, data_ptr, data_stride, parity_ptr or None, parity_stride,
                                         pitch, shard_len, stripes, ctypes.cast(buf, ctypes.c_void_p), arr,
                                         len(updates), stream or None), "rs_update_degraded")

    def read_stripes(self, data_ptr: int, data_stride: int, parity_ptr: int, parity_stride: int,
                     pitch: int, shard_len: int, stripes: int, erased: bytes, reads: Sequence[tuple],
                     stream: int = 0) -> None:
        """rs_read_stripes (degraded read): reads is a sequence of (stripe,
        shard, dst_ptr); the device address dst_ptr receives shard `shard` of
        stripe `stripe` -- copied if erased (stripes * n flags) says it is
        present, else computed from the stripe's survivors.  The stripes are
        only read.  A caller that repeats a large list passes the table
        shard_reads() built from it instead.  Enqueued on stream."""
        if len(erased) != stripes * self.n:
            raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
        arr = reads if isinstance(reads, ctypes.Array) else shard_reads(reads)
        buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_read_stripes(self._h, data_ptr, data_stride, parity_ptr or None, parity_stride,
                                      pitch, shard_len, stripes, ctypes.cast(buf, ctypes.c_void_p), arr,
                                      len(reads), stream or None), "rs_read_stripes")

    def combine(self, jobs: Sequence[tuple], length: int, stream: int = 0) -> None:
        """rs_combine: jobs is a sequence of (src_ptrs, dst_ptrs, coef,
        accumulate); every job multiplies its source buffers (device
        addresses, `length` bytes each) by its nout x nsrc coefficient bytes
        and stores the nout sums at dst_ptrs, or XORs them in when accumulate
        is set.  A caller that repeats a large list passes the table
        combine_jobs() built from it instead.  Enqueued on stream."""
        arr = jobs if isinstance(jobs, ctypes.Array) else combine_jobs(jobs)
        _check(_lib().rs_combine(self._h, arr, arr._count, length, stream or None), "rs_combine")

    def combine_lens(self, jobs: Sequence[tuple], lengths: Sequence[int], stream: int = 0) -> None:
        """rs_combine_lens: combine() with job b over buffers of lengths[b]
        bytes; a job of length 0 does nothing.  A caller that repeats a large
        list passes a ctypes c_size_t array of the lengths, as it passes the
        table of combine_jobs().  Enqueued on stream."""
        arr = jobs if isinstance(jobs, ctypes.Array) else combine_jobs(jobs)
        if len(lengths) != arr._count:
            raise RSError(RS_EINVAL, "lengths must hold one length per job")
        lens = lengths if isinstance(lengths, ctypes.Array) else (ctypes.c_size_t * max(len(lengths), 1))(*lengths)
        _check(_lib().rs_combine_lens(self._h, arr, arr._count, lens, stream or None), "rs_combine_lens")

    def pattern_survivors(self, erased: bytes) -> List[int]:
        """The shard id behind each of the k columns of pattern_rows(erased)."""
        if len(erased) != self.n:
            raise RSError(RS_EINVAL, "erased must hold n flags")
        ids = (ctypes.c_int * self.k)()
        flags = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_pattern_survivors(self._h, ctypes.cast(flags, ctypes.c_void_p), ids),
               "rs_pattern_survivors")
        return list(ids)

    def reconstruct_ptrs(self, shard_ptrs_dev: int, shard_len: int, stripes: int, erased: bytes,
                         stream: int = 0) -> None:
        """rs_reconstruct_ptrs: shard i of stripe s at the device address in
        the device array shard_ptrs_dev[s * n + i].  Every address must be
        16-byte aligned (the kernels move 16-byte vectors; rsmi.h), e.g. rows
        of a pool whose row pitch is a multiple of 16."""
        if len(erased) != stripes * self.n:
            raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
        buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_reconstruct_ptrs(self._h, shard_ptrs_dev, shard_len, stripes,
                                          ctypes.cast(buf, ctypes.c_void_p), stream or None),
               "rs_reconstruct_ptrs")

    def verify_ptrs(self, shard_ptrs_dev: int, shard_len: int, stripes: int, first_bad_ptr: int,
                    erased: Optional[bytes] = None, stream: int = 0) -> None:
        """rs_verify_ptrs: verify_degraded (verify_stripes without flags) for
        shards at the device addresses in the device array
        shard_ptrs_dev[s * n + i], as reconstruct_ptrs.  Entries of erased
        shards are never dereferenced.  Enqueued on stream."""
        buf = None
        if erased is not None:
            if len(erased) != stripes * self.n:
                raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
            buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_verify_ptrs(self._h, shard_ptrs_dev or None, shard_len, stripes,
                                     ctypes.cast(buf, ctypes.c_void_p), first_bad_ptr or None, stream or None),
               "rs_verify_ptrs")

    def encode_ptrs(self, shard_ptrs_dev: int, shard_len: int, stripes: int, stream: int = 0) -> None:
        """rs_encode_ptrs: encode_stripes for shards at the device addresses
        in the device array shard_ptrs_dev[s * n + i], as reconstruct_ptrs:
        the m parity slots of every stripe are written from its k data slots.
        Enqueued on stream."""
        _check(_lib().rs_encode_ptrs(self._h, shard_ptrs_dev or None, shard_len, stripes, stream or None),
               "rs_encode_ptrs")

    def update_ptrs(self, shard_ptrs_dev: int, shard_len: int, stripes: int, updates: Sequence[tuple],
                    offset: int = 0, stream: int = 0) -> None:
        """rs_update_ptrs: update_stripes for shards at the device addresses
        in shard_ptrs_dev[s * n + i].  updates as there; bytes [offset,
        offset + shard_len) of the changed shards' slots take the contents at
        src_ptr and the same bytes of the stripe's parity slots are patched.
        Only the table entries of the changed shards and of the parity of
        listed stripes are dereferenced.  Enqueued on stream."""
        arr = updates if isinstance(updates, ctypes.Array) else shard_updates(updates)
        _check(_lib().rs_update_ptrs(self._h, shard_ptrs_dev or None, offset, shard_len, stripes, arr,
                                     len(updates), stream or None), "rs_update_ptrs")

    def read_ptrs(self, shard_ptrs_dev: int, shard_len: int, stripes: int, erased: Optional[bytes],
                  reads: Sequence[tuple], offset: int = 0, stream: int = 0) -> None:
        """rs_read_ptrs: read_stripes for shards at the device addresses in
        shard_ptrs_dev[s * n + i].  reads as there; dst_ptr receives bytes
        [offset, offset + shard_len) of the shard, copied or computed from the
        stripe's survivors.  Nothing the table names is written and entries of
        erased shards are never dereferenced.  erased None is passed on as
        NULL, which the call refuses.  Enqueued on stream."""
        buf = None
        if erased is not None:
            if len(erased) != stripes * self.n:
                raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
            buf = ctypes.c_char_p(bytes(erased))
        arr = reads if isinstance(reads, ctypes.Array) else shard_reads(reads)
        _check(_lib().rs_read_ptrs(self._h, shard_ptrs_dev or None, offset, shard_len, stripes,
                                   ctypes.cast(buf, ctypes.c_void_p), arr, len(reads), stream or None),
               "rs_read_ptrs")

    def reconstruct_checked_ptrs(self, shard_ptrs_dev: int, shard_len: int, stripes: int, erased: bytes,
                                 first_bad_ptr: int, stream: int = 0) -> None:
        """rs_reconstruct_checked_ptrs: reconstruct_checked for shards at the
        device addresses in shard_ptrs_dev[s * n + i].  The entries of erased
        shards are the destinations: valid, and disjoint from every present
        shard.  Enqueued on stream."""
        if len(erased) != stripes * self.n:
            raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
        buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_reconstruct_checked_ptrs(self._h, shard_ptrs_dev or None, shard_len, stripes,
                                                  ctypes.cast(buf, ctypes.c_void_p), first_bad_ptr or None,
                                                  stream or None), "rs_reconstruct_checked_ptrs")

    def _stripe_lens(self, shard_lens: Sequence[int], stripes: int):
        if len(shard_lens) != stripes:
            raise RSError(RS_EINVAL, "shard_lens must hold one length per stripe")
        if isinstance(shard_lens, ctypes.Array):
            return shard_lens
        return (ctypes.c_size_t * max(stripes, 1))(*shard_lens)

    def verify_ptrs_lens(self, shard_ptrs_dev: int, shard_lens: Sequence[int], stripes: int, first_bad_ptr: int,
                         erased: Optional[bytes] = None, stream: int = 0) -> None:
        """rs_verify_ptrs_lens: verify_ptrs where stripe s has shard_lens[s]
        bytes per shard (a sequence, or a ctypes c_size_t array for a caller
        that repeats a large one).  Bytes past a stripe's length are neither
        read past its last 16-byte column nor compared; a stripe of length 0
        is clean.  Enqueued on stream."""
        lens = self._stripe_lens(shard_lens, stripes)
        buf = None
        if erased is not None:
            if len(erased) != stripes * self.n:
                raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
            buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_verify_ptrs_lens(self._h, shard_ptrs_dev or None, lens, stripes,
                                          ctypes.cast(buf, ctypes.c_void_p), first_bad_ptr or None, stream or None),
               "rs_verify_ptrs_lens")

    def reconstruct_checked_ptrs_lens(self, shard_ptrs_dev: int, shard_lens: Sequence[int], stripes: int,
                                      erased: bytes, first_bad_ptr: int, stream: int = 0) -> None:
        """rs_reconstruct_checked_ptrs_lens: reconstruct_checked_ptrs where
        stripe s has shard_lens[s] bytes per shard, as verify_ptrs_lens.  The
        slot of an erased shard of stripe s receives round_up(shard_lens[s],
        16) bytes.  Enqueued on stream."""
        lens = self._stripe_lens(shard_lens, stripes)
        if len(erased) != stripes * self.n:
            raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
        buf = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_reconstruct_checked_ptrs_lens(self._h, shard_ptrs_dev or None, lens, stripes,
                                                       ctypes.cast(buf, ctypes.c_void_p), first_bad_ptr or None,
                                                       stream or None), "rs_reconstruct_checked_ptrs_lens")

    def correct_columns_ptrs(self, shard_ptrs_dev: int, shard_len: int, stripes: int,
                             erased: Optional[bytes] = None, stream: int = 0):
        """rs_correct_columns_ptrs: correct_columns for shards at the device
        addresses in shard_ptrs_dev[s * n + i].  Returns (status, corrected):
        the status list as correct_columns, corrected a uint32 ndarray of
        stripes * n counts.  The ranges of the present shards must not
        overlap.  Raises only for argument, device or memory errors and for
        more than m erasures."""
        import numpy as np
        buf = None
        if erased is not None:
            if len(erased) != stripes * self.n:
                raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
            buf = ctypes.c_char_p(bytes(erased))
        st = (ctypes.c_int * max(stripes, 1))()
        cnt = np.zeros(max(stripes * self.n, 1), dtype=np.uint32)
        rc = _lib().rs_correct_columns_ptrs(self._h, shard_ptrs_dev or None, shard_len, stripes,
                                            ctypes.cast(buf, ctypes.c_void_p), st,
                                            ctypes.c_void_p(cnt.ctypes.data), stream or None)
        if rc != RS_ETOO_MANY_ERRORS:
            _check(rc, "rs_correct_columns_ptrs")
        return [st[s] for s in range(stripes)], cnt[:stripes * self.n]

    def correct_columns_ptrs_lens(self, shard_ptrs_dev: int, shard_lens: Sequence[int], stripes: int,
                                  erased: Optional[bytes] = None, stream: int = 0):
        """rs_correct_columns_ptrs_lens: correct_columns_ptrs where stripe s
        has shard_lens[s] bytes per shard (as verify_ptrs_lens takes them).
        Bytes at or beyond a stripe's length are neither decoded nor written;
        a stripe of length 0 ends RS_OK with zero counts.  Returns (status,
        corrected) as correct_columns_ptrs; raises only for argument, device
        or memory errors and for more than m erasures."""
        import numpy as np
        lens = self._stripe_lens(shard_lens, stripes)
        buf = None
        if erased is not None:
            if len(erased) != stripes * self.n:
                raise RSError(RS_EINVAL, "erased must hold stripes*n flags")
            buf = ctypes.c_char_p(bytes(erased))
        st = (ctypes.c_int * max(stripes, 1))()
        cnt = np.zeros(max(stripes * self.n, 1), dtype=np.uint32)
        rc = _lib().rs_correct_columns_ptrs_lens(self._h, shard_ptrs_dev or None, lens, stripes,
                                                 ctypes.cast(buf, ctypes.c_void_p), st,
                                                 ctypes.c_void_p(cnt.ctypes.data), stream or None)
        if rc != RS_ETOO_MANY_ERRORS:
            _check(rc, "rs_correct_columns_ptrs_lens")
        return [st[s] for s in range(stripes)], cnt[:stripes * self.n]

    def pattern_count(self) -> int:
        return _lib().rs_pattern_count(self._h)

    (STAT_PATTERNS, STAT_EVICTIONS, STAT_BATCHES_IN_PLACE, STAT_BATCHES_STAGED, STAT_LEASES,
     STAT_ENCODES_IN_PLACE, STAT_DECODES_IN_PLACE, STAT_REC_STRIPES_TABLE, STAT_REC_STRIPES_SYNDROME,
     STAT_ENCODE_BATCHES, STAT_MAILBOX_CALLS, STAT_MAILBOX_RECOVERED, STAT_UPDATE_STRIPES,
     STAT_UPDATE_COPY_COMMITS, STAT_READ_REGENERATED, STAT_READ_COPIED, STAT_CHECK_STRIPES,
     STAT_SCRUB_REGENERATED, STAT_COMBINE_JOBS, STAT_COMBINE_ROWS, STAT_UPDATE_DEGRADED,
     STAT_UPDATE_ABSORBED, STAT_COLUMN_STRIPES, STAT_COLUMN_BYTES, STAT_BATCH_LENS_PASSES,
     STAT_COMBINE_LENS_LAUNCHES, STAT_REPAIR_CHECKED, STAT_SCRUB_LENS_LAUNCHES,
     STAT_COLUMN_LENS_LAUNCHES, STAT_CRC_SECTORS, STAT_CRC_REGENERATED) = range(31)

    def stat(self, which: int) -> int:
        return _lib().rs_stat(self._h, which)

    def pattern_evictions(self) -> int:
        return _lib().rs_pattern_evictions(self._h)

    def pattern_rows(self, erased: bytes):
        """(rows bytes m*k, count) the engine uses for this erasure pattern."""
        m = self.n - self.k
        buf = (ctypes.c_uint8 * max(m * self.k, 1))()
        cnt = ctypes.c_int()
        flags = ctypes.c_char_p(bytes(erased))
        _check(_lib().rs_pattern_rows(self._h, ctypes.cast(flags, ctypes.c_void_p),
                                      ctypes.cast(buf, ctypes.c_void_p), ctypes.byref(cnt)),
               "rs_pattern_rows")
        return bytes(buf)[:m * self.k], cnt.value

    def prepare_patterns(self, max_erasures: int, stream: int = 0) -> None:
        _check(_lib().rs_prepare_patterns(self._h, max_erasures, stream or None),
               "rs_prepare_patterns")

    def fill_splitmix(self, dev_ptr: int, nbytes: int, seed: int, stream: int = 0) -> None:
        _check(_lib().rs_fill_splitmix(self._h, dev_ptr, nbytes, seed & (2**64 - 1),
                                       stream or None), "rs_fill_splitmix")

    # -- signature hashing (blake2b policy, main.go:38-41, :219-223, :82-89) ----
    def blake2b_batch(self, messages: Sequence[bytes], digest_len: int = 32) -> List[bytes]:
        """BLAKE2b digests of many host messages in one GPU launch."""
        if not messages:
            return []
        keep, ptrs, lens = _message_table(messages)
        out = ctypes.create_string_buffer(len(messages) * digest_len)
        _check(_lib().rs_blake2b_batch(self._h, len(messages), ptrs, lens, digest_len,
                                       ctypes.cast(out, ctypes.c_void_p)), "rs_blake2b_batch")
        return _split(out.raw, len(messages), digest_len)

    def blake2b(self, messages: Sequence[bytes], digest_len: int = 32):
        """The hash policy (rs_blake2b): host CPU for one message or a batch
        whose longest chain dominates, the GPU kernel otherwise.  Returns
        (digests, where) with where 0 = host, 1 = GPU."""
        if not messages:
            return [], 0
        keep, ptrs, lens = _message_table(messages)
        out = ctypes.create_string_buffer(len(messages) * digest_len)
        where = ctypes.c_int(0)
        _check(_lib().rs_blake2b(self._h, len(messages), ptrs, lens, digest_len,
                                 ctypes.cast(out, ctypes.c_void_p), ctypes.byref(where)), "rs_blake2b")
        return _split(out.raw, len(messages), digest_len), where.value

    def blake2b_device(self, count: int, ptrs_dev: int, lens_dev: int, order_dev: int,
                       digest_len: int, out_dev: int, stream: int = 0) -> None:
        _check(_lib().rs_blake2b_device(self._h, count, ptrs_dev, lens_dev, order_dev or None,
                                        digest_len, out_dev, stream or None), "rs_blake2b_device")

    def sync(self, stream: int = 0) -> None:
        _check(_lib().rs_stream_sync(self._h, stream or None), "rs_stream_sync")


class Arena:
    """rs_arena: engine-pinned receive memory.  Shard bytes placed here (put,
    or the wire codec's rs_shard_unmarshal_arena) are read in place over
    PCIe by rs_decode_batch's kernel."""

    def __init__(self, nbytes: int):
        self._a = _lib().rs_arena_new(nbytes)
        if not self._a:
            raise RSError(RS_ENOMEM, "rs_arena_new")

    def put(self, data: bytes) -> int:
        """Copies data into a fresh 16-byte aligned slot (rs_arena_put:
        streaming stores, as rs_shard_unmarshal_arena); returns its address."""
        buf = bytes(data)
        p = _lib().rs_arena_put(self._a, buf, len(buf))
        if not p:
            raise RSError(RS_ENOMEM, "rs_arena_put")
        return p

    def used(self) -> int:
        return _lib().rs_arena_used(self._a)

    def reset(self) -> None:
        _lib().rs_arena_reset(self._a)

    def free(self) -> None:
        if getattr(self, "_a", None):
            _lib().rs_arena_free(self._a)
            self._a = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _message_table(messages: Sequence[bytes]):
    """(keep-alive, pointer array, length array) of host messages for the
    hash entry points: one pointer per message when there are few or large
    ones (no Python-side copy), pointers into one joined buffer otherwise."""
    import numpy as np
    cnt = len(messages)
    lens_np = np.fromiter((len(mm) for mm in messages), dtype=np.uint64, count=cnt)
    if cnt <= 1024 or int(lens_np.sum()) > (64 << 20):
        keep = [bytes(mm) for mm in messages]
        ptr_np = np.fromiter((ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value or 0 for b in keep),
                             dtype=np.uint64, count=cnt)
    else:
        keep = b"".join(bytes(mm) for mm in messages)
        base = ctypes.cast(ctypes.c_char_p(keep), ctypes.c_void_p).value or 0
        offs = np.zeros(cnt, dtype=np.uint64)
        np.cumsum(lens_np[:-1], out=offs[1:])
        ptr_np = (offs + np.uint64(base)).astype(np.uint64)
    keep = (keep, ptr_np, lens_np)
    return (keep, ptr_np.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)),
            lens_np.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)))


def _split(raw: bytes, cnt: int, digest_len: int) -> List[bytes]:
    return [raw[i * digest_len:(i + 1) * digest_len] for i in range(cnt)]


def blake2b_host(messages: Sequence[bytes], digest_len: int = 32, threads: int = 0) -> List[bytes]:
    """rs_blake2b_host: BLAKE2b on the host CPU (no context, no GPU)."""
    if not messages:
        return []
    keep, ptrs, lens = _message_table(messages)
    out = ctypes.create_string_buffer(len(messages) * digest_len)
    _check(_lib().rs_blake2b_host(len(messages), ptrs, lens, digest_len, ctypes.cast(out, ctypes.c_void_p),
                                  threads), "rs_blake2b_host")
    return _split(out.raw, len(messages), digest_len)


def crc32c_host(buffers: Sequence[bytes]) -> List[int]:
    """rs_crc32c_host: CRC-32C (RFC 3720) of each buffer on the host CPU (no
    context, no GPU): the reference of the sector checksums."""
    if not buffers:
        return []
    keep, ptrs, lens = _message_table(buffers)
    out = (ctypes.c_uint32 * len(buffers))()
    _check(_lib().rs_crc32c_host(len(buffers), ptrs, lens, ctypes.cast(out, ctypes.c_void_p)), "rs_crc32c_host")
    return list(out)


def NewFEC(k: int, n: int) -> FEC:
    """infectious.NewFEC(k, n) (main.go:73, :248)."""
    return FEC(k, n)


def strerror(code: int) -> str:
    return _lib().rs_strerror(code).decode()

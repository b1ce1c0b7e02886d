"""CPU: rs_crc32c_host, the host reference of the sector checksums (CRC-32C,
RFC 3720), against the RFC's vectors and a bitwise model; and the NULL-ctx
refusal of every checksum call that takes a context."""
import ctypes

import numpy as np

import rsmi

VECTORS = [
    (b"123456789", 0xE3069283),
    (bytes(32), 0x8A9136AA),
    (b"\xff" * 32, 0x62A8AB43),
    (bytes(range(32)), 0x46DD794E),
    (bytes(range(31, -1, -1)), 0x113FDB5C),
    (b"", 0),
]


def bitwise(buf: bytes) -> int:
    """CRC-32C bit by bit: reflected polynomial 0x82F63B78, initial value and
    final XOR 0xFFFFFFFF."""
    crc = 0xFFFFFFFF
    for byte in buf:
        crc ^= byte
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


def test_rfc_vectors():
    for buf, want in VECTORS:
        assert bitwise(buf) == want, "the test's own model"
    assert rsmi.crc32c_host([b for b, _ in VECTORS]) == [c for _, c in VECTORS]
    assert rsmi.crc32c_host([]) == []


def test_against_bitwise_model():
    rng = np.random.default_rng(32)
    lens = list(range(301)) + [4095, 4096, 4097, 65535, 65536, 65537]
    bufs = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in lens]
    got = rsmi.crc32c_host(bufs)
    for n, buf, g in zip(lens, bufs, got):
        assert g == bitwise(buf), n
    # any alignment of the buffer
    base = rng.integers(0, 256, size=100, dtype=np.uint8).tobytes()
    views = [base[o:o + 61] for o in range(9)]
    assert rsmi.crc32c_host(views) == [bitwise(v) for v in views]


def test_count_and_null_arrays():
    lib = rsmi.load()
    out = (ctypes.c_uint32 * 2)(7, 7)
    ptrs = (ctypes.c_void_p * 1)(None)
    lens = (ctypes.c_size_t * 1)(0)
    assert lib.rs_crc32c_host(0, None, None, None) == rsmi.RS_OK
    assert lib.rs_crc32c_host(1, None, lens, ctypes.cast(out, ctypes.c_void_p)) == rsmi.RS_EINVAL
    assert lib.rs_crc32c_host(1, ptrs, None, ctypes.cast(out, ctypes.c_void_p)) == rsmi.RS_EINVAL
    assert lib.rs_crc32c_host(1, ptrs, lens, None) == rsmi.RS_EINVAL
    assert lib.rs_crc32c_host(-1, ptrs, lens, ctypes.cast(out, ctypes.c_void_p)) == rsmi.RS_EINVAL
    # a NULL buffer of length 0 is the empty message; of length 1 it is refused
    assert lib.rs_crc32c_host(1, ptrs, lens, ctypes.cast(out, ctypes.c_void_p)) == rsmi.RS_OK
    assert list(out) == [0, 7]
    lens[0] = 1
    assert lib.rs_crc32c_host(1, ptrs, lens, ctypes.cast(out, ctypes.c_void_p)) == rsmi.RS_EINVAL
    assert list(out) == [0, 7]


def test_null_context_is_rejected_without_a_device():
    lib = rsmi.load()
    st = (ctypes.c_int * 1)()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.rs_crc32c_stripes(None, p, 16, p, 16, 16, 16, 1, None, 512, p, 1, None) == rsmi.RS_EINVAL
    assert lib.rs_crc32c_check_stripes(None, p, 16, p, 16, 16, 16, 1, None, 512, p, 1, p, None) == rsmi.RS_EINVAL
    assert lib.rs_crc32c_ptrs(None, p, 16, 1, None, 512, p, 1, None) == rsmi.RS_EINVAL
    assert lib.rs_crc32c_check_ptrs(None, p, 16, 1, None, 512, p, 1, p, None) == rsmi.RS_EINVAL
    assert lib.rs_correct_crc32c(None, p, 16, p, 16, 16, 16, 1, None, 512, p, 1, st, p, None) == rsmi.RS_EINVAL
    assert buf.raw == bytes(64)

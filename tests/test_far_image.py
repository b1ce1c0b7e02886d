"""CPU: the far-address checker (far_image.py) notices the bugs it exists for.

The whole model runs at wrap = 2^16 instead of 2^32 on numpy buffers of a few
hundred KiB: RS(6,9) stripes of 40-byte shards with a pitch of 2^14 + 48 behind
a margin of 2^15 + 256, so that shard * pitch and stripe * stride leave the low
16 bits exactly as the GPU layouts leave the low 32.  A numpy "engine" encodes
the stripes through a given address function: the exact one passes, and one
with a truncated product, a sign-extended offset or a stray store fails.
"""
import numpy as np
import pytest

import far_image as fi
from strided_image import r16

WRAP = 1 << 16
K, N, S, PITCH = 6, 9, 40, (1 << 14) + 48


def layout(mode="joined", stripes=2, **kw):
    return fi.FarLayout(K, N, S, stripes, PITCH, mode, wrap=WRAP, **kw)


# -- address functions: the offset of (stripe, shard) from a base pointer -------
def exact(s, stride, i, pitch):
    return s * stride + i * pitch


def stripe_product_truncated(s, stride, i, pitch):
    return (s * stride) % WRAP + i * pitch


def shard_product_truncated(s, stride, i, pitch):
    return s * stride + (i * pitch) % WRAP


def offset_sign_extended(s, stride, i, pitch):
    t = (s * stride + i * pitch) % WRAP
    return t - WRAP if t >= WRAP // 2 else t


def encode_engine(dev, offset):
    """rs_encode_stripes on the host: round_up(S, 16) bytes of every data shard
    of every listed stripe are read and of every parity shard written, each at
    base + offset(stripe, stride, shard, pitch)."""
    L, span = dev.L, r16(dev.L.S)
    data = (dev.bufs[0], L.margin)
    parity = (dev.bufs[1], L.margin) if L.mode == "split" else (dev.bufs[0], L.margin + L.k * L.pitch)
    for s in L.listed:
        at = [data[1] + offset(s, L.dss, i, L.pitch) for i in range(L.k)]
        cols = np.stack([data[0][a:a + span] for a in at])
        assert cols.shape == (L.k, span), "a read left the buffer"
        par = fi.oracle_parity_columns(L.k, L.n, cols)
        for r in range(L.m):
            a = parity[1] + offset(s, L.pss, r, L.pitch)
            assert 0 <= a and a + span <= len(parity[0]), "a store left the buffer"
            parity[0][a:a + span] = par[r]


def encode_image(L):
    """Parity slots start as garbage; every one must hold the oracle's parity."""
    img = L.image()
    rng = np.random.default_rng(5)
    for s in L.listed:
        for i in range(L.k, L.n):
            img.garbage(s, i, rng)
    for s in L.listed:
        for i in range(L.k, L.n):
            img.expect_written(s, i)
    return img


def run(L, offset, after=None):
    dev = encode_image(L).upload(fi.NumpyBuffers())
    encode_engine(dev, offset)
    if after:
        after(dev)
    dev.check(offset.__name__)


def test_layout_is_far_at_this_wrap():
    L = layout()
    assert L.margin == WRAP // 2 + 256 and L.dss == N * PITCH + 64
    assert 3 * PITCH < WRAP < 4 * PITCH and L.dss > WRAP          # shards 4, 5 and stripe 1 leave the low 16 bits
    assert sum(L.sizes) < 400 * 1024
    assert L.shard_at(1, 7) == (0, L.margin + K * PITCH + L.dss + PITCH)
    assert L.args([1 << 20]) == ((1 << 20) + L.margin, L.dss, (1 << 20) + L.margin + K * PITCH, L.dss, PITCH, S, 2)
    kinds = [w[3] for w in L.windows]
    assert kinds.count("slot") == 2 * N and kinds.count("alias") >= 2 * N
    # every alias of every slot is watched, exactly
    for s in range(2):
        for i in range(N):
            b, o = L.shard_at(s, i)
            assert L.aliases(o), (s, i)
            for a in L.aliases(o):
                L.locate(b, a - fi.GUARD, L.win)
    Ls = layout("split", 3)
    assert (Ls.dss, Ls.pss) == (K * PITCH + 48, 3 * PITCH + 16) and 2 * Ls.pss > WRAP
    assert Ls.shard_at(2, 8) == (1, Ls.margin + 2 * Ls.pss + 2 * PITCH)
    p = [1 << 20, 1 << 24]
    assert Ls.args(p) == (p[0] + Ls.margin, Ls.dss, p[1] + Ls.margin, Ls.pss, PITCH, S, 3)


@pytest.mark.parametrize("mode,stripes", [("joined", 2), ("split", 3)])
def test_exact_engine_passes(mode, stripes):
    run(layout(mode, stripes), exact)


@pytest.mark.parametrize("mode,stripes", [("joined", 2), ("split", 3)])
@pytest.mark.parametrize("offset", [stripe_product_truncated, shard_product_truncated, offset_sign_extended])
def test_truncated_engines_are_caught(offset, mode, stripes):
    L = layout(mode, stripes)
    # the mutation changes an address of this layout at all
    assert any(offset(s, L.dss, i, PITCH) != exact(s, L.dss, i, PITCH) for s in range(stripes) for i in range(K))
    with pytest.raises(AssertionError, match="bytes differ in window"):
        run(L, offset)


def test_store_past_a_window_is_caught_by_the_segment_sums():
    L = layout()
    b, o = L.shard_at(1, K)
    past = o + r16(S) + fi.GUARD
    with pytest.raises(AssertionError, match="outside every window"):
        L.locate(b, past, 16)

    def stray(dev):
        dev.bufs[b][past:past + 16] = np.random.default_rng(9).integers(0, 256, size=16, dtype=np.uint8)

    with pytest.raises(AssertionError, match="segment sums differ"):
        run(L, exact, after=stray)
    # ... and the windows alone would not have: the same engine passes the window comparison
    dev = encode_image(L).upload(fi.NumpyBuffers())
    encode_engine(dev, exact)
    stray(dev)
    dev.img.check(lambda bb, off, length: dev.bufs[bb][off:off + length], "windows only")


def test_untouched_loose_and_flipped_bytes():
    """The model's own rules: a shard that was expected and not written fails;
    the padding behind S of a written shard is exempt and counted; a flipped
    byte stays or is repaired as the image says."""
    L = layout()
    with pytest.raises(AssertionError, match="bytes differ in window"):
        dev = encode_image(L).upload(fi.NumpyBuffers())
        dev.check("nothing ran")
    img = L.image()
    img.flip(0, 2, 7, 0x5A)
    img.flip(1, 8, S - 1, 0x01, repaired=True)
    dev = img.upload(fi.NumpyBuffers())
    b, o = L.shard_at(1, 8)
    assert dev.bufs[b][o + S - 1] == L.shard(1, 8)[S - 1] ^ 0x01
    dev.bufs[b][o + S - 1] ^= 0x01
    dev.check("flips")
    img.expect_written(1, 8)
    assert img.written == 1 and img.slack == r16(S) - S
    img.loose[0][:1] = True  # a byte exempted that no written shard accounts for
    with pytest.raises(AssertionError, match="loose bytes"):
        img.check(lambda bb, off, length: dev.bufs[bb][off:off + length])


def test_window_overlap_is_refused():
    with pytest.raises(AssertionError, match="slot windows overlap"):
        fi.FarLayout(K, N, S, 2, r16(S) + 32, "joined", wrap=WRAP)
    with pytest.raises(AssertionError, match="leaves the allocation"):
        layout(margin=64)
    with pytest.raises(AssertionError, match="pitch must hold"):
        fi.FarLayout(K, N, S, 2, 32, "joined", wrap=WRAP)


def test_far_by_stripe_index_layout():
    """Many stripes of a small pitch, three of them materialised: windows of
    neighbouring shards merge, and a truncated stripe product is caught."""
    stripes = (1 << 6) + 3
    stride = 14 * 80 + 64
    mid = -(-WRAP // stride)
    L = fi.FarLayout(10, 14, S, stripes, 80, "joined", wrap=WRAP, listed=[0, mid, stripes - 1], merge=True)
    assert (mid - 1) * L.dss < WRAP <= mid * L.dss and L.dss == stride
    assert len(L.regions) < len(L.windows)
    run(L, exact)
    with pytest.raises(AssertionError, match="bytes differ in window"):
        run(L, stripe_product_truncated)


def test_segment_sums_ragged_end():
    nb = fi.NumpyBuffers()
    buf = np.arange(4096 * 2 + 13, dtype=np.uint64).astype(np.uint8)
    sums = nb.sums(buf, 4096)
    assert len(sums) == 3
    assert sums[0] == int(np.frombuffer(buf[:4096], dtype=np.int64).sum())
    assert sums[2] == int(np.frombuffer(buf[8192:8200], dtype=np.int64).sum()) + int(buf[8200:].astype(np.int64).sum())
    buf[8192 + 12] ^= 1
    assert nb.sums(buf, 4096)[:2] == sums[:2] and nb.sums(buf, 4096)[2] != sums[2]


def test_sampled_columns():
    n = ((1 << 31) + 8232 + 15) // 16
    cols = fi.sampled_columns(n)
    c2g = 1 << 27
    for c in (0, 1, 511, 512, c2g - 513, c2g - 1, c2g, c2g + 1, c2g + 511, c2g + 512, n - 2, n - 1):
        assert c in cols  # test_bitslice_rec_past_2gib's set
    assert cols == sorted(set(cols)) and cols[0] == 0 and cols[-1] == n - 1 and len(cols) < 40
    assert fi.sampled_columns(3) == [0, 1, 2]
    idx = fi.column_index([0, 2])
    assert idx.tolist() == list(range(16)) + list(range(32, 48))

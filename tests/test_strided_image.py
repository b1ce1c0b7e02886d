"""The whole-image model of test_gpu_strided_image.py has teeth: one flipped
byte in any region that a call must leave alone -- or in the payload it must
write -- makes Image.check() fail and name the offset; only the padding
[S, round_up(S, 16)) of written shards is exempt, and the exemption cannot
grow.  No GPU: the "device bytes" are copies of the model."""
import numpy as np
import pytest

import strided_image as si

K, N, S, STRIPES = 4, 6, 100, 3   # round_up(S, 16) = 112: 12 loose bytes per written shard


def flipped(img, buf, off):
    got = [w.copy() for w in img.want]
    got[buf][off] ^= 0x01
    return got


def raises_at(img, buf, off):
    with pytest.raises(AssertionError, match=rf"{img.names[buf]}: 1 bytes differ, first offsets \[{off}\]"):
        img.check(flipped(img, buf, off))


@pytest.mark.parametrize("mode", ["split", "joined"])
def test_layout_geometry(mode):
    L = si.Layout(K, N, S, STRIPES, seed=1, mode=mode)
    data, dss, parity, pss, pitch, shard_len, stripes = L.args([0x10000, 0x90000])
    assert pitch == 112 + 32 and shard_len == S and stripes == STRIPES
    if mode == "split":
        assert (dss, pss) == (K * pitch + 48, (N - K) * pitch + 16)
        assert (data, parity) == (0x10000 + si.GUARD, 0x90000 + si.GUARD)
        assert [len(b) for b in L.pristine] == [2 * si.GUARD + STRIPES * dss, 2 * si.GUARD + STRIPES * pss]
    else:
        assert dss == pss == N * pitch + 64 and parity == data + K * pitch
        assert [len(b) for b in L.pristine] == [2 * si.GUARD + STRIPES * dss]
    E = si.oracle.fec_matrix(K, N)
    for s in range(STRIPES):
        shards = []
        for i in range(N):
            b, o = L.shard_at(s, i)
            assert o % 16 == 0 and si.GUARD <= o and o + pitch <= len(L.pristine[b]) - si.GUARD
            shards.append(L.pristine[b][o:o + S].tobytes())
        assert b"".join(shards[K:]) == si.oracle.encode(E, K, N, b"".join(shards[:K]))


@pytest.mark.parametrize("mode", ["split", "joined"])
def test_encode_image_has_teeth(mode):
    L = si.Layout(K, N, S, STRIPES, seed=2, mode=mode)
    img = L.encode_image(seed=3)
    img.check([w.copy() for w in img.want])
    assert img.written == STRIPES * (N - K)
    for b in range(len(img.init)):  # before the call the parity is garbage
        assert (b == len(img.init) - 1) == (not np.array_equal(img.init[b], L.pristine[b]))
    pb, po = L.shard_at(1, K + 1)
    db, do = L.shard_at(2, 0)
    raises_at(img, pb, po)                       # payload of a parity shard, first byte
    raises_at(img, pb, po + S - 1)               # ... and last
    raises_at(img, pb, po + si.r16(S))           # padding behind round_up(S, 16)
    raises_at(img, pb, po + L.pitch - 1)
    raises_at(img, db, do + 17)                  # the data an encode only reads
    raises_at(img, db, do + S + 3)               # ... and its padding
    raises_at(img, db, si.GUARD + L.dss - 1)     # a stride gap (the last byte of stripe 0's stride)
    raises_at(img, pb, L.shard_at(0, N - 1)[1] + L.pitch)  # the gap behind stripe 0's last parity shard
    for b in range(len(img.init)):               # guard bands, both ends of every buffer
        raises_at(img, b, 0)
        raises_at(img, b, si.GUARD - 1)
        raises_at(img, b, len(img.init[b]) - si.GUARD)
        raises_at(img, b, len(img.init[b]) - 1)
    for off in range(po + S, po + si.r16(S)):    # the exempt bytes
        img.check(flipped(img, pb, off))


def test_reconstruct_image_has_teeth():
    L = si.Layout(K, N, S, STRIPES, seed=4, mode="joined")
    er = np.zeros((STRIPES, N), dtype=np.uint8)
    er[0, [1, 4]] = 1
    er[2, 3] = 1
    img = L.reconstruct_image(er, seed=5)
    img.check([w.copy() for w in img.want])
    assert img.written == 3
    _, eo = L.shard_at(0, 1)
    _, so = L.shard_at(0, 2)
    assert np.array_equal(img.want[0][eo:eo + S], L.pristine[0][eo:eo + S])          # regenerated
    assert not np.array_equal(img.init[0][eo:eo + S], L.pristine[0][eo:eo + S])      # from garbage
    assert np.array_equal(img.want[0][eo + si.r16(S):eo + L.pitch], img.init[0][eo + si.r16(S):eo + L.pitch])
    raises_at(img, 0, eo + 50)                   # an erased shard's payload
    raises_at(img, 0, eo + si.r16(S))            # the garbage behind it
    raises_at(img, 0, so + 50)                   # a survivor
    raises_at(img, 0, so + S)                    # a survivor's padding, inside round_up(S, 16)
    raises_at(img, 0, so + L.pitch - 1)          # ... and behind it
    raises_at(img, 0, L.shard_at(1, 0)[1] + 5)   # a stripe with nothing erased
    img.check(flipped(img, 0, eo + S))           # exempt
    # repaired in part: stripe 2's shard keeps its garbage
    part = er.copy()
    part[2] = 0
    half = L.reconstruct_image(er, seed=5, repaired=part)
    assert half.written == 2 and all(np.array_equal(a, b) for a, b in zip(half.init, img.init))
    with pytest.raises(AssertionError):
        half.check([w.copy() for w in img.want])


def test_pool_image_has_teeth():
    P = si.Pool(K, N, S, STRIPES, seed=6)
    assert P.nrows == STRIPES * N + si.DECOYS and P.row_bytes == 112 + 32
    assert len(set(P.rows.reshape(-1)) | set(P.decoys)) == P.nrows
    tab = P.table(0x40000)
    assert tab.shape == (STRIPES, N) and tab[1, 2] == 0x40000 + P.row_at(P.rows[1, 2]) and (tab % 16 == 0).all()
    er = np.zeros((STRIPES, N), dtype=np.uint8)
    er[1, [0, 5]] = 1
    img = P.reconstruct_image(er, seed=7)
    img.check([w.copy() for w in img.want])
    eo, so, do = P.row_at(P.rows[1, 5]), P.row_at(P.rows[1, 1]), P.row_at(P.decoys[7])
    raises_at(img, 0, eo)
    raises_at(img, 0, eo + P.row_bytes - 1)
    raises_at(img, 0, so + S + 1)                # a survivor's padding
    raises_at(img, 0, do)                        # a decoy row
    raises_at(img, 0, do + P.row_bytes - 1)
    raises_at(img, 0, si.GUARD - 1)
    raises_at(img, 0, len(img.init[0]) - si.GUARD)
    img.check(flipped(img, 0, eo + S + 11))


def test_enlarged_loose_mask_is_refused():
    L = si.Layout(K, N, S, STRIPES, seed=8, mode="split")
    img = L.encode_image(seed=9)
    _, po = L.shard_at(0, K)
    img.loose[1][po + si.r16(S)] = True          # one more byte exempt
    with pytest.raises(AssertionError, match="loose bytes"):
        img.check([w.copy() for w in img.want])
    img.loose[1][po + si.r16(S)] = False
    img.check([w.copy() for w in img.want])
    img.written += 1                             # the count follows the written shards
    with pytest.raises(AssertionError, match="loose bytes"):
        img.check([w.copy() for w in img.want])


def test_erasure_sets():
    for k, n in ((10, 14), (64, 80), (5, 8)):
        er = si.erasure_set(k, n, seed=1)
        e = er.sum(axis=1)
        assert len(er) == len(si.fixed_patterns(k, n)) + 17 and e.max() == n - k and e[-1] == 0
        assert (e[:-1] >= 1).all()
    row = np.zeros(80, dtype=np.uint8)
    assert si.lowest_parity_row(row, 64, 80) == 16
    row[[0, 1]] = 1
    assert si.lowest_parity_row(row, 64, 80) == 14   # survivors: parity rows 15 and 14
    row[64 + 15] = 1
    assert si.lowest_parity_row(row, 64, 80) == 13   # row 15 erased: survivors 14 and 13
    row[64 + 2] = 1
    assert si.lowest_parity_row(row, 64, 80) == 2

"""GPU: whole-image checks of rs_encode_stripes, rs_reconstruct_stripes and
rs_reconstruct_ptrs on strided layouts (strided_image.py).

Every call under test gets a shard pitch above round_up(S, 16), stripe strides
with gaps that differ between data and parity (or one allocation of whole
stripes, parity = data + k * pitch), and buffers with guard bands; everything
that is not payload is random bytes.  After the call the WHOLE image of every
device buffer is compared with a host model: the written shards hold the
oracle's bytes in [0, S), and every other byte -- the data an encode reads,
survivors, pitch padding behind round_up(S, 16), stride gaps, guards, decoy
rows, the pointer table -- is what was placed there before the call.  Only
bytes [S, round_up(S, 16)) of written shards are exempt (rsmi.h: "bytes
between shard_len and the next multiple of 16 are coded too: padding").

Each test asserts the kernel names and the reconstruct counters, so it fails
if routing moves away from the kernel it is meant to exercise.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the RSMI_ITERS / RSMI_NT children
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "noise-erasurecode-plugin_amd"), os.path.join(_root, "tests")):
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
import strided_image as si  # noqa: E402

# id: (k, n), RSMI_* knobs of the context, kernel_name(0), kernel_name(1),
# erasure caps of the reconstruct calls (the split-table variant of a launch
# is chosen by its largest erasure count: one call per row-group size), and
# the least erasure count the syndrome kernel takes (None: no syndrome kernel).
IDS = {
    # register pointers, dynamic rows
    "t10": ((10, 14), {}, "K10_MG4_B256", "K10_MG4_B256", None, None),
    # m < MG
    "t4": ((4, 6), {}, "K4_MG4_B256", "K4_MG4_B256", None, None),
    # K8_MG6 encode, K8_MG4 / K8_MG6 reconstruct
    "t8": ((8, 14), {"RSMI_BITSLICE": "0"}, "K8_MG6_B256", "K8_MG6_B256", (4, 6), None),
    # K64_MG16 encode, K64_MG4 / K64_MG8 / K64_MG16 reconstruct (LDS pointers)
    "t64": ((64, 80), {"RSMI_BITSLICE": "0", "RSMI_BITSLICE_REC": "0"}, "K64_MG16_B256", "K64_MG16_B256",
            (4, 8, 16), None),
    # m = 36: three row groups of 16, the last one of 4 rows
    "t64w": ((64, 100), {}, "K64_MG16_B256", "K64_MG16_B256", None, None),
    # runtime k, m = 3
    "r5": ((5, 8), {}, "K0_MG4_B256", "K0_MG4_B256", None, None),
    # runtime k, m = 32: four row groups of 8
    "r17": ((17, 49), {}, "K0_MG8_B256", "K0_MG8_B256", None, None),
    "b64": ((64, 80), {"RSMI_SMALL_SPLIT": "0"}, "bitslice_k64_m16", "bitslice_rec_k64_m16", None, 1),
    # the t4 / t8 row-subset syndrome kernels next to the full one
    "b64t": ((64, 80), {"RSMI_SMALL_SPLIT": "0", "RSMI_BITSLICE_TOPS": "1"}, "bitslice_k64_m16",
             "bitslice_rec_k64_m16 +t4,8", None, 1),
    # split table (e < 5) and syndrome kernel in one call
    "b64s": ((64, 80), {"RSMI_SMALL_SPLIT": "0", "RSMI_BITSLICE_REC_MIN_E": "5"}, "bitslice_k64_m16",
             "K64_MG4_B256 (e<5) + bitslice_rec_k64_m16", None, 5),
    "b8": ((8, 14), {"RSMI_SMALL_SPLIT": "0"}, "bitslice_k8_m6", "bitslice_rec_k8_m6", None, 1),
    "b10": ((10, 14), {"RSMI_BITSLICE": "1", "RSMI_BITSLICE_REC_MIN_E": "1", "RSMI_SMALL_SPLIT": "0"},
            "bitslice_k10_m4", "bitslice_rec_k10_m4", None, 1),
}
# Split-table kernels, one block per 256 columns: one column | exactly one
# block | a block plus one live lane | not a multiple of 16.
TABLE_S = [16, 4096, 4112, 5000]
# Bit-sliced kernels, one block per 512 columns, a wave per 128 of them, lane
# l coding columns l and 64 + l of its wave's (bs_cols, geometry 0): a lone
# column | a ragged second column | 65 columns: one live lane of the upper
# half, waves 1-3 idle | 257 columns: one lane of wave 2, its upper column
# past the end | exactly one window | a window plus one column | a partial,
# ragged second window.
BITS_S = [16, 17, 1040, 4112, 8192, 8208, 12328]
MODES = ["split", "joined"]
PTR_IDS = ["t10", "t64", "r17", "b64", "b64t", "b8"]


def sizes(name):
    return BITS_S if name.startswith("b") else TABLE_S


def stripe_counts(name):
    return [1, 9] if IDS[name][0][0] == 64 or name == "r17" else [1, 9, 19]


def _encode_cases():
    """Every id meets every S of its family in both modes, and every stripe
    count: S number i runs with counts i and i + 1 (cyclic)."""
    out = []
    for name in IDS:
        cnt = stripe_counts(name)
        for i, S in enumerate(sizes(name)):
            for j in (0, 1):
                out.append((name, S, cnt[(i + j) % len(cnt)], MODES[(i + j) % 2]))
    return out


def _reconstruct_cases():
    """Every id meets every S of its family, the modes alternating; ids of
    one code and S follow each other and share the oracle's stripes."""
    out = [(S, q, name, MODES[(i + q) % 2]) for q, name in enumerate(IDS) for i, S in enumerate(sizes(name))]
    return [(name, S, mode) for S, q, name, mode in sorted(out, key=lambda c: (c[2][0], c[0], c[1]))]


def _fec_env(k, n, **env):
    """FEC built with RSMI_* knobs set (the kernel choice is made at rs_new)."""
    old = {key: os.environ.get(key) for key in env}
    os.environ.update(env)
    try:
        return rsmi.NewFEC(k, n)
    finally:
        for key, v in old.items():
            if v is None:
                del os.environ[key]
            else:
                os.environ[key] = v


_CTX = {}


def ctx(name):
    if name not in _CTX:
        (k, n), env = IDS[name][:2]
        _CTX[name] = _fec_env(k, n, **env)
    return _CTX[name]


def assert_kernels(f, name, suffix=""):
    _, _, enc, rec, _, _ = IDS[name]
    assert f.kernel_name(0) == enc + suffix, (name, f.kernel_name(0))
    assert f.kernel_name(1) == rec + suffix, (name, f.kernel_name(1))


_LAYOUTS = {}


def layout(name, S, stripes, mode):
    k, n = IDS[name][0]
    key = (k, n, S, stripes, mode)
    if key not in _LAYOUTS:
        while len(_LAYOUTS) >= 8:  # the last few: neighbouring cases share them
            del _LAYOUTS[next(iter(_LAYOUTS))]
        _LAYOUTS[key] = si.Layout(k, n, S, stripes, seed=k * 7919 + n * 104729 + S * 13 + stripes + len(mode), mode=mode)
    return _LAYOUTS[key]


def upload(img):
    return [torch.from_numpy(b).cuda() for b in img.init]


def download(dev):
    return [t.cpu().numpy() for t in dev]


def check_encode(f, L, what):
    img = L.encode_image(seed=L.S + L.stripes)
    dev = upload(img)
    f.encode_stripes(*L.args([t.data_ptr() for t in dev]))
    f.sync()
    img.check(download(dev), what)


def check_reconstruct(f, name, L, er, what):
    """One reconstruct call per erasure cap on the same device buffers: a
    call flags the stripes whose erasure count lies in (previous cap, cap],
    and the shards of the others, destroyed or not, must stay as they are."""
    k, n, m = L.k, L.n, L.m
    caps, min_e = IDS[name][4] or (m,), IDS[name][5]
    e = er.sum(axis=1)
    dev = upload(L.reconstruct_image(er, seed=L.S + 1))
    args = L.args([t.data_ptr() for t in dev])
    done = np.zeros_like(er)
    lo = 0
    for cap in caps:
        now = er * ((e > lo) & (e <= cap))[:, None].astype(np.uint8)
        lo = cap
        want_syn = int(((now.sum(axis=1) >= min_e)).sum()) if min_e else 0
        want_tab = int((now.sum(axis=1) > 0).sum()) - want_syn
        tab0, syn0 = f.stat(f.STAT_REC_STRIPES_TABLE), f.stat(f.STAT_REC_STRIPES_SYNDROME)
        f.reconstruct_stripes(*args, now.tobytes())
        f.sync()
        done |= now
        L.reconstruct_image(er, seed=L.S + 1, repaired=done).check(download(dev), f"{what} e<={cap}")
        assert f.stat(f.STAT_REC_STRIPES_TABLE) - tab0 == want_tab, (what, cap)
        assert f.stat(f.STAT_REC_STRIPES_SYNDROME) - syn0 == want_syn, (what, cap)
        if min_e and min_e > 1:
            assert want_tab > 0 and want_syn > 0, "both kernels in one call"
    assert np.array_equal(done, er)


def check_both(f, name, S, stripes, mode, what):
    check_encode(f, layout(name, S, stripes, mode), f"{what} encode {name} S={S}")
    k, n = IDS[name][0]
    er = si.random_erasures(np.random.default_rng(S + k), stripes, n, n - k)
    er[stripes // 2] = 0  # one stripe with nothing erased
    check_reconstruct(f, name, layout(name, S, stripes, mode), er, f"{what} reconstruct {name} S={S}")


@pytest.mark.parametrize("name,S,stripes,mode", _encode_cases())
def test_encode_image(name, S, stripes, mode):
    f = ctx(name)
    assert_kernels(f, name)
    check_encode(f, layout(name, S, stripes, mode), f"{name} S={S} stripes={stripes} {mode}")


@pytest.mark.parametrize("name,S,mode", _reconstruct_cases())
def test_reconstruct_image(name, S, mode):
    f = ctx(name)
    assert_kernels(f, name)
    k, n = IDS[name][0]
    er = si.erasure_set(k, n, seed=S * 3 + k)
    if name == "b64t":  # all three syndrome kernels: top 4 rows, top 8 rows, all 16
        lows = [si.lowest_parity_row(row, k, n) for row in er if row.any()]
        assert {0, 1, 2} <= {0 if lo >= 12 else 1 if lo >= 8 else 2 for lo in lows}
    e, lo = er.sum(axis=1), 0
    for cap in IDS[name][4] or ():  # every row-group size gets stripes
        assert ((e > lo) & (e <= cap)).any(), (name, S, cap)
        lo = cap
    check_reconstruct(f, name, layout(name, S, len(er), mode), er, f"{name} S={S} {mode}")


@pytest.mark.parametrize("name,S", [(name, S) for name in PTR_IDS for S in sizes(name)])
def test_reconstruct_ptrs_image(name, S):
    f = ctx(name)
    assert_kernels(f, name)
    k, n = IDS[name][0]
    er = si.erasure_set(k, n, seed=S * 3 + k)
    if name == "b64t":
        lows = [si.lowest_parity_row(row, k, n) for row in er if row.any()]
        assert {0, 1, 2} <= {0 if lo >= 12 else 1 if lo >= 8 else 2 for lo in lows}
    P = si.Pool(k, n, S, len(er), seed=S * 5 + n)
    img = P.reconstruct_image(er, seed=S + 2)
    dev = upload(img)
    table_h = P.table(dev[0].data_ptr())
    table = torch.from_numpy(table_h.copy()).cuda()
    min_e = IDS[name][5]
    erased = int(er.any(axis=1).sum())
    tab0, syn0 = f.stat(f.STAT_REC_STRIPES_TABLE), f.stat(f.STAT_REC_STRIPES_SYNDROME)
    f.reconstruct_ptrs(table.data_ptr(), S, len(er), er.tobytes())
    f.sync()
    img.check(download(dev), f"{name} S={S} pool")
    assert np.array_equal(table.cpu().numpy(), table_h), "the pointer table changed"
    assert f.stat(f.STAT_REC_STRIPES_TABLE) - tab0 == (0 if min_e else erased)
    assert f.stat(f.STAT_REC_STRIPES_SYNDROME) - syn0 == (erased if min_e else 0)


@pytest.mark.parametrize("name", ["t10", "b64"])
@pytest.mark.parametrize("knob", [{"RSMI_XCD": "0"}, {"RSMI_XCD": "1"}, {"RSMI_XCD_ENC_REGION": "3"}],
                         ids=["xcd0", "xcd1", "enc_region3"])
def test_xcd_orders_image(name, knob):
    """The XCD-aware block orders (xcd.hpp) off, on for every kernel, and with
    encode regions of 3 blocks: 9 stripes, one past a multiple of 8."""
    (k, n), env = IDS[name][:2]
    f = _fec_env(k, n, **env, **knob)
    assert_kernels(f, name)
    check_both(f, name, 4112, 9, "joined", f"{knob}")
    f.close()


def _run_child(which, env):
    run = subprocess.run([sys.executable, os.path.abspath(__file__), which], env=dict(os.environ, **env),
                         capture_output=True, text=True, timeout=180)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{which} child ok" in run.stdout


def test_matmul_multi_iteration_child():
    """RSMI_ITERS is read once per process: a child with RSMI_ITERS=2 runs
    rs_matmul_kernel's multi-iteration loop -- the software-pipelined reload
    of the register-pointer variant (t10) and the LDS pointer path (r17, t64)
    -- on 8,208-byte shards (three column chunks, two blocks: the second
    block's second iteration lies past the shard), 12,288 (three full chunks)
    and 4,112 (two chunks, one block)."""
    _run_child("iters", {"RSMI_ITERS": "2"})


def test_matmul_temporal_variant_child():
    """RSMI_NT=0 is read once per process: a child runs K10_MG4_B256_T, the
    temporal-policy twin of the headline kernel."""
    _run_child("nt", {"RSMI_NT": "0"})


if __name__ == "__main__":
    if sys.argv[1] == "iters":
        assert os.environ.get("RSMI_ITERS") == "2"
        for q, name in enumerate(("t10", "r17", "t64")):
            assert_kernels(ctx(name), name)
            for i, S in enumerate((8208, 12288, 4112)):
                check_both(ctx(name), name, S, 9, MODES[(i + q) % 2], "iters")
    elif sys.argv[1] == "nt":
        assert os.environ.get("RSMI_NT") == "0"
        assert ctx("t10").kernel_name(0) == "K10_MG4_B256_T"
        assert_kernels(ctx("t10"), "t10", suffix="_T")
        for i, S in enumerate((16, 5000)):
            check_both(ctx("t10"), "t10", S, 9, MODES[i], "nt")
    print(f"{sys.argv[1]} child ok")

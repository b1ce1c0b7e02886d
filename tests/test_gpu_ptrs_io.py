"""GPU: rs_encode_ptrs, rs_update_ptrs and rs_read_ptrs -- writing parity,
overwriting shards and serving degraded reads on the pointer placement (shard
i of stripe s at shard_ptrs[s * n + i], anywhere in device memory).

Every case is a ptrs_io_model.Case: one arena -- a strided_image.Pool (random
rows, row padding, decoys, guard bands) and behind it the call's src or dst
buffers, each with a guard band -- and a table in which every entry the call
must not load names a DECOY row, so that a mistake shows as a wrong byte or a
changed decoy, never as a fault.  After every call the WHOLE arena and the
device table are compared with the expected image, whose bytes never come from
the engine (oracle parity, oracle re-encode of updated data, the bytes the pool
held before shards were lost).  Each call is also compared bit for bit with
its strided counterpart on a strided copy of the same stripes.
"""
import ctypes
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from ptrs_io_model import encode_case, read_case, update_case  # noqa: E402
from strided_image import Pool, fixed_patterns, r16, random_erasures  # noqa: E402

CLEAN = rsmi.RS_VERIFY_CLEAN
# register pointers, MG4 | MG8 | runtime k, MG16 | bit-sliced encode twin, LDS
# pointer path | m = 28: several row groups, the update's commit by copy | m = 1
# | k = 1 | m = 0 | n = 256
CODES = {"rs4_6": (4, 6), "rs10_14": (10, 14), "rs8_14": (8, 14), "rs3_19": (3, 19), "rs64_80": (64, 80),
         "rs12_40": (12, 40), "rs4_5": (4, 5), "rs1_3": (1, 3), "rs3_3": (3, 3), "rs240_256": (240, 256)}
# one column | exactly one 4 KiB block chunk | a chunk plus one column | not a
# multiple of 16 | several chunks
SHAPES = [16, 4096, 4112, 5000, 3 * 4096 + 40]
STRIPES = [1, 3, 37]
CASES = ([(c, S, st) for c in CODES if c != "rs240_256" for S in SHAPES for st in STRIPES] +
         # one bit-sliced block of 512 columns, and one column more
         [("rs64_80", S, st) for S in (8192, 8208) for st in STRIPES] +
         [("rs240_256", S, st) for S in (16, 4112) for st in STRIPES])
ENCODE_NAME = {"rs4_6": "K4_MG4_B256", "rs10_14": "K10_MG4_B256", "rs8_14": "bitslice_k8_m6_ptrs",
               "rs3_19": "K0_MG8_B256", "rs64_80": "bitslice_k64_m16_ptrs", "rs12_40": "K0_MG8_B256"}
UPDATE_NAME = {"rs4_6": "update_MG4_B256_ptrs", "rs8_14": "update_MG8_B256_ptrs", "rs3_19": "update_MG16_B256_ptrs",
               "rs64_80": "update_MG16_B256_ptrs", "rs12_40": "update_MG16_B256_ptrs", "rs4_5": "update_MG4_B256_ptrs"}
READ_NAME = {"rs4_6": "read_K4_MG4_B256_ptrs", "rs10_14": "read_K10_MG4_B256_ptrs", "rs8_14": "read_K8_MG4_B256_ptrs",
             "rs3_19": "read_K0_MG4_B256_ptrs", "rs64_80": "read_K64_MG4_B256_ptrs",
             "rs240_256": "read_K0_MG4_B256_ptrs"}

_POOLS = {}
_FECS = {}


def pool(code, S, stripes):
    key = (code, S, stripes)
    if key not in _POOLS:
        while len(_POOLS) >= 4:
            del _POOLS[next(iter(_POOLS))]
        k, n = CODES[code]
        _POOLS[key] = Pool(k, n, S, stripes, seed=k * 1000003 + n * 10007 + S * 31 + stripes)
    return _POOLS[key]


def fec(code):
    if code not in _FECS:
        _FECS[code] = rsmi.FEC(*CODES[code], device=0)
    return _FECS[code]


class Gpu:
    """ptrs_io_model's engine interface over the C ABI: the arena and the table
    go to the device, addresses become base + offset, and both come back."""

    def __init__(self, f):
        self.f = f

    def up(self, arena, table):
        self.dev = torch.from_numpy(arena).cuda()
        self.base = self.dev.data_ptr()
        assert self.base % 16 == 0
        self.tab = torch.from_numpy(table + self.base).cuda()
        return self.tab.data_ptr()

    def down(self):
        self.f.sync()
        return self.dev.cpu().numpy(), self.tab.cpu().numpy() - self.base

    def encode_ptrs(self, arena, table, S, stripes):
        self.f.encode_ptrs(self.up(arena, table), S, stripes)
        return self.down()

    def update_ptrs(self, arena, table, S, stripes, updates, offset):
        tp = self.up(arena, table)
        self.f.update_ptrs(tp, S, stripes, [(s, c, self.base + o) for s, c, o in updates], offset=offset)
        return self.down()

    def read_ptrs(self, arena, table, S, stripes, erased, reads, offset):
        tp = self.up(arena, table)
        self.f.read_ptrs(tp, S, stripes, erased.tobytes(), [(s, i, self.base + o) for s, i, o in reads],
                         offset=offset)
        return self.down()

    def verify(self, S, stripes, erased=None):
        fb = torch.zeros(stripes, dtype=torch.int32, device="cuda:0")
        self.f.verify_ptrs(self.tab.data_ptr(), S, stripes, fb.data_ptr(), erased=erased)
        self.f.sync()
        return fb.cpu().numpy().view(np.uint32)


class Strided:
    """A strided copy of a case's stripes as the arena holds them before the
    call: whole rows (padding included) at pitch row_bytes, one buffer."""

    def __init__(self, case):
        sc, P = case.sc, case.sc.P
        self.sc, self.pitch = sc, P.row_bytes
        img = np.stack([case.init[sc.at(s, i):sc.at(s, i) + P.row_bytes] for s in range(P.stripes) for i in range(sc.n)])
        self.dev = torch.from_numpy(img.reshape(-1)).cuda()

    def args(self, off=0):
        d = self.dev.data_ptr() + off
        return (d, self.sc.n * self.pitch, d + self.sc.k * self.pitch, self.sc.n * self.pitch, self.pitch)

    def rows(self):
        return self.dev.cpu().numpy().reshape(self.sc.P.stripes, self.sc.n, self.pitch)


def same_as_strided(case, got, st, what):
    """Every pool row after the pointer call equals the strided copy's row
    after the strided call (rows whose table entry named a decoy included)."""
    rows, sc = st.rows(), case.sc
    for s in range(sc.P.stripes):
        for i in range(sc.n):
            assert np.array_equal(got[0][sc.at(s, i):sc.at(s, i) + st.pitch], rows[s, i]), (what, s, i)


def erasures(P, seed):
    if P.m == 0:
        return np.zeros((P.stripes, P.n), dtype=np.uint8)
    fx = fixed_patterns(P.k, P.n)
    rnd = random_erasures(np.random.default_rng(seed), P.stripes, P.n, P.m)
    return np.stack([fx[(s // 2 + seed) % len(fx)] if s % 2 == 0 else rnd[s] for s in range(P.stripes)])


def slices(S):
    """The slice to the shard's end and a middle multiple of 16, where S has room."""
    out = []
    if S > 16:
        out.append((16, S - 16))
    if S >= 64:
        out.append((16, 16 * ((S - 16) // 32)))
    return out


# --------------------------------------------------------------- encode ----
@pytest.mark.parametrize("code,S,stripes", CASES)
def test_encode(code, S, stripes):
    P, f = pool(code, S, stripes), fec(code)
    case, g = encode_case(P, 11), Gpu(f)
    got = case.run(g)
    case.check(got, "encode_ptrs")
    if P.m:
        assert np.array_equal(g.verify(S, stripes), np.full(stripes, CLEAN, dtype=np.uint32))
    case.check(g.down(), "encode_ptrs, verified")
    st = Strided(case)
    f.encode_stripes(*st.args(), S, stripes)
    f.sync()
    same_as_strided(case, got, st, "encode_stripes")


# --------------------------------------------------------------- update ----
@pytest.mark.parametrize("code,S,stripes", CASES)
def test_update(code, S, stripes):
    P, f = pool(code, S, stripes), fec(code)
    for sl in [None] + slices(S):
        case, g = update_case(P, 12, sl=sl), Gpu(f)
        got = case.run(g)
        case.check(got, f"update_ptrs {sl}")
        off, length = sl or (0, S)
        st = Strided(case)
        src = torch.from_numpy(case.init).cuda()
        f.update_stripes(*st.args(off), length, stripes,
                         [(s, c, src.data_ptr() + o) for s, c, o in case.args["updates"]])
        f.sync()
        same_as_strided(case, got, st, f"update_stripes {sl}")
        if P.m:
            # through the real rows behind the decoys: every stripe is a codeword again
            g.up(got[0], P.table(0).reshape(-1))
            assert np.array_equal(g.verify(S, stripes), np.full(stripes, CLEAN, dtype=np.uint32)), sl


# ----------------------------------------------------------------- read ----
@pytest.mark.parametrize("code,S,stripes", CASES)
def test_read(code, S, stripes):
    P, f = pool(code, S, stripes), fec(code)
    plans = [(None, 1 if stripes >= 3 else None)] + [(sl, None) for sl in slices(S)[:1]]
    if stripes < 3:
        plans.append((None, 0))  # the only stripes there are: a call of its own for the overfull one
    for seed, (sl, overfull) in enumerate(plans):
        case, g = read_case(P, 13, erasures(P, 20 + seed), sl=sl, overfull=overfull), Gpu(f)
        got = case.run(g)
        case.check(got, f"read_ptrs {sl} overfull {overfull}")
        off, length = sl or (0, S)
        W, st = r16(length), Strided(case)
        dst = torch.zeros(len(case.args["reads"]) * W, dtype=torch.uint8, device="cuda:0")
        f.read_stripes(*st.args(off), length, stripes, case.args["erased"].tobytes(),
                       [(s, i, dst.data_ptr() + j * W) for j, (s, i, _) in enumerate(case.args["reads"])])
        f.sync()
        ref = dst.cpu().numpy()
        for j, (s, i, o) in enumerate(case.args["reads"]):
            assert np.array_equal(got[0][o:o + W], ref[j * W:(j + 1) * W]), ("read_stripes", sl, s, i)


# ------------------------------------------------------------- refusals ----
def refused(code, call, what):
    with pytest.raises(rsmi.RSError) as e:
        call()
    assert e.value.code == code, (what, e.value.code)


def test_refusals():
    P, f = pool("rs4_6", 4112, 3), fec("rs4_6")
    S, stripes, E, ID, NE = P.S, P.stripes, rsmi.RS_EINVAL, rsmi.RS_EBAD_SHARE_ID, rsmi.RS_ENOT_ENOUGH
    big = 16 << 28
    er = erasures(P, 1)
    over = er.copy()
    over[0, :3] = 1  # 3 > m erasures, and the reads below want an erased shard of stripe 0
    for case in (encode_case(P, 1), update_case(P, 2), read_case(P, 3, er)):
        g = Gpu(f)
        tp = g.up(case.init, case.table)
        b, fl = g.base, case.args.get("erased", er).tobytes()
        upd = [(s, c, b + o) for s, c, o in case.args.get("updates", [])] or [(0, 0, b + 4096)]
        rds = [(s, i, b + o) for s, i, o in case.args.get("reads", [])] or [(0, 0, b + 4096)]
        for what, code, call in [
            ("encode NULL table", E, lambda: f.encode_ptrs(0, S, stripes)),
            ("encode misaligned table", E, lambda: f.encode_ptrs(tp + 4, S, stripes)),
            ("encode 2^28 columns", E, lambda: f.encode_ptrs(tp, big, stripes)),
            ("encode 2^32 stripes", E, lambda: f.encode_ptrs(tp, S, 1 << 32)),
            ("encode 2^31 blocks", E, lambda: f.encode_ptrs(tp, 16, 1 << 31)),
            ("update NULL table", E, lambda: f.update_ptrs(0, S, stripes, upd)),
            ("update misaligned table", E, lambda: f.update_ptrs(tp + 4, S, stripes, upd)),
            ("update 2^28 columns", E, lambda: f.update_ptrs(tp, big, stripes, upd)),
            ("update offset + columns", E, lambda: f.update_ptrs(tp, S, stripes, upd, offset=big - 16)),
            ("update 2^32 stripes", E, lambda: f.update_ptrs(tp, S, 1 << 32, upd)),
            # 4,096 jobs x 2^19 column chunks of 2 GiB shards (refused before anything is read: src and
            # dst are bare aligned addresses)
            ("update 2^31 blocks", E, lambda: f.update_ptrs(tp, 1 << 31, 4096, [(s, 0, 16) for s in range(4096)])),
            ("update misaligned offset", E, lambda: f.update_ptrs(tp, 16, stripes, upd, offset=8)),
            ("update stripe >= stripes", E, lambda: f.update_ptrs(tp, S, stripes, upd + [(stripes, 0, upd[0][2])])),
            ("update duplicate", E, lambda: f.update_ptrs(tp, S, stripes, upd + upd[:1])),
            ("update misaligned src", E, lambda: f.update_ptrs(tp, S, stripes, [(0, 0, upd[0][2] + 8)])),
            ("update NULL src", E, lambda: f.update_ptrs(tp, S, stripes, [(0, 0, 0)])),
            ("update shard >= k", ID, lambda: f.update_ptrs(tp, S, stripes, [(0, P.k, upd[0][2])])),
            ("read NULL table", E, lambda: f.read_ptrs(0, S, stripes, fl, rds)),
            ("read misaligned table", E, lambda: f.read_ptrs(tp + 4, S, stripes, fl, rds)),
            ("read NULL erased", E, lambda: f.read_ptrs(tp, S, stripes, None, rds)),
            ("read 2^28 columns", E, lambda: f.read_ptrs(tp, big, stripes, fl, rds)),
            ("read offset + columns", E, lambda: f.read_ptrs(tp, S, stripes, fl, rds, offset=big - 16)),
            ("read 2^31 blocks", E, lambda: f.read_ptrs(tp, 1 << 31, 4096, bytes([1] + [0] * (P.n - 1)) * 4096,
                                                        [(s, 0, 16 + (s << 31)) for s in range(4096)])),
            ("read 2^31 copy blocks", E, lambda: f.read_ptrs(tp, 1 << 31, 4096, bytes(4096 * P.n),
                                                             [(s, 0, 16 + (s << 31)) for s in range(4096)])),
            ("read misaligned offset", E, lambda: f.read_ptrs(tp, 16, stripes, fl, rds, offset=8)),
            ("read stripe >= stripes", E, lambda: f.read_ptrs(tp, S, stripes, fl, rds + [(stripes, 0, rds[0][2])])),
            ("read duplicate", E, lambda: f.read_ptrs(tp, S, stripes, fl, rds + rds[:1])),
            ("read misaligned dst", E, lambda: f.read_ptrs(tp, S, stripes, fl, [(0, 0, rds[0][2] + 8)])),
            ("read dst ranges meet", E, lambda: f.read_ptrs(tp, S, stripes, fl, [(0, 0, rds[0][2]),
                                                                                 (0, 1, rds[0][2] + 16)])),
            ("read shard >= n", ID, lambda: f.read_ptrs(tp, S, stripes, fl, [(0, P.n, rds[0][2])])),
            ("read more than m erasures", NE, lambda: f.read_ptrs(tp, S, stripes, over.tobytes(), [(0, 0, rds[0][2])])),
        ]:
            refused(code, call, what)
        # reserved != 0, NULL ctx and 2^32 stripes of a read (the binding wants stripes * n flags): through ctypes
        lib = ctypes.CDLL(rsmi.LIB_PATH)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        lib.rs_encode_ptrs.argtypes = [vp, vp, sz, sz, vp]
        lib.rs_update_ptrs.argtypes = [vp, vp, sz, sz, sz, ctypes.POINTER(rsmi.ShardUpdate), sz, vp]
        lib.rs_read_ptrs.argtypes = [vp, vp, sz, sz, sz, vp, ctypes.POINTER(rsmi.ShardRead), sz, vp]
        ua, ra = rsmi.shard_updates(upd[:1]), rsmi.shard_reads(rds[:1])
        flags = ctypes.c_char_p(fl)
        assert lib.rs_encode_ptrs(None, tp, S, stripes, None) == E
        assert lib.rs_update_ptrs(None, tp, 0, S, stripes, ua, 1, None) == E
        assert lib.rs_read_ptrs(None, tp, 0, S, stripes, flags, ra, 1, None) == E
        assert lib.rs_read_ptrs(f._h, tp, 0, S, 1 << 32, flags, ra, 1, None) == E
        # NULL lists with count > 0 (the binding always passes an array)
        assert lib.rs_update_ptrs(f._h, tp, 0, S, stripes, None, 1, None) == E
        assert lib.rs_read_ptrs(f._h, tp, 0, S, stripes, flags, None, 1, None) == E
        ua[0].reserved = ra[0].reserved = 1
        assert lib.rs_update_ptrs(f._h, tp, 0, S, stripes, ua, 1, None) == E
        assert lib.rs_read_ptrs(f._h, tp, 0, S, stripes, flags, ra, 1, None) == E
        # nothing to do: RS_OK, nothing launched
        f.encode_ptrs(tp, S, 0)
        f.encode_ptrs(tp, 0, stripes)
        f.update_ptrs(tp, S, stripes, [])
        f.update_ptrs(tp, 0, stripes, upd)
        f.read_ptrs(tp, S, stripes, fl, [])
        f.read_ptrs(tp, S, 0, b"", rds)
        got = g.down()
        assert np.array_equal(got[0], case.init), case.op
        assert np.array_equal(got[1], case.table), case.op


def test_refusals_bitsliced_encode():
    """The block bound of the generated twin's grid: 2^31 stripes of one
    block each, refused before the table is read."""
    P, f = pool("rs64_80", 16, 3), fec("rs64_80")
    assert f.kernel_name(20) == "bitslice_k64_m16_ptrs"
    case, g = encode_case(P, 1), Gpu(f)
    tp = g.up(case.init, case.table)
    refused(rsmi.RS_EINVAL, lambda: f.encode_ptrs(tp, 16, 1 << 31), "bit-sliced encode 2^31 blocks")
    refused(rsmi.RS_EINVAL, lambda: f.encode_ptrs(tp, 8208, 1 << 30), "bit-sliced encode 2^31 blocks, two per stripe")
    refused(rsmi.RS_EINVAL, lambda: f.encode_ptrs(tp + 4, 16, 3), "bit-sliced encode misaligned table")
    got = g.down()
    assert np.array_equal(got[0], case.init) and np.array_equal(got[1], case.table)


# --------------------------------------------------------- kernel names ----
@pytest.mark.parametrize("code", sorted(CODES))
def test_kernel_names(code):
    f = fec(code)
    k, n = CODES[code]
    enc = f.kernel_name(20)
    if code in ENCODE_NAME:
        assert enc == ENCODE_NAME[code]
    # a twin exists for a bit-sliced encode only: the split-table kernel reads the table itself
    assert (enc != f.kernel_name(0)) == f.kernel_name(0).startswith("bitslice"), (enc, f.kernel_name(0))
    if enc != f.kernel_name(0):
        assert enc == f.kernel_name(0) + "_ptrs"
    assert f.kernel_name(21) == f.kernel_name(3) + "_ptrs" == UPDATE_NAME.get(code, f.kernel_name(21))
    assert f.kernel_name(22) == f.kernel_name(4) + "_ptrs" == READ_NAME.get(code, f.kernel_name(22))


# -------------------------------------------------------------- threads ----
def test_four_threads_one_ctx():
    f = fec("rs10_14")
    errors = []
    # the pools and the cases are made here: the threads only call the engine and compare
    cases = []
    for t in range(4):
        P = Pool(10, 14, 4112 + 16 * t, 5, seed=700 + t)
        cases.append([c for rep in range(3) for c in (encode_case(P, 40 + t), update_case(P, 50 + t + rep),
                                                      read_case(P, 60 + t, erasures(P, 70 + t + rep), overfull=1))])

    def work(t):
        try:
            for i, case in enumerate(cases[t]):
                case.check(case.run(Gpu(f)), f"thread {t} call {i}")
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# -------------------------------------------------------- life sequence ----
def combine_encode(f, E, g, sc, table, S, stripes):
    b = g.base
    t = table.reshape(stripes, sc.n)
    f.combine([([b + t[s, c] for c in range(sc.k)], [b + t[s, i] for i in range(sc.k, sc.n)],
                E[sc.k * sc.k:], 0) for s in range(stripes)], S)


def combine_update(f, E, g, sc, table, S, stripes, updates):
    """update_by_combine's route for present shards: parity ^= E * (old ^ new)
    as one accumulate job per stripe over (old, new) pairs, then the commit."""
    b, t, k = g.base, table.reshape(stripes, sc.n), sc.k
    by = {}
    for s, c, o in updates:
        by.setdefault(s, []).append((c, o))
    jobs = []
    for s, lst in by.items():
        src = [b + t[s, c] for c, _ in lst] + [b + o for _, o in lst]
        coef = bytes(E[(k + r) * k + c] for r in range(sc.m) for c, _ in lst * 2)
        jobs.append((src, [b + t[s, i] for i in range(k, sc.n)], coef, 1))
    f.combine(jobs, S)
    f.combine([([b + o], [b + t[s, c]], bytes([1]), 0) for s, c, o in updates], S)


def combine_read(f, g, sc, table, S, stripes, er, reads):
    b, t, k = g.base, table.reshape(stripes, sc.n), sc.k
    jobs = []
    for s, i, o in reads:
        if not er[s, i]:
            jobs.append(([b + t[s, i]], [b + o], bytes([1]), 0))
            continue
        rows, _ = f.pattern_rows(er[s].tobytes())
        surv = f.pattern_survivors(er[s].tobytes())
        rank = int(er[s, :i].sum())
        jobs.append(([b + t[s, c] for c in surv], [b + o], bytes(rows[rank * k:(rank + 1) * k]), 0))
    f.combine(jobs, S)


@pytest.mark.parametrize("code,S,stripes", [("rs10_14", 5000, 5), ("rs64_80", 8208, 3), ("rs12_40", 4112, 3)])
def test_life_sequence(code, S, stripes):
    P, f = pool(code, S, stripes), fec(code)
    E = f.matrix()
    clean = np.full(stripes, CLEAN, dtype=np.uint32)

    def both(case, route, what):
        """The call on one pool, the rs_combine route it replaces on a second,
        identical one: the image after each, and the two byte for byte."""
        g, h = Gpu(f), Gpu(f)
        got = case.run(g)
        case.check(got, what)
        h.up(case.init, case.table)
        route(h)
        alt = h.down()
        case.check(alt, what + ", by rs_combine")
        assert np.array_equal(got[0], alt[0])
        return g, got[0]

    case = encode_case(P, 31)
    sc = case.sc
    g, arena = both(case, lambda h: combine_encode(f, E, h, sc, case.table, S, stripes), "encode")
    assert np.array_equal(g.verify(S, stripes), clean)
    case.check(g.down(), "verify")

    upd = update_case(P, 32, arena=arena, decoys=False)
    g, arena = both(upd, lambda h: combine_update(f, E, h, sc, upd.table, S, stripes, upd.args["updates"]), "update")

    er = erasures(P, 33)
    er[stripes - 1] = 0  # one stripe stays intact
    rd = read_case(P, 34, er, arena=arena)
    g, after = both(rd, lambda h: combine_read(f, h, rd.sc, rd.table, S, stripes, er, rd.args["reads"]), "read")
    lost = after[:rd.sc.pool_len]

    upd2 = update_case(P, 35, listed={stripes - 1: [0]}, arena=lost, entry_row=rd.sc.entry_row)
    g, arena2 = both(upd2, lambda h: combine_update(f, E, h, sc, upd2.table, S, stripes, upd2.args["updates"]),
                     "update of an intact stripe")

    # repair: the erased shards go back to their own rows; everything else stays
    want = arena2.copy()
    for s, i in zip(*np.nonzero(er)):
        want[sc.at(s, i):sc.at(s, i) + r16(S)] = arena[sc.at(s, i):sc.at(s, i) + r16(S)]
    table = P.table(0).reshape(-1)
    g = Gpu(f)
    tp = g.up(arena2, table)
    fb = torch.zeros(stripes, dtype=torch.int32, device="cuda:0")
    f.reconstruct_checked_ptrs(tp, S, stripes, er.tobytes(), fb.data_ptr())
    got = g.down()
    assert np.array_equal(fb.cpu().numpy().view(np.uint32), clean)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], table)
    assert np.array_equal(g.verify(S, stripes), clean)
    assert np.array_equal(g.down()[0], want)

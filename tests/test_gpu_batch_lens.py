"""GPU: rs_encode_batch_lens / rs_decode_batch_lens -- the batched host API
for messages of different lengths, one pass of the per-job-length combine
kernel per staging group -- and the host mirror that uses them.

Every expected byte comes from the oracle (oracle.encode, oracle.decode) or
from the message itself, never from the calls under test, and every
comparison is exact; rs_encode / rs_decode of the message alone must agree
too.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the RSMI_BATCH_STAGE_MB child of test_batch_lens_staging_groups_child
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "noise-erasurecode-plugin_amd"), os.path.join(_root, "tests")):
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
from oracle import oracle  # noqa: E402

# (k, m): RS(10,4), RS(4,2), RS(8,14), RS(64,16), RS(17,49), RS(1,2)
CODES = [(10, 4), (4, 2), (8, 14), (64, 16), (17, 49), (1, 2)]
# nothing | one byte | a column and a byte | one 4 KiB block chunk | a chunk and three bytes |
# odd | sixteen chunks and seven bytes | config 1's shard
SHARDS = [0, 1, 17, 4096, 4099, 6553, 65543, 104858]

DUMMY = b"\0" * 32  # where a share that is never read points
_FECS = {}


def fec(k, m):
    if (k, m) not in _FECS:
        _FECS[(k, m)] = rsmi.FEC(k, k + m, device=0)
    return _FECS[(k, m)]


class Message:
    """A message of k * S seeded bytes and its n shares by the oracle."""

    def __init__(self, k, m, S, seed):
        self.k, self.n, self.S = k, k + m, S
        self.data = oracle.splitmix_bytes(k * S, seed).tobytes() if S else b""
        self.parity = oracle.encode(oracle.fec_matrix(k, k + m), k, k + m, self.data) if S else b""
        self.shares = [self.data[i * S:(i + 1) * S] for i in range(k)] + [self.parity[i * S:(i + 1) * S] for i in range(m)]


_MESSAGES = {}


def messages(k, m):
    """One message per shard length of SHARDS, computed once per code."""
    if (k, m) not in _MESSAGES:
        _MESSAGES[(k, m)] = [Message(k, m, S, 1000 * k + 10 * m + i) for i, S in enumerate(SHARDS)]
    return _MESSAGES[(k, m)]


def addr(b):
    return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value


class Guarded:
    """An output buffer of `size` bytes between two 64-byte guard bands."""

    BAND = bytes(range(64, 128))

    def __init__(self, size):
        self.size = size
        self.buf = ctypes.create_string_buffer(self.BAND + b"\xA5" * size + self.BAND, 128 + size)
        self.ptr = ctypes.addressof(self.buf) + 64

    def result(self):
        """The output, once both bands are found intact."""
        raw = self.buf.raw
        assert raw[:64] == self.BAND and raw[64 + self.size:] == self.BAND, "a guard band was written"
        return raw[64:64 + self.size]


def encode_lens(f, inputs):
    """rs_encode_batch_lens of inputs = [bytes, or (None, length) for a NULL
    input]: (return code, parities, statuses)."""
    lib = rsmi.load()
    B, m = len(inputs), f.n - f.k
    keep = [x for x in inputs if isinstance(x, bytes)]
    ins = (ctypes.c_void_p * B)(*[addr(x) if isinstance(x, bytes) else None for x in inputs])
    lens = (ctypes.c_size_t * B)(*[len(x) if isinstance(x, bytes) else x[1] for x in inputs])
    outs = [Guarded(lens[b] // f.k * m) for b in range(B)]
    outp = (ctypes.c_void_p * B)(*[o.ptr for o in outs])
    st = (ctypes.c_int * B)(*[77] * B)
    rc = lib.rs_encode_batch_lens(f.handle, B, ins, lens, outp, st)
    del keep
    return rc, [o.result() for o in outs], list(st)


def decode_lens(f, msgs):
    """rs_decode_batch_lens of msgs = [(share length, [(number, address)],
    dst address or None)]: (return code, outputs, statuses, numbers and share
    addresses as the call left them)."""
    lib = rsmi.load()
    B = len(msgs)
    counts = (ctypes.c_int * B)(*[len(sh) for _, sh, _ in msgs])
    flat = [x for _, sh, _ in msgs for x in sh]
    nums = (ctypes.c_int * max(len(flat), 1))(*[num for num, _ in flat])
    ptrs = (ctypes.c_void_p * max(len(flat), 1))(*[p for _, p in flat])
    lens = (ctypes.c_size_t * B)(*[S for S, _, _ in msgs])
    outs = [Guarded(f.k * S) if dst is None else None for S, _, dst in msgs]
    dsts = (ctypes.c_void_p * B)(*[o.ptr if o is not None else dst for o, (_, _, dst) in zip(outs, msgs)])
    st = (ctypes.c_int * B)(*[77] * B)
    rc = lib.rs_decode_batch_lens(f.handle, B, counts, nums, ptrs, lens, dsts, st)
    res = [ctypes.string_at(dst, f.k * S) if o is None else o.result() for o, (S, _, dst) in zip(outs, msgs)]
    return rc, res, list(st), list(nums), list(ptrs)


def stats(f):
    return {name: f.stat(getattr(f, "STAT_" + name)) for name in
            ("BATCH_LENS_PASSES", "ENCODE_BATCHES", "BATCHES_STAGED", "BATCHES_IN_PLACE", "COMBINE_LENS_LAUNCHES")}


def delta(f, before):
    after = stats(f)
    return {name: after[name] - before[name] for name in before}


@pytest.mark.parametrize("k,m", CODES)
def test_encode_batch_lens_against_the_oracle(k, m):
    f = fec(k, m)
    msgs = messages(k, m)
    inputs = [x.data for x in msgs]
    # within the same batch: a NULL message and (where k allows one) a length that is no multiple of k
    inputs.insert(3, (None, k * 512))
    if k > 1:
        inputs.insert(6, b"\x01" * (k * 300 + 1))
    before = stats(f)
    rc, par, st = encode_lens(f, inputs)
    d = delta(f, before)
    assert d["BATCH_LENS_PASSES"] == 1 and d["ENCODE_BATCHES"] == 0 and d["COMBINE_LENS_LAUNCHES"] == 0
    want_st = [rsmi.RS_EINVAL if isinstance(x, tuple) else rsmi.RS_ELEN_NOT_MULTIPLE if len(x) % k else rsmi.RS_OK for x in inputs]
    assert st == want_st
    assert rc == rsmi.RS_EINVAL  # the first failing status in message order
    good = [p for p, x in zip(par, inputs) if isinstance(x, bytes) and len(x) % k == 0]
    for x, p in zip(msgs, good):
        assert p == x.parity, x.S
        assert p == f.encode_parity(x.data), x.S
    # the Python face of the call
    par2, st2 = f.EncodeBatchLens([x for x in inputs if isinstance(x, bytes)])
    assert [p for p in par2 if p is not None] == good
    assert [s for s in st2 if s] == ([rsmi.RS_ELEN_NOT_MULTIPLE] if k > 1 else [])


def subsets(msgs, seed):
    """A seeded k-subset of every message's shares, in shuffled order; every
    other message's is drawn without share 0, so that it has a data shard to
    regenerate whatever the draw (with k = 1 two draws in three have none)."""
    rng = np.random.default_rng(seed)
    return [[int(i) + (b + 1) % 2 for i in rng.permutation(x.n - (b + 1) % 2)[:x.k]] for b, x in enumerate(msgs)]


@pytest.mark.parametrize("k,m", CODES)
def test_decode_batch_lens_against_the_oracle(k, m):
    f = fec(k, m)
    n = k + m
    msgs = messages(k, m)
    E = oracle.fec_matrix(k, n)
    keep = subsets(msgs, seed=k * 100 + m)
    arena = rsmi.Arena(3 * sum((x.S + 255) // 256 * 256 * x.k for x in msgs) + 4096)  # the odd messages, then all
    batch = []
    for b, (x, ids) in enumerate(zip(msgs, keep)):
        in_arena = b % 2 == 1  # every other message has its shares in engine-pinned memory
        batch.append((x.S, [(i, (arena.put(x.shares[i]) if in_arena else addr(x.shares[i])) if x.S else addr(DUMMY)) for i in ids], None))
    # one message with k + 2 shares, one of them corrupted: the Correct path
    x = msgs[4]
    bad = bytearray(x.shares[1 % n])
    bad[7] ^= 0x40
    bad = bytes(bad)
    ids = list(range(k + 2))
    batch.insert(2, (x.S, [(i, addr(bad) if i == 1 % n else addr(x.shares[i])) for i in reversed(ids)], None))
    # one message with k - 1 shares, in front of everything: the call's return value
    y = msgs[3]
    batch.insert(0, (y.S, [(i, addr(y.shares[i])) for i in range(k - 1)], None))
    expect = [None, msgs[0].data, msgs[1].data, x.data] + [z.data for z in msgs[2:]]
    before = stats(f)
    rc, outs, st, nums, _ = decode_lens(f, batch)
    d = delta(f, before)
    assert rc == rsmi.RS_ENOT_ENOUGH and st == [rsmi.RS_ENOT_ENOUGH] + [rsmi.RS_OK] * (len(batch) - 1)
    for b, (got, want) in enumerate(zip(outs, expect)):
        if want is not None:
            assert got == want, b
    # against the oracle's decode of the same shares, and rs_decode of the message alone
    for x, ids in zip(msgs, keep):
        if x.S:
            rc2, ref = oracle.decode(E, k, n, [(i, x.shares[i]) for i in sorted(ids)])
            assert rc2 == 0 and ref == x.data
            assert f.Decode(None, [rsmi.Share(i, x.shares[i]) for i in ids]) == x.data
    # the caller's numbers come back sorted per message
    at = 0
    for S, sh, _ in batch:
        mine = nums[at:at + len(sh)]
        if len(sh) >= k:
            assert mine == sorted(num for num, _ in sh)
        at += len(sh)
    # one pass for the messages of exactly k shares; pageable and arena messages mixed: staged and in place
    assert d["BATCH_LENS_PASSES"] == 1 and d["BATCHES_STAGED"] == 1 and d["BATCHES_IN_PLACE"] == 0
    # all of them in the arena: a pass that stages nothing
    before = stats(f)
    allin = [(x.S, [(i, arena.put(x.shares[i])) for i in ids], None) for x, ids in zip(msgs, keep) if x.S]
    rc, outs, st, _, _ = decode_lens(f, allin)
    assert rc == 0 and outs == [x.data for x in msgs if x.S]
    d = delta(f, before)
    assert d["BATCH_LENS_PASSES"] == 1 and d["BATCHES_IN_PLACE"] == 1 and d["BATCHES_STAGED"] == 0
    arena.free()
    # the Python face of the call: shares sorted in place
    lists = [[rsmi.Share(i, x.shares[i]) for i in ids] for x, ids in zip(msgs, keep)]
    outs, st = f.DecodeBatchLens(lists)
    assert st == [0] * len(msgs) and outs == [x.data for x in msgs]
    assert all([s.Number for s in sh] == sorted(ids) for sh, ids in zip(lists, keep))


def test_decode_batch_lens_aliasing():
    """Message b's dst holds message b''s survivors, with different lengths;
    one dst holds its own message's shares."""
    k, m = 10, 4
    f = fec(k, m)
    S = [5000, 3000, 4099, 1000, 2000]
    msgs = [Message(k, m, s, 900 + i) for i, s in enumerate(S)]
    keep = subsets(msgs, seed=5)
    holder = {2: 0, 1: 2, 3: 1, 4: 4}  # message -> the message whose dst holds its survivors
    bufs = [ctypes.create_string_buffer(k * s) for s in S]
    base = [ctypes.addressof(b) for b in bufs]
    extra = {}
    batch = []
    for b, (x, ids) in enumerate(zip(msgs, keep)):
        sh = []
        for slot, i in enumerate(ids):
            if b in holder:
                p = base[holder[b]] + slot * x.S
                ctypes.memmove(p, x.shares[i], x.S)
            else:
                extra[(b, i)] = x.shares[i]
                p = addr(extra[(b, i)])
            sh.append((i, p))
        batch.append((x.S, sh, base[b]))
    rc, outs, st, nums, ptrs = decode_lens(f, batch)
    assert rc == 0 and st == [0] * len(S)
    assert outs == [x.data for x in msgs]
    # the caller's arrays: sorted by number, every pointer the caller's own
    at = 0
    for _, sh, _ in batch:
        assert list(zip(nums[at:at + k], ptrs[at:at + k])) == sorted(sh)
        at += k


def test_batch_lens_pass_through():
    """One length for every message that is left to code: the equal-length
    pass and its counters; one such message: no batched pass of either kind."""
    k, m = 10, 4
    f = fec(k, m)
    same = [Message(k, m, 4099, 300 + i) for i in range(5)]
    keep = subsets(same, seed=9)
    before = stats(f)
    rc, par, st = encode_lens(f, [x.data for x in same] + [b"", b"\x02" * 11])  # an empty and a failing message beside them
    assert rc == rsmi.RS_ELEN_NOT_MULTIPLE and st == [0] * 6 + [rsmi.RS_ELEN_NOT_MULTIPLE]
    assert par[:5] == [x.parity for x in same]
    d = delta(f, before)
    assert d["ENCODE_BATCHES"] == 1 and d["BATCH_LENS_PASSES"] == 0
    before = stats(f)
    batch = [(x.S, [(i, addr(x.shares[i])) for i in ids], None) for x, ids in zip(same, keep)]
    rc, outs, st, _, _ = decode_lens(f, batch + [(0, [(i, addr(DUMMY)) for i in range(k)], None)])
    assert rc == 0 and outs[:5] == [x.data for x in same]
    d = delta(f, before)
    assert d["BATCHES_STAGED"] == 1 and d["BATCH_LENS_PASSES"] == 0
    # exactly one message to code
    before = stats(f)
    rc, par, st = encode_lens(f, [b"", same[0].data, (None, 10 * k), b"\x03" * (k + 1)])
    assert st == [0, 0, rsmi.RS_EINVAL, rsmi.RS_ELEN_NOT_MULTIPLE] and par[1] == same[0].parity
    rc, outs, st, _, _ = decode_lens(f, [batch[0], (17, [(i, addr(DUMMY)) for i in range(k - 1)], None)])
    assert st == [0, rsmi.RS_ENOT_ENOUGH] and rc == rsmi.RS_ENOT_ENOUGH and outs[0] == same[0].data
    d = delta(f, before)
    assert d["ENCODE_BATCHES"] == 0 and d["BATCHES_STAGED"] == 0 and d["BATCHES_IN_PLACE"] == 0 and d["BATCH_LENS_PASSES"] == 0


def check_staging_groups(f, k, m):
    """40 messages with seeded shard lengths between 4 KiB and 200 KiB; with a
    2 MiB staging cap they go in several groups."""
    rng = np.random.default_rng(41)
    msgs = [Message(k, m, int(s), 7000 + i) for i, s in enumerate(rng.integers(4096, 200 * 1024 + 1, size=40))]
    inputs = [x.data for x in msgs]
    inputs[30] = inputs[30] + b"\x01"        # fails alone, in a late group
    inputs[35] = (None, k * 4096)
    before = stats(f)
    rc, par, st = encode_lens(f, inputs)
    d = delta(f, before)
    assert rc == rsmi.RS_ELEN_NOT_MULTIPLE  # the first failing status across the groups
    assert st == [rsmi.RS_ELEN_NOT_MULTIPLE if b == 30 else rsmi.RS_EINVAL if b == 35 else 0 for b in range(40)]
    assert all(p == x.parity for b, (p, x) in enumerate(zip(par, msgs)) if b not in (30, 35))
    assert d["BATCH_LENS_PASSES"] >= 2 and d["ENCODE_BATCHES"] == 0
    keep = subsets(msgs, seed=42)
    batch = [(x.S, [(i, addr(x.shares[i])) for i in ids], None) for x, ids in zip(msgs, keep)]
    batch[25] = (msgs[25].S, batch[25][1][:k - 1], None)
    batch[33] = (msgs[33].S, [(k + m, p) for _, p in batch[33][1]], None)  # a share number outside [0, n)
    before = stats(f)
    rc, outs, st, _, _ = decode_lens(f, batch)
    d = delta(f, before)
    assert rc == rsmi.RS_ENOT_ENOUGH
    assert st == [rsmi.RS_ENOT_ENOUGH if b == 25 else rsmi.RS_EBAD_SHARE_ID if b == 33 else 0 for b in range(40)]
    assert all(o == x.data for b, (o, x) in enumerate(zip(outs, msgs)) if b not in (25, 33))
    assert d["BATCH_LENS_PASSES"] >= 2


def test_batch_lens_staging_groups_child():
    """RSMI_BATCH_STAGE_MB is read once per process: a child with a 2 MiB cap."""
    env = dict(os.environ, RSMI_BATCH_STAGE_MB="2")
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "staging child ok" in run.stdout


def test_batch_lens_device_set():
    """A {0, 0} device set: contiguous message ranges balanced by bytes, a
    pass on each member."""
    k, m = 10, 4
    fs = rsmi.FEC(k, k + m, devices=[0, 0])
    msgs = [x for x in messages(k, m) if x.S] + [Message(k, m, s, 50 + s) for s in (70000, 33, 50000, 90001)]
    before = [fs.member(i).stat(fs.STAT_BATCH_LENS_PASSES) for i in range(2)]
    rc, par, st = encode_lens(fs, [x.data for x in msgs])
    assert rc == 0 and par == [x.parity for x in msgs]
    mid = [fs.member(i).stat(fs.STAT_BATCH_LENS_PASSES) for i in range(2)]
    assert all(b > a for a, b in zip(before, mid))
    keep = subsets(msgs, seed=3)
    rc, outs, st, _, _ = decode_lens(fs, [(x.S, [(i, addr(x.shares[i])) for i in ids], None) for x, ids in zip(msgs, keep)])
    assert rc == 0 and outs == [x.data for x in msgs]
    after = [fs.member(i).stat(fs.STAT_BATCH_LENS_PASSES) for i in range(2)]
    assert all(b > a for a, b in zip(mid, after))
    assert fs.stat(fs.STAT_BATCH_LENS_PASSES) == sum(after)
    fs.close()


def test_plugin_batches_messages_of_different_lengths():
    """The host mirror: prepareShardsBatch of 40 inputs of 40 lengths makes
    prepareShards' shards through the mixed-length pass, and ReceiveBatch
    decodes and verifies shards of messages of different lengths."""
    import hashlib

    from rsmi import host as h
    k, n = 10, 14
    me = h.PeerID("127.0.0.1:3000", b"self")

    def sign(digest):
        return hashlib.blake2b(b"signed:" + digest, digest_size=32).digest()

    def verify(digest, sig):
        return sig == sign(digest)

    p = h.NewShardPlugin(sign, verify, k, n, hash_len=32)
    inputs = [oracle.splitmix_bytes(10 * (100 + 37 * i), 60 + i).tobytes() for i in range(40)] + [b"abc"]
    cached = h.CachedFEC(k, n)
    passes0 = cached.Stat(rsmi.FEC.STAT_BATCH_LENS_PASSES)
    out, codes = p.prepareShardsBatch(me, inputs)
    assert cached.Stat(rsmi.FEC.STAT_BATCH_LENS_PASSES) - passes0 >= 1
    assert codes[-1] != 0 and all(c == 0 for c in codes[:-1])  # len % k != 0 -> Encode error
    E = oracle.fec_matrix(k, n)
    for inp, shards in zip(inputs[:-1], out[:-1]):
        assert shards == p.prepareShards(me, inp)
        assert b"".join(s.ShardData for s in shards[k:]) == oracle.encode(E, k, n, inp)
    # the receive side: every message loses up to 3 shards; the arrivals are interleaved
    rng = np.random.default_rng(8)
    arrivals = []
    for shards in out[:-1]:
        lost = rng.choice(n, size=int(rng.integers(0, 4)), replace=False)
        arrivals += [(me, shards[i]) for i in range(n) if i not in lost]
    arrivals = [arrivals[i] for i in rng.permutation(len(arrivals))]
    recv = h.NewShardPlugin(sign, verify, k, n, hash_len=32)
    passes0 = cached.Stat(rsmi.FEC.STAT_BATCH_LENS_PASSES)
    evs, codes = recv.ReceiveBatch(arrivals)
    assert all(c == 0 for c in codes)
    done = [e for e in evs if e.decoded]
    assert len(done) == 40 and all(e.verified for e in done)
    assert sorted(e.message for e in done) == sorted(inputs[:-1])
    assert cached.Stat(rsmi.FEC.STAT_BATCH_LENS_PASSES) - passes0 >= 1
    # ... as Receive, one arrival at a time, decodes them
    seq = h.NewShardPlugin(sign, verify, k, n, hash_len=32)
    for (s, sh), e in zip(arrivals, evs):
        one = seq.Receive(s, sh)
        assert (one.pooled, one.decoded, one.verified, one.message) == (e.pooled, e.decoded, e.verified, e.message)
    # the host FEC's face of the encode call
    got = cached.EncodeBatchLens(inputs)
    assert got[-1] is None and got[:-1] == [oracle.encode(E, k, n, x) for x in inputs[:-1]]


if __name__ == "__main__":
    assert os.environ.get("RSMI_BATCH_STAGE_MB") == "2"
    check_staging_groups(fec(4, 2), 4, 2)
    print("staging child ok")

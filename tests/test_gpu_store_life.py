"""GPU: the device-resident calls in sequence -- the life of a store -- against
the byte-exact host model of store_model.py.

The engine and the model are driven through the same seeded scenario
(store_model.Driver): fill and encode, update, lose shards, degraded read and
update, damage, degraded verify, checked repair, column scrub, repair again,
shard-level scrub, reconstruct, verify, and then twelve further ops drawn from
those whose preconditions hold.  Nothing is set up afresh between two calls:
the stripes, the pool of source / destination rows and the first_bad rows
live in device buffers for the whole run, and at every checkpoint the WHOLE
image -- guards, pitch padding, stride gaps, decoy rows, garbage-filled erased
slots -- is compared with the model's bytes, which come from the bytes that
are stored and never from the pristine payload.

Every scenario runs twice from one seed: "every" synchronises and compares
after each op; "async" queues all enqueue-and-return calls back to back on
one non-default stream and compares only where a synchronous call or the end
of the run forces it, so a failure in "async" alone points at the lifetime of
a job table or a lease.  test_store_model.py proves the driver, the scenarios
and the ledger on the CPU first.

The scenarios of store_model_io.py run beside those of store_model.py:
placement "ptrs_io" (rs_encode_ptrs, rs_update_ptrs and rs_read_ptrs, the last
two over a per-call table whose never-loaded entries name decoy rows),
placement "ptrs_lens" (a shard length per stripe: the three _lens calls, and
one call per run of equal lengths for everything else), and on all of them
and a second set of strided ones a checksum table kept up to date through the
whole life, with the check and the repair by checksum among the ops.

test_ledger must run after the scenarios of this file (it reads their
counters): run the file whole.
"""
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import rsmi  # noqa: E402
import store_model as sm  # noqa: E402
import store_model_io as io  # noqa: E402

SCENARIOS = sm.scenarios() + io.scenarios_io()
BY_ID = {x[0]: x for x in SCENARIOS}
GRANS = ("every", "async")
# the same scenarios on a device set, and RS(64,16) under its two A/B knobs
SET_CODES = ((10, 14), (13, 18))
KNOBS = (("RSMI_REPAIR_FUSED", "0"), ("RSMI_SMALL_SPLIT", "0"))

_FECS = {}
RAN = set()
TIMES = {}


def fec(k, n, context="plain"):
    """One context per (code, context).  The knobs are read when a context is created."""
    key = (k, n, context)
    if key not in _FECS:
        if context == "plain":
            _FECS[key] = rsmi.FEC(k, n, device=0)
        elif context == "set":
            _FECS[key] = rsmi.FEC(k, n, devices=[0, 0])
        else:
            name, value = context
            old = os.environ.get(name)
            os.environ[name] = value
            try:
                _FECS[key] = rsmi.FEC(k, n, device=0)
            finally:
                del os.environ[name]
                if old is not None:
                    os.environ[name] = old
    return _FECS[key]


class GpuEngine:
    """The rsmi.FEC binding on torch device buffers, behind the interface of
    store_model.HostEngine.  Every call goes to one stream: the default one,
    or a stream of the run's own.  The driver's host-side writes (garbage,
    damage, new contents) are uploaded on a side stream and applied in stream
    order by a device copy, so they synchronise nothing.  ENQUEUED lists the
    calls that are given stream=: the enqueue-and-return ones, and the
    synchronous scrubs and repairs (correct_*), which take a stream as well."""

    ENQUEUED = ("encode_stripes", "verify_stripes", "verify_degraded", "verify_ptrs", "reconstruct_stripes",
                "reconstruct_ptrs", "reconstruct_checked", "reconstruct_checked_ptrs", "update_stripes",
                "update_degraded", "read_stripes", "combine", "correct_stripes", "correct_degraded",
                "correct_columns", "correct_columns_ptrs", "encode_ptrs", "update_ptrs", "read_ptrs",
                "verify_ptrs_lens", "reconstruct_checked_ptrs_lens", "correct_columns_ptrs_lens", "crc32c_stripes",
                "crc32c_check_stripes", "crc32c_ptrs", "crc32c_check_ptrs", "correct_crc32c")

    def __init__(self, f, arrays, own_stream):
        self.f = f
        self.stream = torch.cuda.Stream() if own_stream else torch.cuda.default_stream()
        self.side = torch.cuda.Stream()
        self.dev = [torch.from_numpy(a.copy()).cuda() for a in arrays]
        self.bases = [d.data_ptr() for d in self.dev]
        assert all(b % 256 == 0 for b in self.bases)
        self.keep = []
        torch.cuda.synchronize()

    def adr(self, buf, off):
        return self.bases[buf] + off

    def __getattr__(self, name):
        if name in self.ENQUEUED:
            fn, s = getattr(self.f, name), self.stream.cuda_stream
            return lambda *a, **kw: fn(*a, stream=s, **kw)
        if name in ("pattern_rows", "pattern_survivors"):
            return getattr(self.f, name)
        raise AttributeError(name)

    def _upload(self, data):
        with torch.cuda.stream(self.side):
            t = torch.from_numpy(np.ascontiguousarray(data, dtype=np.uint8).copy()).cuda()
        self.side.synchronize()
        self.keep.append(t)
        return t

    def poke(self, buf, off, data):
        t = self._upload(data)
        with torch.cuda.stream(self.stream):
            self.dev[buf][off:off + len(data)].copy_(t)

    def xor(self, buf, off, data):
        t = self._upload(data)
        with torch.cuda.stream(self.stream):
            self.dev[buf][off:off + len(data)].bitwise_xor_(t)

    def sync(self):
        self.f.sync(self.stream.cuda_stream)
        torch.cuda.synchronize()

    def snapshot(self):
        return [d.cpu().numpy() for d in self.dev]


def life(ident, gran, context="plain"):
    k, n = BY_ID[ident][1:3]
    f = fec(k, n, context)
    t0 = time.perf_counter()
    io.driver(lambda k, n, names, arrays: GpuEngine(f, arrays, own_stream=gran == "async"),
              BY_ID[ident], gran, (ident, gran, context)).run()
    TIMES[(ident, gran, context)] = time.perf_counter() - t0
    print(f"{ident} {gran} {context}: {TIMES[(ident, gran, context)]:.2f} s")
    RAN.add((ident, gran, context))


@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("ident", [x[0] for x in SCENARIOS])
def test_store_life(ident, gran):
    life(ident, gran)


@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("ident", [x[0] for x in SCENARIOS
                                   if (x[1], x[2]) in SET_CODES and not x[0].startswith("seed")])
def test_store_life_device_set(ident, gran):
    """The same scenarios on rsmi.FEC(k, n, devices=[0, 0])."""
    life(ident, gran, "set")


@pytest.mark.parametrize("gran", GRANS)
@pytest.mark.parametrize("knob", KNOBS, ids=[f"{a}={b}" for a, b in KNOBS])
@pytest.mark.parametrize("ident", [x[0] for x in SCENARIOS if (x[1], x[2]) == (64, 80)])
def test_store_life_knobs(ident, knob, gran):
    """RS(64,16) once more with the two launches in the checked repair's
    place, and with small calls kept on the bit-sliced kernels."""
    life(ident, gran, knob)


STATS = ("STAT_REC_STRIPES_TABLE", "STAT_REC_STRIPES_SYNDROME", "STAT_REPAIR_CHECKED", "STAT_CHECK_STRIPES",
         "STAT_COLUMN_STRIPES", "STAT_COLUMN_BYTES", "STAT_UPDATE_STRIPES", "STAT_UPDATE_COPY_COMMITS",
         "STAT_UPDATE_DEGRADED", "STAT_UPDATE_ABSORBED", "STAT_READ_REGENERATED", "STAT_READ_COPIED",
         "STAT_COMBINE_JOBS", "STAT_SCRUB_REGENERATED", "STAT_CRC_SECTORS", "STAT_CRC_REGENERATED",
         "STAT_SCRUB_LENS_LAUNCHES", "STAT_COLUMN_LENS_LAUNCHES")


def test_ledger():
    """The walk cannot quietly skip what it exists to test: every scenario of
    this file ran, every op kind the header defines for its code ran in it
    (the refusal of rs_correct_columns for m > 16 included), every damage step
    damaged a stripe, the engine's own counters moved (the contexts are this
    file's, so their counters started at zero), RS(64,20) is served by the
    K64 / MG16 variants and RS(64,16) on the pointer placement by the twins.
    For the scenarios of store_model_io.py also what check_ledger_io lists:
    the new op kinds ran, no encode, plain update or read of "ptrs_io" and
    "ptrs_lens" went through rs_combine, slices, decoys and regenerated reads
    happened, mixed, equal and empty lengths reached every _lens call, the
    repair by checksum repaired beyond the codeword radius and refused a
    codeword of other data."""
    want = ({(x[0], g, "plain") for x in SCENARIOS for g in GRANS} |
            {(x[0], g, "set") for x in SCENARIOS for g in GRANS
             if (x[1], x[2]) in SET_CODES and not x[0].startswith("seed")} |
            {(x[0], g, kn) for x in SCENARIOS for g in GRANS for kn in KNOBS if (x[1], x[2]) == (64, 80)})
    assert want <= RAN, sorted(want - RAN, key=str)
    for ident, gran, context in sorted(want, key=str):
        _, k, n, _, stripes, placement = BY_ID[ident][:6]
        if len(BY_ID[ident]) == 7:
            sm.check_ledger((ident, gran, context), k, n, stripes, placement == "ptrs")
        else:
            io.check_ledger_io((ident, gran, context), BY_ID[ident])
    total = {name: sum(f.stat(getattr(f, name)) for f in _FECS.values()) for name in STATS}
    print(total)
    assert all(v > 0 for v in total.values()), total
    f = fec(64, 84)
    names = [f.kernel_name(0), f.kernel_name(2)]   # rs_kernel_name: which = 0 encode, which = 2 verify
    print(names)
    assert all("K64" in x and "MG16" in x for x in names), names
    # RS(12,40) ran "ptrs_io" only: its updates and reads are those of the pointer calls
    f = fec(12, 40)
    only = {name: f.stat(getattr(f, name)) for name in ("STAT_UPDATE_STRIPES", "STAT_READ_REGENERATED",
                                                        "STAT_READ_COPIED")}
    assert {x[5] for x in SCENARIOS if (x[1], x[2]) == (12, 40)} == {"ptrs_io"} and all(only.values()), only
    f = fec(64, 80)
    names = [f.kernel_name(20), f.kernel_name(21), f.kernel_name(22)]
    print(names)
    assert names == ["bitslice_k64_m16_ptrs", "update_MG16_B256_ptrs", "read_K64_MG4_B256_ptrs"], names
    slow = max(TIMES, key=TIMES.get)
    print(f"slowest case {slow}: {TIMES[slow]:.2f} s; all cases {sum(TIMES.values()):.1f} s")

"""CPU: the planner of rs_combine (csrc/combine_plan.cpp, rsmi::plan_combine)
and the parts of the binding that need no GPU.

The planner checks run in a stand-alone C++ program (its own main) built from
csrc/combine_plan.cpp with -fsanitize=address,undefined and run directly."""
import ctypes
import os
import subprocess

from conftest import PKG
from test_capi_symbols import HEADERS, header_functions

CSRC = os.path.join(PKG, "csrc")

PROGRAM = r"""
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "combine_plan.hpp"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<uint32_t>((z ^ (z >> 31)) >> 16);
}

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++failures;                                   \
            std::printf("FAIL %s:%d: ", #cond, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

// A job that owns its host arrays.
struct Job {
    std::vector<uint64_t> src, dst;
    std::vector<uint8_t> coef;
    uint32_t accumulate = 0, reserved = 0;
};
static Job job(std::vector<uint64_t> src, std::vector<uint64_t> dst, uint32_t accumulate = 0) {
    Job j;
    j.src = std::move(src);
    j.dst = std::move(dst);
    j.coef.resize(j.src.size() * j.dst.size());
    for (uint8_t& c : j.coef) c = static_cast<uint8_t>(rnd());
    j.accumulate = accumulate;
    return j;
}
static std::vector<rs_combine_job> view(const std::vector<Job>& jobs) {
    std::vector<rs_combine_job> v;
    for (const Job& j : jobs) {
        rs_combine_job c{};
        c.src = j.src.data();
        c.dst = j.dst.data();
        c.coef = j.coef.data();
        c.nsrc = static_cast<uint32_t>(j.src.size());
        c.nout = static_cast<uint32_t>(j.dst.size());
        c.accumulate = j.accumulate;
        c.reserved = j.reserved;
        v.push_back(c);
    }
    return v;
}

static bool empty(const rsmi::CombinePlan& p) {
    return p.jobs.empty() && p.addrs.empty() && p.coef.empty() && p.max_nsrc == 0 && p.max_nout == 0 && p.rows == 0;
}
static void stale(rsmi::CombinePlan* p) {  // contents that must not survive a refusal
    p->jobs.push_back(rsmi::CombineJob{0, 0, 1, 1, 0});
    p->addrs.push_back(16);
    p->coef.push_back(1);
    p->max_nsrc = p->max_nout = 9;
    p->rows = 3;
}

// The plan, expanded, is exactly the jobs given.
static void expands(const char* what, const std::vector<Job>& jobs, size_t len) {
    const std::vector<rs_combine_job> v = view(jobs);
    rsmi::CombinePlan p;
    stale(&p);
    const int rc = rsmi::plan_combine(v.data(), v.size(), len, &p);
    CHECK(rc == RS_OK, "%s: status %d", what, rc);
    if (rc != RS_OK) return;
    CHECK(p.jobs.size() == jobs.size(), "%s: %zu jobs for %zu", what, p.jobs.size(), jobs.size());
    if (p.jobs.size() != jobs.size()) return;
    uint64_t addr = 0, coef = 0, rows = 0;
    uint32_t max_nsrc = 0, max_nout = 0;
    for (size_t b = 0; b < jobs.size(); ++b) {
        const rsmi::CombineJob& j = p.jobs[b];
        const Job& w = jobs[b];
        CHECK(j.addr == addr && j.coef == coef, "%s: job %zu tables at %u / %u, not %llu / %llu", what, b, j.addr, j.coef,
              (unsigned long long)addr, (unsigned long long)coef);
        CHECK(j.nsrc == w.src.size() && j.nout == w.dst.size() && j.accumulate == w.accumulate, "%s: job %zu shape", what, b);
        if (j.addr + static_cast<uint64_t>(j.nsrc) + j.nout > p.addrs.size() ||
            j.coef + static_cast<uint64_t>(j.nsrc) * j.nout > p.coef.size()) {
            CHECK(false, "%s: job %zu runs past its tables", what, b);
            return;
        }
        CHECK(std::equal(w.src.begin(), w.src.end(), p.addrs.begin() + j.addr), "%s: job %zu sources", what, b);
        CHECK(std::equal(w.dst.begin(), w.dst.end(), p.addrs.begin() + j.addr + j.nsrc), "%s: job %zu destinations", what, b);
        CHECK(std::equal(w.coef.begin(), w.coef.end(), p.coef.begin() + j.coef), "%s: job %zu coefficients", what, b);
        addr += w.src.size() + w.dst.size();
        coef += w.coef.size();
        rows += w.dst.size();
        max_nsrc = std::max<uint32_t>(max_nsrc, w.src.size());
        max_nout = std::max<uint32_t>(max_nout, w.dst.size());
    }
    CHECK(p.addrs.size() == addr && p.coef.size() == coef, "%s: table sizes", what);
    CHECK(p.rows == rows && p.max_nsrc == max_nsrc && p.max_nout == max_nout, "%s: rows %llu, max %u x %u", what,
          (unsigned long long)p.rows, p.max_nout, p.max_nsrc);
}

static void refused(const char* what, const std::vector<Job>& jobs, size_t len) {
    const std::vector<rs_combine_job> v = view(jobs);
    rsmi::CombinePlan p;
    stale(&p);
    const int rc = rsmi::plan_combine(v.data(), v.size(), len, &p);
    CHECK(rc == RS_EINVAL, "%s: status %d, want %d", what, rc, RS_EINVAL);
    CHECK(empty(p), "%s: plan not empty", what);
}
static void refused_raw(const char* what, const rs_combine_job* jobs, size_t count, size_t len) {
    rsmi::CombinePlan p;
    stale(&p);
    const int rc = rsmi::plan_combine(jobs, count, len, &p);
    CHECK(rc == RS_EINVAL, "%s: status %d, want %d", what, rc, RS_EINVAL);
    CHECK(empty(p), "%s: plan not empty", what);
}

int main() {
    const size_t len = 1000, span = 1008;  // round_up(len, 16)
    const uint64_t A = 0x100000, B = 0x200000, D = 0x800000;

    // shapes at the limits, mixed modes, shared and repeated sources
    expands("one job", {job({A}, {D})}, len);
    expands("limits", {job(std::vector<uint64_t>(256, A), {D}, 1)}, len);
    {
        std::vector<uint64_t> src, dst;
        for (uint64_t i = 0; i < 256; ++i) src.push_back(A + 16 * i), dst.push_back(D + span * i);
        expands("256 x 256", {job(src, dst)}, len);
    }
    expands("mixed", {job({A, B}, {D, D + span}, 1), job({A, A + 16, A}, {D + 2 * span}), job({B}, {D + 5 * span, D + 3 * span}, 1)},
            len);

    // nothing to do: RS_OK and an empty plan, whatever the pointers
    {
        rsmi::CombinePlan p;
        stale(&p);
        CHECK(rsmi::plan_combine(nullptr, 0, len, &p) == RS_OK && empty(p), "count == 0");
        rs_combine_job bad{};
        bad.nsrc = 999;
        stale(&p);
        CHECK(rsmi::plan_combine(&bad, 0, len, &p) == RS_OK && empty(p), "count == 0 reads no job");
        stale(&p);
        CHECK(rsmi::plan_combine(&bad, 1, 0, &p) == RS_OK && empty(p), "len == 0 reads no job");
    }

    // refusals, each leaving the plan empty
    {
        refused_raw("NULL jobs", nullptr, 1, len);
        const Job good = job({A, B}, {D});
        const std::vector<Job> goods = {good};
        const std::vector<rs_combine_job> v = view(goods);
        refused_raw("count == 2^32", v.data(), size_t(1) << 32, len);
        // 2^28 or more 16-byte columns, as the stripe calls (buffers 2^40 apart: no overlap at that length)
        const std::vector<Job> fars = {job({16}, {1ull << 40})};
        const std::vector<rs_combine_job> far = view(fars);
        refused_raw("len of 2^28 columns", far.data(), 1, (size_t(1) << 32));
        refused_raw("len of 2^28 columns, less 15", far.data(), 1, (size_t(1) << 32) - 15);
        rsmi::CombinePlan p;
        CHECK(rsmi::plan_combine(far.data(), 1, (size_t(1) << 32) - 16, &p) == RS_OK, "len of 2^28 - 1 columns");
        rs_combine_job j = v[0];
        j.src = nullptr;
        refused_raw("NULL src", &j, 1, len);
        j = v[0], j.dst = nullptr;
        refused_raw("NULL dst", &j, 1, len);
        j = v[0], j.coef = nullptr;
        refused_raw("NULL coef", &j, 1, len);
        j = v[0], j.nsrc = 0;
        refused_raw("nsrc == 0", &j, 1, len);
        j = v[0], j.nout = 0;
        refused_raw("nout == 0", &j, 1, len);
        j = v[0], j.nsrc = 257;  // refused before src[256] is read
        refused_raw("nsrc == 257", &j, 1, len);
        j = v[0], j.nout = 257;
        refused_raw("nout == 257", &j, 1, len);
        j = v[0], j.accumulate = 2;
        refused_raw("accumulate == 2", &j, 1, len);
        j = v[0], j.reserved = 1;
        refused_raw("reserved", &j, 1, len);
        refused("NULL source address", {job({A, 0}, {D})}, len);
        refused("NULL destination address", {job({A}, {D, 0})}, len);
        refused("misaligned source", {job({A + 8}, {D})}, len);
        refused("misaligned destination", {job({A}, {D + 1})}, len);
        refused("second job bad", {good, job({A}, {D + span + 4})}, len);
    }

    // the overlap rule at its edges
    {
        // destinations that touch at round_up(len, 16) are accepted, one byte closer (16: alignment) refused
        expands("dst touch dst", {job({A}, {D, D + span})}, len);
        refused("dst meets dst", {job({A}, {D, D + span - 16})}, len);
        refused("dst twice", {job({A}, {D, D})}, len);
        refused("dst meets dst of another job", {job({A}, {D + span - 16}), job({B}, {D})}, len);
        expands("dst touch dst of another job", {job({A}, {D + span}), job({B}, {D})}, len);
        // a source next to a destination, on either side
        expands("src touches dst from below", {job({D - span}, {D})}, len);
        expands("src touches dst from above", {job({D + span}, {D})}, len);
        refused("src shares the dst's first 16 bytes", {job({D - span + 16}, {D})}, len);
        refused("src shares the dst's last 16 bytes", {job({D + span - 16}, {D})}, len);
        refused("src is dst", {job({D}, {D})}, len);
        // the padding counts: [len, round_up(len, 16)) of a dst is written
        refused("src starts in the dst's padding", {job({D + 992}, {D})}, len);
        // a dst meeting a src of a different job, either order
        refused("dst meets an earlier job's src", {job({A}, {D}), job({B}, {A + 16})}, len);
        refused("dst meets a later job's src", {job({A}, {D}), job({D + 32}, {B})}, len);
        // with len = 16 neighbours 16 bytes apart are disjoint
        expands("len 16", {job({A, A + 16}, {A + 32, A + 48})}, 16);
        refused("len 17", {job({A, A + 16}, {A + 32, A + 48})}, 17);
        // sources repeat and overlap freely, within a job and across jobs
        expands("repeated sources", {job({A, A, A + 16, A + 16}, {D}), job({A, A + 32}, {D + span}, 1)}, len);
    }

    // fixed-seed sweep: disjoint destinations carved from one region in shuffled order, sources from another
    for (int rep = 0; rep < 100; ++rep) {
        const size_t l = 1 + rnd() % 5000, sp = (l + 15) / 16 * 16;
        std::vector<uint64_t> slots;
        for (uint64_t i = 0; i < 600; ++i) slots.push_back(D + i * sp);
        for (size_t i = slots.size() - 1; i > 0; --i) std::swap(slots[i], slots[rnd() % (i + 1)]);
        std::vector<Job> jobs;
        size_t used = 0;
        const size_t count = 1 + rnd() % 12;
        for (size_t b = 0; b < count; ++b) {
            const size_t nsrc = 1 + rnd() % 40, nout = 1 + rnd() % 40;
            std::vector<uint64_t> src, dst;
            for (size_t i = 0; i < nsrc; ++i) src.push_back(A + 16ull * (rnd() % 1000));
            for (size_t i = 0; i < nout; ++i) dst.push_back(slots[used++]);
            jobs.push_back(job(src, dst, rnd() & 1));
        }
        expands("sweep", jobs, l);
        // one more job whose source lies in a destination of the first
        jobs.push_back(job({jobs[0].dst.back() + (sp > 16 ? 16 : 0)}, {slots[used]}));
        refused("sweep, poisoned", jobs, l);
    }

    // 10^5 jobs: the overlap check sorts, it does not compare every pair (5 x 10^9 pairs for these)
    {
        std::vector<Job> jobs;
        for (uint64_t b = 0; b < 100000; ++b)
            jobs.push_back(job({A + 16 * (b % 1000), A + 16 * ((7 * b) % 1000)}, {D + ((b * 48271) % 100000) * span}, b & 1));
        const std::vector<rs_combine_job> v = view(jobs);
        rsmi::CombinePlan p;
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = rsmi::plan_combine(v.data(), v.size(), len, &p);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        CHECK(rc == RS_OK && p.jobs.size() == 100000 && p.rows == 100000, "10^5 jobs: status %d", rc);
        CHECK(ms < 1000.0, "10^5 jobs planned in %.0f ms", ms);
        std::printf("10^5 jobs planned in %.1f ms\n", ms);
        jobs[77777].dst[0] = jobs[3].dst[0] + 16;
        refused("10^5 jobs, two destinations meet", jobs, len);
    }
    std::printf("plan_combine: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_combine_standalone_sanitized(tmp_path):
    src = tmp_path / "combine_plan_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "combine_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "combine_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_combine: 0 failures" in run.stdout


def test_combine_entry_points_are_exported():
    import rsmi
    assert "rs_combine" in rsmi.EXPORTS and "rs_pattern_survivors" in rsmi.EXPORTS
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    assert hasattr(lib, "rs_combine") and hasattr(lib, "rs_pattern_survivors")
    assert sorted(rsmi.EXPORTS) == header_functions(HEADERS[:1])
    assert ctypes.sizeof(rsmi.CombineJob) == 40
    assert (rsmi.FEC.STAT_COMBINE_JOBS, rsmi.FEC.STAT_COMBINE_ROWS) == (18, 19)


def test_combine_jobs_helper_keeps_its_arrays():
    import rsmi
    arr = rsmi.combine_jobs([([16, 32], [64], b"\x01\x02", 0), ([16], [96, 128, 160], bytes([3, 0, 1]), 1)])
    assert arr._count == 2
    assert (arr[0].nsrc, arr[0].nout, arr[0].accumulate, arr[0].reserved) == (2, 1, 0, 0)
    assert (arr[1].nsrc, arr[1].nout, arr[1].accumulate) == (1, 3, 1)
    assert [arr[0].src[i] for i in range(2)] == [16, 32] and arr[0].dst[0] == 64
    assert [arr[1].dst[i] for i in range(3)] == [96, 128, 160]
    assert [arr[0].coef[i] for i in range(2)] == [1, 2] and [arr[1].coef[i] for i in range(3)] == [3, 0, 1]


def test_null_context_is_rejected_without_a_device():
    """rs_combine and rs_pattern_survivors refuse a NULL context with
    RS_EINVAL before touching HIP; callable on a CPU-only machine."""
    import rsmi
    lib = rsmi.load()
    arr = rsmi.combine_jobs([([16], [32], b"\x01", 0)])
    assert lib.rs_combine(None, arr, 1, 16, None) == rsmi.RS_EINVAL
    assert lib.rs_combine(None, None, 0, 16, None) == rsmi.RS_EINVAL
    assert lib.rs_combine(None, arr, 1, 0, None) == rsmi.RS_EINVAL
    ids = (ctypes.c_int * 4)()
    assert lib.rs_pattern_survivors(None, None, ids) == rsmi.RS_EINVAL

"""CPU: the planner of rs_update_stripes (csrc/update_plan.cpp,
rsmi::plan_updates) and the parts of the binding that need no GPU.

The planner checks run in a stand-alone C++ program (its own main) built from
csrc/update_plan.cpp with -fsanitize=address,undefined and run directly."""
import ctypes
import os
import subprocess

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "update_plan.hpp"

static uint64_t rng_state = 0x13198A2E03707344ull;
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

static const void* addr(uint64_t a) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(a)); }
static rs_shard_update upd(uint64_t stripe, uint32_t shard, uint64_t src) {
    rs_shard_update u{};
    u.stripe = stripe;
    u.shard = shard;
    u.src = addr(src);
    return u;
}

using Triple = std::tuple<uint64_t, uint32_t, uint64_t>;  // stripe, shard, src

// The plan's structure, and its jobs expanded back to (stripe, shard, src).
static std::vector<Triple> expand(const rsmi::UpdatePlan& p, const char* what) {
    std::vector<Triple> out;
    uint32_t next = 0, max_j = 0;
    for (size_t b = 0; b < p.jobs.size(); ++b) {
        const rsmi::UpdateJob& job = p.jobs[b];
        CHECK(job.j >= 1, "%s: empty job %zu", what, b);
        CHECK(job.first == next, "%s: job %zu starts at %u, not %u", what, b, job.first, next);
        if (b) CHECK(p.jobs[b - 1].stripe < job.stripe, "%s: jobs not in strictly increasing stripe order at %zu", what, b);
        if (static_cast<size_t>(job.first) + job.j > p.entries.size()) {
            CHECK(false, "%s: job %zu runs past the entry table", what, b);
            return out;
        }
        for (uint32_t i = job.first; i < job.first + job.j; ++i) {
            CHECK(p.entries[i].pad == 0, "%s: entry %u pad", what, i);
            out.emplace_back(job.stripe, p.entries[i].shard, p.entries[i].src);
        }
        next = job.first + job.j;
        max_j = std::max(max_j, job.j);
    }
    CHECK(next == p.entries.size(), "%s: %zu entries, jobs cover %u", what, p.entries.size(), next);
    CHECK(max_j == p.max_j, "%s: max_j %u, jobs say %u", what, p.max_j, max_j);
    return out;
}

static void refused(const char* what, int k, size_t stripes, const std::vector<rs_shard_update>& u, int want) {
    rsmi::UpdatePlan p;
    p.jobs.push_back(rsmi::UpdateJob{7, 0, 1});  // stale contents must not survive a refusal
    p.max_j = 9;
    const int rc = rsmi::plan_updates(k, stripes, u.data(), u.size(), &p);
    CHECK(rc == want, "%s: status %d, want %d", what, rc, want);
    CHECK(p.jobs.empty() && p.entries.empty() && p.max_j == 0, "%s: plan not empty", what);
}

int main() {
    // shuffled entries of three stripes, interleaved
    {
        const std::vector<rs_shard_update> u = {upd(5, 3, 0x1000), upd(0, 9, 0x2000), upd(5, 0, 0x3000), upd(2, 4, 0x4000),
                                                upd(0, 1, 0x5000), upd(5, 7, 0x6000)};
        rsmi::UpdatePlan p;
        CHECK(rsmi::plan_updates(10, 6, u.data(), u.size(), &p) == RS_OK, "grouping");
        CHECK(p.jobs.size() == 3 && p.entries.size() == 6 && p.max_j == 3, "grouping: %zu jobs, %zu entries, max_j %u",
              p.jobs.size(), p.entries.size(), p.max_j);
        const std::vector<Triple> got = expand(p, "grouping");
        const std::vector<Triple> want = {{0, 1, 0x5000}, {0, 9, 0x2000}, {2, 4, 0x4000},
                                          {5, 0, 0x3000}, {5, 3, 0x1000}, {5, 7, 0x6000}};
        CHECK(got == want, "grouping: wrong jobs");
        if (p.jobs.size() == 3) {
            CHECK(p.jobs[0].stripe == 0 && p.jobs[0].j == 2, "job 0");
            CHECK(p.jobs[1].stripe == 2 && p.jobs[1].j == 1, "job 1");
            CHECK(p.jobs[2].stripe == 5 && p.jobs[2].j == 3, "job 2");
        }
    }
    // one entry; j = k in one stripe
    {
        rsmi::UpdatePlan p;
        const rs_shard_update one = upd(36, 9, 0x10);
        CHECK(rsmi::plan_updates(10, 37, &one, 1, &p) == RS_OK && p.jobs.size() == 1 && p.max_j == 1, "one entry");
        std::vector<rs_shard_update> all;
        for (uint32_t i = 0; i < 10; ++i) all.push_back(upd(1, 9 - i, 0x100 + 16 * i));
        CHECK(rsmi::plan_updates(10, 2, all.data(), all.size(), &p) == RS_OK && p.jobs.size() == 1 && p.max_j == 10, "j = k");
        expand(p, "j = k");
    }
    // count == 0: RS_OK and an empty plan, whatever the pointer
    {
        rsmi::UpdatePlan p;
        p.max_j = 3;
        CHECK(rsmi::plan_updates(10, 4, nullptr, 0, &p) == RS_OK && p.jobs.empty() && p.entries.empty() && p.max_j == 0,
              "count == 0");
        const rs_shard_update bad = upd(99, 99, 1);
        CHECK(rsmi::plan_updates(10, 4, &bad, 0, &p) == RS_OK && p.jobs.empty(), "count == 0 reads no entry");
    }
    // refusals
    {
        rsmi::UpdatePlan p;
        CHECK(rsmi::plan_updates(10, 4, nullptr, 1, &p) == RS_EINVAL, "NULL updates");
        refused("shard == k", 10, 4, {upd(0, 1, 0x10), upd(1, 10, 0x20)}, RS_EBAD_SHARE_ID);
        refused("stripe == stripes", 10, 4, {upd(4, 1, 0x10)}, RS_EINVAL);
        refused("stripe far out", 10, 4, {upd(~0ull, 1, 0x10)}, RS_EINVAL);
        refused("duplicate", 10, 4, {upd(3, 2, 0x10), upd(1, 2, 0x20), upd(3, 2, 0x30)}, RS_EINVAL);
        refused("duplicate, same src", 10, 4, {upd(3, 2, 0x10), upd(3, 2, 0x10)}, RS_EINVAL);
        refused("NULL src", 10, 4, {upd(0, 0, 0)}, RS_EINVAL);
        refused("misaligned src", 10, 4, {upd(0, 0, 0x18)}, RS_EINVAL);
        refused("misaligned src, odd", 10, 4, {upd(0, 0, 0x1001)}, RS_EINVAL);
        rs_shard_update r = upd(0, 0, 0x10);
        r.reserved = 1;
        refused("reserved", 10, 4, {r}, RS_EINVAL);
        // the same shard id in different stripes is no duplicate
        const std::vector<rs_shard_update> ok = {upd(0, 2, 0x10), upd(1, 2, 0x10)};
        CHECK(rsmi::plan_updates(10, 4, ok.data(), ok.size(), &p) == RS_OK && p.jobs.size() == 2, "same shard, two stripes");
    }
    // fixed-seed sweep: the jobs, expanded, are the input set
    for (int rep = 0; rep < 200; ++rep) {
        const int k = 1 + static_cast<int>(rnd() % 64);
        const size_t stripes = 1 + rnd() % 50;
        std::set<std::pair<uint64_t, uint32_t>> seen;
        std::vector<rs_shard_update> u;
        std::vector<Triple> want;
        const size_t count = rnd() % (2 * stripes + 1);
        for (size_t i = 0; i < count; ++i) {
            const uint64_t s = rnd() % stripes;
            const uint32_t sh = rnd() % static_cast<uint32_t>(k);
            if (!seen.insert({s, sh}).second) continue;
            const uint64_t src = 16ull * (1 + rnd());
            u.push_back(upd(s, sh, src));
            want.emplace_back(s, sh, src);
        }
        rsmi::UpdatePlan p;
        const int rc = rsmi::plan_updates(k, stripes, u.data(), u.size(), &p);
        CHECK(rc == RS_OK, "sweep %d: status %d", rep, rc);
        std::vector<Triple> got = expand(p, "sweep");
        CHECK(std::is_sorted(got.begin(), got.end()), "sweep %d: not in (stripe, shard) order", rep);
        std::sort(want.begin(), want.end());
        CHECK(got == want, "sweep %d: jobs do not expand to the input", rep);
        std::set<uint64_t> distinct;
        for (const Triple& t : want) distinct.insert(std::get<0>(t));
        CHECK(p.jobs.size() == distinct.size(), "sweep %d: %zu jobs for %zu stripes", rep, p.jobs.size(), distinct.size());
    }
    std::printf("plan_updates: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_updates_standalone_sanitized(tmp_path):
    src = tmp_path / "update_plan_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "update_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "update_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_updates: 0 failures" in run.stdout


def test_update_entry_point_is_exported():
    import rsmi
    assert "rs_update_stripes" in rsmi.EXPORTS
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    assert hasattr(lib, "rs_update_stripes")
    assert ctypes.sizeof(rsmi.ShardUpdate) == 24
    assert (rsmi.FEC.STAT_UPDATE_STRIPES, rsmi.FEC.STAT_UPDATE_COPY_COMMITS) == (12, 13)


def test_null_context_is_rejected_without_a_device():
    """rs_update_stripes refuses a NULL context with RS_EINVAL before
    touching HIP; callable on a CPU-only machine."""
    import rsmi
    lib = rsmi.load()
    one = (rsmi.ShardUpdate * 1)(rsmi.ShardUpdate(0, 0, 0, 16))
    assert lib.rs_update_stripes(None, None, 0, None, 0, 16, 16, 1, one, 1, None) == rsmi.RS_EINVAL
    assert lib.rs_update_stripes(None, None, 0, None, 0, 16, 16, 1, None, 0, None) == rsmi.RS_EINVAL

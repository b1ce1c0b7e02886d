"""CPU: the planner of rs_read_stripes (csrc/read_plan.cpp, rsmi::plan_reads)
and the parts of the binding that need no GPU.

The planner checks run in a stand-alone C++ program (its own main) built from
csrc/read_plan.cpp with -fsanitize=address,undefined and run directly."""
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

#include "read_plan.hpp"

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

static rs_shard_read rd(uint64_t stripe, uint32_t shard, uint64_t dst) {
    rs_shard_read r{};
    r.stripe = stripe;
    r.shard = shard;
    r.dst = reinterpret_cast<void*>(static_cast<uintptr_t>(dst));
    return r;
}

using Triple = std::tuple<uint64_t, uint32_t, uint64_t>;  // stripe, shard, dst

// erased[stripes][n] with the listed (stripe, shard) pairs set.
static std::vector<uint8_t> flags(size_t stripes, int n, const std::vector<std::pair<size_t, int>>& gone) {
    std::vector<uint8_t> f(stripes * n, 0);
    for (const auto& g : gone) f[g.first * n + g.second] = 1;
    return f;
}

// Brute force: the number of erased ids below `shard`.
static uint32_t rank_of(const uint8_t* fl, uint32_t shard) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < shard; ++i) r += fl[i] != 0;
    return r;
}

// The plan's structure against the flags, and the plan expanded back to
// (stripe, shard, dst): a job's entry of row r is the r-th erased id.
static std::vector<Triple> expand(const rsmi::ReadPlan& p, int n, const std::vector<uint8_t>& er, const char* what) {
    std::vector<Triple> out;
    uint32_t next = 0, max_j = 0;
    CHECK(p.erased.size() == p.jobs.size() * static_cast<size_t>(n), "%s: %zu compact flags for %zu jobs", what,
          p.erased.size(), p.jobs.size());
    if (p.erased.size() != p.jobs.size() * static_cast<size_t>(n)) return out;
    for (size_t b = 0; b < p.jobs.size(); ++b) {
        const rsmi::ReadJob& job = p.jobs[b];
        const uint8_t* fl = er.data() + job.stripe * n;
        CHECK(job.j >= 1, "%s: empty job %zu", what, b);
        CHECK(job.first == next, "%s: job %zu starts at %u, not %u", what, b, job.first, next);
        if (b) CHECK(p.jobs[b - 1].stripe < job.stripe, "%s: jobs not in strictly increasing stripe order at %zu", what, b);
        for (int i = 0; i < n; ++i)
            CHECK(p.erased[b * n + i] == (fl[i] ? 1 : 0), "%s: compact flag %d of job %zu", what, i, b);
        if (static_cast<size_t>(job.first) + job.j > p.entries.size()) {
            CHECK(false, "%s: job %zu runs past the entry table", what, b);
            return out;
        }
        std::vector<uint32_t> ids;  // erased ids in increasing order
        for (int i = 0; i < n; ++i)
            if (fl[i]) ids.push_back(static_cast<uint32_t>(i));
        for (uint32_t i = job.first; i < job.first + job.j; ++i) {
            const rsmi::ReadEntry& e = p.entries[i];
            CHECK(e.pad == 0, "%s: entry %u pad", what, i);
            if (i > job.first) CHECK(p.entries[i - 1].row < e.row, "%s: entry %u not in row order", what, i);
            if (e.row >= ids.size()) {
                CHECK(false, "%s: entry %u row %u of %zu erasures", what, i, e.row, ids.size());
                continue;
            }
            CHECK(e.row == rank_of(fl, ids[e.row]), "%s: rank", what);
            out.emplace_back(job.stripe, ids[e.row], e.dst);
        }
        next = job.first + job.j;
        max_j = std::max(max_j, job.j);
    }
    CHECK(next == p.entries.size(), "%s: %zu entries, jobs cover %u", what, p.entries.size(), next);
    CHECK(max_j == p.max_j, "%s: max_j %u, jobs say %u", what, p.max_j, max_j);
    for (size_t i = 0; i < p.copies.size(); ++i) {
        const rsmi::ReadCopy& c = p.copies[i];
        CHECK(c.pad == 0 && c.shard < static_cast<uint32_t>(n), "%s: copy %zu", what, i);
        CHECK(er[c.stripe * n + c.shard] == 0, "%s: copy %zu of an erased shard", what, i);
        out.emplace_back(c.stripe, c.shard, c.dst);
    }
    return out;
}

static void refused(const char* what, int k, int n, size_t stripes, const std::vector<uint8_t>& er, size_t bytes,
                    const std::vector<rs_shard_read>& r, int want) {
    rsmi::ReadPlan p;
    p.jobs.push_back(rsmi::ReadJob{7, 0, 1});  // stale contents must not survive a refusal
    p.copies.push_back(rsmi::ReadCopy{1, 1, 0, 16});
    p.erased.assign(3, 1);
    p.max_j = 9;
    const int rc = rsmi::plan_reads(k, n, stripes, er.data(), bytes, r.data(), r.size(), &p);
    CHECK(rc == want, "%s: status %d, want %d", what, rc, want);
    CHECK(p.jobs.empty() && p.entries.empty() && p.copies.empty() && p.erased.empty() && p.max_j == 0,
          "%s: plan not empty", what);
}

int main() {
    const int k = 10, n = 14;
    // shuffled entries of four stripes, interleaved: missing data, missing
    // parity, present data, present parity
    {
        // stripe 0: 1, 9, 12 gone | stripe 2: 4 gone | stripe 3: nothing gone | stripe 5: 0, 3, 7, 13 gone
        const std::vector<uint8_t> er = flags(6, n, {{0, 1}, {0, 9}, {0, 12}, {2, 4}, {5, 0}, {5, 3}, {5, 7}, {5, 13}});
        const std::vector<rs_shard_read> r = {rd(5, 7, 0x1000),  rd(0, 12, 0x2000), rd(5, 0, 0x3000), rd(2, 4, 0x4000),
                                              rd(0, 1, 0x5000),  rd(5, 13, 0x6000), rd(0, 2, 0x7000), rd(3, 11, 0x8000),
                                              rd(5, 12, 0x9000), rd(2, 3, 0xA000)};
        rsmi::ReadPlan p;
        CHECK(rsmi::plan_reads(k, n, 6, er.data(), 0x1000, r.data(), r.size(), &p) == RS_OK, "grouping");
        CHECK(p.jobs.size() == 3 && p.entries.size() == 6 && p.copies.size() == 4 && p.max_j == 3,
              "grouping: %zu jobs, %zu entries, %zu copies, max_j %u", p.jobs.size(), p.entries.size(), p.copies.size(),
              p.max_j);
        if (p.jobs.size() == 3 && p.entries.size() == 6) {
            CHECK(p.jobs[0].stripe == 0 && p.jobs[0].j == 2, "job 0");
            CHECK(p.jobs[1].stripe == 2 && p.jobs[1].j == 1, "job 1");
            CHECK(p.jobs[2].stripe == 5 && p.jobs[2].j == 3, "job 2");
            // stripe 0 wants ids 1 (rank 0) and 12 (rank 2); stripe 5 wants 0, 7, 13 (ranks 0, 2, 3)
            const uint32_t rows[6] = {0, 2, 0, 0, 2, 3};
            const uint64_t dsts[6] = {0x5000, 0x2000, 0x4000, 0x3000, 0x1000, 0x6000};
            for (int i = 0; i < 6; ++i)
                CHECK(p.entries[i].row == rows[i] && p.entries[i].dst == dsts[i], "entry %d: row %u dst %llx", i,
                      p.entries[i].row, static_cast<unsigned long long>(p.entries[i].dst));
        }
        std::vector<Triple> got = expand(p, n, er, "grouping");
        std::vector<Triple> want;
        for (const rs_shard_read& x : r) want.emplace_back(x.stripe, x.shard, reinterpret_cast<uintptr_t>(x.dst));
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        CHECK(got == want, "grouping: the plan does not expand to the input");
        // present entries are copies in (stripe, shard) order
        if (p.copies.size() == 4) {
            const Triple c[4] = {{0, 2, 0x7000}, {2, 3, 0xA000}, {3, 11, 0x8000}, {5, 12, 0x9000}};
            for (int i = 0; i < 4; ++i)
                CHECK(Triple(p.copies[i].stripe, p.copies[i].shard, p.copies[i].dst) == c[i], "copy %d", i);
        }
    }
    // a stripe with more than m erasures that wants present shards only is
    // served; unlisted stripes may be flagged fully erased
    {
        std::vector<uint8_t> er(4 * n, 1);  // everything erased ...
        for (int i = 0; i < n; ++i) er[1 * n + i] = i < 5;  // ... but stripe 1: five erasures, ids 0..4
        for (int i = 0; i < n; ++i) er[2 * n + i] = i == 13;
        const std::vector<rs_shard_read> r = {rd(1, 9, 0x100), rd(2, 13, 0x200), rd(1, 5, 0x300)};
        rsmi::ReadPlan p;
        CHECK(rsmi::plan_reads(k, n, 4, er.data(), 0x100, r.data(), r.size(), &p) == RS_OK, "present only");
        CHECK(p.jobs.size() == 1 && p.jobs[0].stripe == 2 && p.copies.size() == 2 && p.entries.size() == 1 &&
                  p.entries[0].row == 0,
              "present only: %zu jobs, %zu copies", p.jobs.size(), p.copies.size());
        expand(p, n, er, "present only");
        // the same stripe wanting one of its erased shards: not enough
        refused("five erasures, one wanted", k, n, 4, er, 0x100, {rd(1, 9, 0x100), rd(1, 4, 0x200)}, RS_ENOT_ENOUGH);
        // a later stripe's refusal drops the jobs planned before it
        refused("not enough, after a good job", k, n, 4, er, 0x100, {rd(2, 13, 0x100), rd(3, 0, 0x200)}, RS_ENOT_ENOUGH);
        // exactly m erasures are enough
        for (int i = 0; i < n; ++i) er[3 * n + i] = i >= 10;
        CHECK(rsmi::plan_reads(k, n, 4, er.data(), 0x100, r.data(), 2, &p) == RS_OK, "m erasures");
        const rs_shard_read four = rd(3, 12, 0x100);
        CHECK(rsmi::plan_reads(k, n, 4, er.data(), 0x100, &four, 1, &p) == RS_OK && p.jobs.size() == 1 &&
                  p.entries[0].row == 2,
              "m erasures, parity wanted");
    }
    // count == 0: RS_OK and an empty plan, whatever the pointers
    {
        rsmi::ReadPlan p;
        p.max_j = 3;
        CHECK(rsmi::plan_reads(k, n, 4, nullptr, 16, nullptr, 0, &p) == RS_OK && p.jobs.empty() && p.entries.empty() &&
                  p.copies.empty() && p.max_j == 0,
              "count == 0");
    }
    // k == n: copies only; an erased shard cannot be computed
    {
        const std::vector<uint8_t> er = flags(2, 6, {{1, 2}});
        const std::vector<rs_shard_read> r = {rd(1, 5, 0x100), rd(0, 0, 0x200)};
        rsmi::ReadPlan p;
        CHECK(rsmi::plan_reads(6, 6, 2, er.data(), 0x100, r.data(), r.size(), &p) == RS_OK && p.jobs.empty() &&
                  p.copies.size() == 2,
              "k == n");
        refused("k == n, erased wanted", 6, 6, 2, er, 0x100, {rd(1, 2, 0x100)}, RS_ENOT_ENOUGH);
    }
    // refusals
    {
        const std::vector<uint8_t> er = flags(4, n, {{0, 1}, {3, 2}});
        rsmi::ReadPlan p;
        const rs_shard_read one = rd(0, 1, 0x100);
        CHECK(rsmi::plan_reads(k, n, 4, er.data(), 16, nullptr, 1, &p) == RS_EINVAL, "NULL reads");
        CHECK(rsmi::plan_reads(k, n, 4, nullptr, 16, &one, 1, &p) == RS_EINVAL, "NULL erased");
        refused("shard == n", k, n, 4, er, 16, {rd(0, 1, 0x100), rd(1, 14, 0x200)}, RS_EBAD_SHARE_ID);
        refused("stripe == stripes", k, n, 4, er, 16, {rd(4, 1, 0x100)}, RS_EINVAL);
        refused("stripe far out", k, n, 4, er, 16, {rd(~0ull, 1, 0x100)}, RS_EINVAL);
        refused("duplicate", k, n, 4, er, 16, {rd(3, 2, 0x100), rd(1, 2, 0x200), rd(3, 2, 0x300)}, RS_EINVAL);
        refused("duplicate present", k, n, 4, er, 16, {rd(1, 2, 0x100), rd(1, 2, 0x200)}, RS_EINVAL);
        refused("NULL dst", k, n, 4, er, 16, {rd(0, 0, 0)}, RS_EINVAL);
        refused("misaligned dst", k, n, 4, er, 16, {rd(0, 0, 0x108)}, RS_EINVAL);
        refused("misaligned dst, odd", k, n, 4, er, 16, {rd(0, 0, 0x1001)}, RS_EINVAL);
        rs_shard_read r = rd(0, 0, 0x100);
        r.reserved = 1;
        refused("reserved", k, n, 4, er, 16, {r}, RS_EINVAL);
        // dst ranges: equal, overlapping by one column, in either list order; touching ranges are fine
        refused("same dst", k, n, 4, er, 0x40, {rd(0, 1, 0x100), rd(1, 1, 0x100)}, RS_EINVAL);
        refused("dst overlap", k, n, 4, er, 0x40, {rd(0, 1, 0x100), rd(2, 5, 0x400), rd(1, 1, 0x130)}, RS_EINVAL);
        refused("dst overlap, descending", k, n, 4, er, 0x40, {rd(0, 1, 0x130), rd(2, 5, 0x400), rd(1, 1, 0x100)}, RS_EINVAL);
        const std::vector<rs_shard_read> touch = {rd(0, 1, 0x140), rd(1, 1, 0x100), rd(2, 5, 0x180)};
        CHECK(rsmi::plan_reads(k, n, 4, er.data(), 0x40, touch.data(), touch.size(), &p) == RS_OK, "touching dst ranges");
        // list defects come before any erasure count: stripe 2 has five erasures and wants one of them
        std::vector<uint8_t> er5 = er;
        for (int i = 0; i < 5; ++i) er5[2 * n + i] = 1;
        refused("not enough", k, n, 4, er5, 16, {rd(2, 0, 0x100)}, RS_ENOT_ENOUGH);
        refused("defect before not enough", k, n, 4, er5, 16, {rd(2, 0, 0x100), rd(3, 14, 0x200)}, RS_EBAD_SHARE_ID);
        refused("duplicate before not enough", k, n, 4, er5, 16, {rd(2, 0, 0x100), rd(0, 3, 0x200), rd(0, 3, 0x300)}, RS_EINVAL);
        refused("overlap before not enough", k, n, 4, er5, 32, {rd(2, 0, 0x100), rd(0, 3, 0x110)}, RS_EINVAL);
        // the same shard id in different stripes is no duplicate
        const std::vector<rs_shard_read> ok = {rd(0, 2, 0x100), rd(1, 2, 0x200)};
        CHECK(rsmi::plan_reads(k, n, 4, er.data(), 16, ok.data(), ok.size(), &p) == RS_OK && p.copies.size() == 2,
              "same shard, two stripes");
    }
    // fixed-seed sweep: the plan, expanded, is the input multiset
    for (int rep = 0; rep < 200; ++rep) {
        const int kk = 1 + static_cast<int>(rnd() % 64);
        const int nn = kk + static_cast<int>(rnd() % 20);
        const int mm = nn - kk;
        const size_t stripes = 1 + rnd() % 50;
        std::vector<uint8_t> er(stripes * nn, 0);
        std::vector<bool> over(stripes, false);  // more than m erasures (or junk flags): only present shards are wanted
        for (size_t s = 0; s < stripes; ++s) {
            const uint32_t kind = rnd() % 8;
            int e = mm ? static_cast<int>(rnd() % (mm + 1)) : 0;
            if (kind == 0) {
                e = std::min(nn - 1, mm + 1 + static_cast<int>(rnd() % 3));
                over[s] = e > mm;
            }
            for (int placed = 0; placed < e;) {
                const uint32_t id = rnd() % nn;
                if (!er[s * nn + id]) er[s * nn + id] = static_cast<uint8_t>(1 + rnd() % 255), ++placed;
            }
        }
        std::set<std::pair<uint64_t, uint32_t>> seen;
        std::vector<rs_shard_read> r;
        std::vector<Triple> want;
        std::set<uint64_t> job_stripes;
        const size_t count = rnd() % (3 * stripes + 1);
        uint64_t dst = 0x1000;
        for (size_t i = 0; i < count; ++i) {
            const uint64_t s = rnd() % stripes;
            const uint32_t sh = rnd() % static_cast<uint32_t>(nn);
            if (over[s] && er[s * nn + sh]) continue;
            if (!seen.insert({s, sh}).second) continue;
            dst += 0x40 + 16ull * (rnd() % 4);
            r.push_back(rd(s, sh, dst));
            want.emplace_back(s, sh, dst);
            if (er[s * nn + sh]) job_stripes.insert(s);
        }
        for (size_t i = r.size(); i > 1; --i) std::swap(r[i - 1], r[rnd() % i]);
        rsmi::ReadPlan p;
        const int rc = rsmi::plan_reads(kk, nn, stripes, er.data(), 0x40, r.data(), r.size(), &p);
        CHECK(rc == RS_OK, "sweep %d: status %d", rep, rc);
        std::vector<Triple> got = expand(p, nn, er, "sweep");
        std::sort(got.begin(), got.end());
        std::sort(want.begin(), want.end());
        CHECK(got == want, "sweep %d: the plan does not expand to the input", rep);
        CHECK(p.jobs.size() == job_stripes.size(), "sweep %d: %zu jobs for %zu stripes", rep, p.jobs.size(),
              job_stripes.size());
    }
    std::printf("plan_reads: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_reads_standalone_sanitized(tmp_path):
    src = tmp_path / "read_plan_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "read_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "read_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_reads: 0 failures" in run.stdout


def test_read_entry_point_is_exported():
    import rsmi
    assert "rs_read_stripes" in rsmi.EXPORTS
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    assert hasattr(lib, "rs_read_stripes")
    assert ctypes.sizeof(rsmi.ShardRead) == 24
    assert (rsmi.FEC.STAT_READ_REGENERATED, rsmi.FEC.STAT_READ_COPIED) == (14, 15)


def test_null_context_is_rejected_without_a_device():
    """rs_read_stripes refuses a NULL context with RS_EINVAL before touching
    HIP; callable on a CPU-only machine."""
    import rsmi
    lib = rsmi.load()
    one = (rsmi.ShardRead * 1)(rsmi.ShardRead(0, 0, 0, 16))
    flags = ctypes.create_string_buffer(14)
    fp = ctypes.cast(flags, ctypes.c_void_p)
    assert lib.rs_read_stripes(None, None, 0, None, 0, 16, 16, 1, fp, one, 1, None) == rsmi.RS_EINVAL
    assert lib.rs_read_stripes(None, None, 0, None, 0, 16, 16, 1, None, None, 0, None) == rsmi.RS_EINVAL

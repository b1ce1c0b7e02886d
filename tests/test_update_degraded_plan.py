"""CPU: the planner of rs_update_degraded (csrc/update_degraded_plan.cpp,
rsmi::plan_update_degraded) and the parts of the binding that need no GPU.

The planner checks run in a stand-alone C++ program (its own main) built from
csrc/update_degraded_plan.cpp and csrc/update_plan.cpp with
-fsanitize=address,undefined and run directly."""
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
#include <vector>

#include "update_degraded_plan.hpp"

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

static const void* addr(uint64_t a) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(a)); }
static rs_shard_update upd(uint64_t stripe, uint32_t shard, uint64_t src) {
    rs_shard_update u{};
    u.stripe = stripe;
    u.shard = shard;
    u.src = addr(src);
    return u;
}

using rsmi::UpdateDegradedPlan;

static bool empty(const UpdateDegradedPlan& p) {
    return p.jobs.empty() && p.entries.empty() && p.rows.empty() && p.erased.empty() && p.decode_jobs == 0 &&
           p.max_j == 0 && p.max_src == 0 && p.absorbed == 0 && !p.degraded;
}

// The plan's structure against a model computed from the flags directly.
static void check_plan(const UpdateDegradedPlan& p, int k, int n, const std::vector<uint8_t>& fl,
                       const std::vector<rs_shard_update>& u, const char* what) {
    const int m = n - k;
    std::set<uint64_t> listed;
    for (const rs_shard_update& x : u) listed.insert(x.stripe);
    CHECK(p.jobs.size() == listed.size(), "%s: %zu jobs for %zu stripes", what, p.jobs.size(), listed.size());
    uint32_t next = 0, next_row = 0, max_j = 0, max_src = 0, decode = 0;
    uint64_t absorbed = 0;
    bool degraded = false;
    std::vector<uint8_t> flags;
    for (size_t b = 0; b < p.jobs.size(); ++b) {
        const rsmi::DegJob& job = p.jobs[b];
        if (b) CHECK(p.jobs[b - 1].stripe < job.stripe, "%s: jobs not in stripe order at %zu", what, b);
        CHECK(job.first == next && job.row_first == next_row, "%s: job %zu starts at %u / %u", what, b, job.first,
              job.row_first);
        CHECK(job.j >= 1 && job.jx <= job.j, "%s: job %zu j %u jx %u", what, b, job.j, job.jx);
        CHECK(job.pat == rsmi::kDegNoPattern, "%s: job %zu pat", what, b);
        if (static_cast<size_t>(job.first) + job.j > p.entries.size() ||
            static_cast<size_t>(job.row_first) + job.nrows > p.rows.size()) {
            CHECK(false, "%s: job %zu runs past a table", what, b);
            return;
        }
        const uint8_t* f = &fl[job.stripe * n];
        // the model: this stripe's entries in shard order, split
        std::vector<std::pair<uint32_t, uint64_t>> mine, present, gone;
        for (const rs_shard_update& x : u)
            if (x.stripe == job.stripe) mine.push_back({x.shard, reinterpret_cast<uintptr_t>(x.src)});
        std::sort(mine.begin(), mine.end());
        for (const auto& e : mine) (f[e.first] ? gone : present).push_back(e);
        CHECK(job.j == mine.size() && job.jx == gone.size(), "%s: job %zu split %u / %u", what, b, job.j, job.jx);
        for (size_t i = 0; i < present.size() && i < job.j; ++i) {
            const rsmi::DegEntry& e = p.entries[job.first + i];
            CHECK(e.shard == present[i].first && e.src == present[i].second && e.rank == rsmi::kDegPresent && e.old == 0,
                  "%s: job %zu present entry %zu", what, b, i);
        }
        for (size_t i = 0; i < gone.size() && present.size() + i < job.j; ++i) {
            const rsmi::DegEntry& e = p.entries[job.first + present.size() + i];
            uint32_t rank = 0;
            for (uint32_t id = 0; id < gone[i].first; ++id) rank += f[id] != 0;
            CHECK(e.shard == gone[i].first && e.src == gone[i].second && e.rank == rank && e.old == 0,
                  "%s: job %zu erased entry %zu: shard %u rank %u, want %u rank %u", what, b, i, e.shard, e.rank,
                  gone[i].first, rank);
        }
        std::vector<uint32_t> rows;
        int e_all = 0;
        for (int id = 0; id < n; ++id) e_all += f[id] != 0;
        for (int r = 0; r < m; ++r)
            if (!f[k + r]) rows.push_back(r);
        CHECK(job.nrows == rows.size() && std::equal(rows.begin(), rows.end(), p.rows.begin() + job.row_first),
              "%s: job %zu present rows", what, b);
        if (job.jx > 0) {
            CHECK(e_all <= m, "%s: job %zu planned a decode with %d erasures", what, b, e_all);
            for (int id = 0; id < n; ++id) flags.push_back(f[id] ? 1 : 0);
            ++decode;
            absorbed += job.jx;
        }
        degraded |= e_all > 0;
        max_j = std::max(max_j, job.j);
        max_src = std::max(max_src, job.jx ? k + job.j : job.j);
        next = job.first + job.j;
        next_row = job.row_first + job.nrows;
    }
    CHECK(next == p.entries.size() && next_row == p.rows.size(), "%s: tables not covered", what);
    CHECK(p.max_j == max_j && p.max_src == max_src, "%s: max_j %u / %u, max_src %u / %u", what, p.max_j, max_j,
          p.max_src, max_src);
    CHECK(p.decode_jobs == decode && p.absorbed == absorbed && p.degraded == degraded, "%s: totals", what);
    CHECK(p.erased == flags, "%s: pattern flags", what);
}

static void refused(const char* what, int k, int n, size_t stripes, const std::vector<uint8_t>& fl,
                    const std::vector<rs_shard_update>& u, int want, const rsmi::UpdateExtent* ext = nullptr) {
    UpdateDegradedPlan p;
    p.jobs.push_back(rsmi::DegJob{7, 0, 1, 1, 0, 2, 3});  // stale contents must not survive a refusal
    p.entries.push_back(rsmi::DegEntry{16, 0, 1, 0});
    p.rows.push_back(1);
    p.erased.push_back(1);
    p.decode_jobs = 1;
    p.max_j = 9;
    p.max_src = 19;
    p.absorbed = 4;
    p.degraded = true;
    const int rc = rsmi::plan_update_degraded(k, n, stripes, fl.data(), u.data(), u.size(), ext, &p);
    CHECK(rc == want, "%s: status %d, want %d", what, rc, want);
    CHECK(empty(p), "%s: plan not empty", what);
}

int main() {
    const int k = 10, n = 14;
    // Six stripes; stripe 3 is never listed and holds garbage flags.
    std::vector<uint8_t> fl(6 * n, 0);
    std::fill(fl.begin() + 3 * n, fl.begin() + 4 * n, uint8_t(0xFF));
    fl[1 * n + 11] = 1;                                       // stripe 1: a parity shard
    fl[2 * n + 4] = 7;                                        // stripe 2: the changed shard (any non-zero value)
    fl[4 * n + 2] = fl[4 * n + 6] = fl[4 * n + 10] = fl[4 * n + 13] = 1;  // stripe 4: e = m
    for (int id : {0, 1, 2, 11, 12}) fl[5 * n + id] = 1;      // stripe 5: e = 5 > m
    // the split, the ranks and the present rows
    {
        const std::vector<rs_shard_update> u = {upd(4, 6, 0x600), upd(0, 9, 0x100), upd(4, 3, 0x300), upd(2, 4, 0x400),
                                                upd(1, 0, 0x500), upd(4, 2, 0x200), upd(5, 7, 0x700), upd(4, 9, 0x900)};
        UpdateDegradedPlan p;
        CHECK(rsmi::plan_update_degraded(k, n, 6, fl.data(), u.data(), u.size(), nullptr, &p) == RS_OK, "split");
        check_plan(p, k, n, fl, u, "split");
        CHECK(p.jobs.size() == 5 && p.decode_jobs == 2 && p.absorbed == 3 && p.max_j == 4 && p.max_src == 14 && p.degraded,
              "split: totals");
        if (p.jobs.size() == 5) {
            const rsmi::DegJob& j4 = p.jobs[3];
            CHECK(j4.stripe == 4 && j4.j == 4 && j4.jx == 2 && j4.nrows == 2, "split: stripe 4");
            // present 3, 9 first; then erased 2 (rank 0) and 6 (rank 1)
            const rsmi::DegEntry* e = &p.entries[j4.first];
            CHECK(e[0].shard == 3 && e[1].shard == 9 && e[2].shard == 2 && e[2].rank == 0 && e[3].shard == 6 && e[3].rank == 1,
                  "split: stripe 4 order");
            CHECK(p.rows[j4.row_first] == 1 && p.rows[j4.row_first + 1] == 2, "split: stripe 4 rows");
            // stripe 5: e > m, only a present shard changed: served, pair form
            CHECK(p.jobs[4].stripe == 5 && p.jobs[4].jx == 0 && p.jobs[4].nrows == 2, "split: stripe 5");
            CHECK(p.jobs[0].nrows == 4 && p.jobs[1].nrows == 3 && p.jobs[2].jx == 1, "split: stripes 0-2");
            CHECK(p.erased.size() == 2u * n && p.erased[4] == 1 && p.erased[n + 13] == 1, "split: flags are 0 / 1");
        }
    }
    // no flag in any listed stripe: not degraded (the garbage of stripe 3 is not looked at)
    {
        const std::vector<rs_shard_update> u = {upd(0, 1, 0x10), upd(0, 2, 0x20)};
        UpdateDegradedPlan p;
        CHECK(rsmi::plan_update_degraded(k, n, 6, fl.data(), u.data(), u.size(), nullptr, &p) == RS_OK && !p.degraded &&
                  p.decode_jobs == 0 && p.max_src == 2,
              "intact");
        check_plan(p, k, n, fl, u, "intact");
    }
    // count == 0: RS_OK and an empty plan, whatever the pointers
    {
        UpdateDegradedPlan p;
        p.max_j = 3;
        CHECK(rsmi::plan_update_degraded(k, n, 6, nullptr, nullptr, 0, nullptr, &p) == RS_OK && empty(p), "count == 0");
    }
    // refusals, and their order: the list first, the flags last
    {
        const rsmi::UpdateExtent ext{0x100000, 0x200000, 0x300000, 0x400000, 0x1000};
        UpdateDegradedPlan p;
        const rs_shard_update one = upd(0, 0, 0x10);
        CHECK(rsmi::plan_update_degraded(k, n, 6, nullptr, &one, 1, nullptr, &p) == RS_EINVAL && empty(p), "NULL erased");
        CHECK(rsmi::plan_update_degraded(k, n, 6, fl.data(), nullptr, 1, nullptr, &p) == RS_EINVAL, "NULL updates");
        refused("shard == k", k, n, 6, fl, {upd(0, 1, 0x10), upd(1, 10, 0x20)}, RS_EBAD_SHARE_ID);
        refused("stripe == stripes", k, n, 6, fl, {upd(6, 1, 0x10)}, RS_EINVAL);
        refused("duplicate", k, n, 6, fl, {upd(1, 2, 0x10), upd(0, 2, 0x20), upd(1, 2, 0x30)}, RS_EINVAL);
        refused("NULL src", k, n, 6, fl, {upd(0, 0, 0)}, RS_EINVAL);
        refused("misaligned src", k, n, 6, fl, {upd(0, 0, 0x18)}, RS_EINVAL);
        rs_shard_update r = upd(0, 0, 0x10);
        r.reserved = 1;
        refused("reserved", k, n, 6, fl, {r}, RS_EINVAL);
        refused("src in the data region", k, n, 6, fl, {upd(0, 0, 0x1FF800)}, RS_EINVAL, &ext);
        refused("src in the parity region", k, n, 6, fl, {upd(0, 0, 0x2FF010)}, RS_EINVAL, &ext);
        // U_x with e > m
        refused("erased changed shard, e > m", k, n, 6, fl, {upd(5, 1, 0x10)}, RS_ENOT_ENOUGH);
        refused("erased changed shard, e > m, among good ones", k, n, 6, fl, {upd(0, 1, 0x10), upd(5, 7, 0x20), upd(5, 2, 0x30)},
                RS_ENOT_ENOUGH);
        // a defect of the list wins over the flags, wherever it stands
        refused("bad id after too many erasures", k, n, 6, fl, {upd(5, 1, 0x10), upd(0, 10, 0x20)}, RS_EBAD_SHARE_ID);
        refused("duplicate after too many erasures", k, n, 6, fl, {upd(5, 1, 0x10), upd(0, 3, 0x20), upd(0, 3, 0x30)}, RS_EINVAL);
        refused("src in a region after too many erasures", k, n, 6, fl, {upd(5, 1, 0x10), upd(0, 3, 0x100000)}, RS_EINVAL, &ext);
        // a src that only touches the regions' ends is fine
        const std::vector<rs_shard_update> ok = {upd(0, 3, 0x200000), upd(1, 3, 0xFF000)};
        CHECK(rsmi::plan_update_degraded(k, n, 6, fl.data(), ok.data(), ok.size(), &ext, &p) == RS_OK && p.jobs.size() == 2,
              "src at the regions' ends");
        // e > m with present shards only: served
        const std::vector<rs_shard_update> pres = {upd(5, 3, 0x10), upd(5, 9, 0x20)};
        CHECK(rsmi::plan_update_degraded(k, n, 6, fl.data(), pres.data(), pres.size(), nullptr, &p) == RS_OK &&
                  p.jobs.size() == 1 && p.jobs[0].jx == 0 && p.decode_jobs == 0 && p.degraded && p.max_src == 2,
              "e > m, present only");
        // m == 0: an erased changed shard cannot be absorbed
        std::vector<uint8_t> f4(2 * 4, 0);
        f4[4 + 1] = 1;
        refused("m == 0, erased changed shard", 4, 4, 2, f4, {upd(1, 1, 0x10)}, RS_ENOT_ENOUGH);
        const rs_shard_update p4 = upd(1, 2, 0x10);
        CHECK(rsmi::plan_update_degraded(4, 4, 2, f4.data(), &p4, 1, nullptr, &p) == RS_OK && p.jobs[0].nrows == 0 && p.degraded,
              "m == 0, present changed shard");
    }
    // fixed-seed sweep against the model
    for (int rep = 0; rep < 300; ++rep) {
        const int kk = 1 + static_cast<int>(rnd() % 40), mm = static_cast<int>(rnd() % 9), nn = kk + mm;
        const size_t stripes = 1 + rnd() % 30;
        std::vector<uint8_t> f(stripes * nn, 0);
        for (size_t s = 0; s < stripes; ++s) {
            const int e = (rnd() % 3 == 0) ? 0 : static_cast<int>(rnd() % (mm + 2));
            for (int t = 0; t < e; ++t) f[s * nn + rnd() % nn] = static_cast<uint8_t>(1 + rnd() % 255);
        }
        std::set<std::pair<uint64_t, uint32_t>> seen;
        std::vector<rs_shard_update> u;
        const size_t count = rnd() % (2 * stripes + 1);
        for (size_t i = 0; i < count; ++i) {
            const uint64_t s = rnd() % stripes;
            const uint32_t sh = rnd() % static_cast<uint32_t>(kk);
            if (!seen.insert({s, sh}).second) continue;
            u.push_back(upd(s, sh, 16ull * (1 + rnd())));
        }
        // the model's verdict: RS_ENOT_ENOUGH iff a listed stripe has an erased changed shard and e > m
        bool too_many = false;
        for (const rs_shard_update& x : u) {
            int e = 0;
            for (int id = 0; id < nn; ++id) e += f[x.stripe * nn + id] != 0;
            too_many |= f[x.stripe * nn + x.shard] != 0 && e > mm;
        }
        UpdateDegradedPlan p;
        const int rc = rsmi::plan_update_degraded(kk, nn, stripes, f.data(), u.data(), u.size(), nullptr, &p);
        CHECK(rc == (too_many ? RS_ENOT_ENOUGH : RS_OK), "sweep %d: status %d, too_many %d", rep, rc, too_many);
        if (rc == RS_OK) check_plan(p, kk, nn, f, u, "sweep");
        else CHECK(empty(p), "sweep %d: refused plan not empty", rep);
    }
    std::printf("plan_update_degraded: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_update_degraded_standalone_sanitized(tmp_path):
    src = tmp_path / "update_degraded_plan_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "update_degraded_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src),
                    os.path.join(CSRC, "update_degraded_plan.cpp"), os.path.join(CSRC, "update_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_update_degraded: 0 failures" in run.stdout


def test_update_degraded_entry_point_is_exported():
    import rsmi
    assert "rs_update_degraded" in rsmi.EXPORTS
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    assert hasattr(lib, "rs_update_degraded")
    assert (rsmi.FEC.STAT_UPDATE_DEGRADED, rsmi.FEC.STAT_UPDATE_ABSORBED) == (20, 21)
    assert hasattr(rsmi.FEC, "update_degraded")


def test_null_context_is_rejected_without_a_device():
    """rs_update_degraded refuses a NULL context with RS_EINVAL before
    touching HIP; callable on a CPU-only machine."""
    import rsmi
    lib = rsmi.load()
    one = (rsmi.ShardUpdate * 1)(rsmi.ShardUpdate(0, 0, 0, 16))
    flags = ctypes.create_string_buffer(14)
    fp = ctypes.cast(flags, ctypes.c_void_p)
    assert lib.rs_update_degraded(None, None, 0, None, 0, 16, 16, 1, fp, one, 1, None) == rsmi.RS_EINVAL
    assert lib.rs_update_degraded(None, None, 0, None, 0, 16, 16, 1, None, None, 0, None) == rsmi.RS_EINVAL

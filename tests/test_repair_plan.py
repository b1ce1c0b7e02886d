"""CPU: the planner of rs_reconstruct_checked / rs_reconstruct_checked_ptrs
(csrc/check_plan.cpp, rsmi::plan_repairs and rsmi::plan_repairs_ptrs) and the
parts of the binding that need no GPU.

The planner checks run in a stand-alone C++ program (its own main) built from
csrc/check_plan.cpp with -fsanitize=address,undefined and run directly."""
import ctypes
import os
import subprocess

import pytest

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "check_plan.hpp"

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

static const rsmi::CheckLayout kLay{0x10000000ull, 0x80000000ull, 0x40000ull, 0x30000ull, 0x1010ull};

static std::vector<uint8_t> flags(size_t stripes, int n, const std::vector<std::pair<size_t, int>>& gone) {
    std::vector<uint8_t> f(stripes * n, 0);
    for (const auto& g : gone) f[g.first * n + g.second] = 1;
    return f;
}

// Rebuild's rule, written the long way: every present data share, then the
// highest-numbered present parity until there are k.
static std::vector<int> rebuild_choice(int k, int n, const uint8_t* fl) {
    std::vector<int> c;
    for (int i = 0; i < k; ++i)
        if (!fl[i]) c.push_back(i);
    for (int i = n - 1; i >= k && static_cast<int>(c.size()) < k; --i)
        if (!fl[i]) c.push_back(i);
    std::sort(c.begin(), c.end());
    return c;
}

static int plan(bool ptrs, int k, int n, size_t stripes, const uint8_t* er, const uint32_t* list, size_t count,
                rsmi::CheckPlan* p) {
    return ptrs ? rsmi::plan_repairs_ptrs(k, n, stripes, er, list, count, p)
                : rsmi::plan_repairs(k, n, stripes, er, list, count, kLay, p);
}

// The whole plan against a brute-force model.  `order` lists the planned
// stripes (all of them, or the caller's list).
static void model(const char* what, bool ptrs, int k, int n, const std::vector<uint8_t>& er,
                  const std::vector<uint32_t>& order, const rsmi::CheckPlan& p) {
    const int m = n - k;
    std::vector<uint32_t> intact;
    size_t saturated = 0, b = 0;
    uint32_t next = 0;
    CHECK(p.flags.size() == p.jobs.size() * static_cast<size_t>(n), "%s: %zu compact flags for %zu jobs", what,
          p.flags.size(), p.jobs.size());
    if (p.flags.size() != p.jobs.size() * static_cast<size_t>(n)) return;
    for (uint32_t s : order) {
        const uint8_t* fl = er.data() + static_cast<size_t>(s) * n;
        int e = 0;
        for (int i = 0; i < n; ++i) e += fl[i] != 0;
        if (e == 0) {
            intact.push_back(s);
            continue;
        }
        saturated += e == m;
        if (b >= p.jobs.size()) {
            CHECK(false, "%s: no job for stripe %u", what, s);
            return;
        }
        const rsmi::ReadJob& job = p.jobs[b];
        const uint8_t* xf = &p.flags[b * n];
        CHECK(job.stripe == s, "%s: job %zu is stripe %llu, want %u", what, b,
              static_cast<unsigned long long>(job.stripe), s);
        CHECK(job.first == next, "%s: job %zu starts at %u, not %u", what, b, job.first, next);
        CHECK(job.j == static_cast<uint32_t>(m), "%s: job %zu has %u entries, want %d", what, b, job.j, m);
        // X' holds exactly m flags, all 0 / 1, contains X, and leaves exactly Rebuild's choice
        int cnt = 0;
        std::vector<int> left, xp;
        for (int i = 0; i < n; ++i) {
            CHECK(xf[i] <= 1, "%s: compact flag %d of job %zu is %u", what, i, b, xf[i]);
            cnt += xf[i] != 0;
            if (fl[i]) CHECK(xf[i] == 1, "%s: X' of job %zu lacks erased id %d", what, b, i);
            if (xf[i]) xp.push_back(i);
            else left.push_back(i);
        }
        CHECK(cnt == m, "%s: X' of job %zu has %d flags, want %d", what, b, cnt, m);
        CHECK(left == rebuild_choice(k, n, fl), "%s: survivors of job %zu are not Rebuild's", what, b);
        if (static_cast<size_t>(job.first) + job.j > p.entries.size() || xp.size() != job.j) {
            CHECK(false, "%s: job %zu runs past the entry table", what, b);
            return;
        }
        // entries: every id of X' in id order, entry t with row t, stored iff erased
        int stores = 0;
        for (uint32_t t = 0; t < job.j; ++t) {
            const rsmi::ReadEntry& en = p.entries[job.first + t];
            const int id = xp[t];
            CHECK(en.row == t, "%s: job %zu entry %u: row %u", what, b, t, en.row);
            CHECK(en.pad == (fl[id] ? rsmi::kRepairStore : rsmi::kRepairCompare),
                  "%s: job %zu entry %u (id %d): store bit %u, erased %u", what, b, t, id, en.pad, fl[id]);
            stores += en.pad == rsmi::kRepairStore;
            if (!fl[id]) CHECK(id >= k, "%s: job %zu: data shard %d compared", what, b, id);
            const uint64_t at = ptrs  ? static_cast<uint64_t>(id)
                                : id < k ? kLay.data + s * kLay.data_ss + static_cast<uint64_t>(id) * kLay.pitch
                                         : kLay.parity + s * kLay.parity_ss + static_cast<uint64_t>(id - k) * kLay.pitch;
            CHECK(en.dst == at, "%s: job %zu entry %u: dst %llx, want %llx", what, b, t,
                  static_cast<unsigned long long>(en.dst), static_cast<unsigned long long>(at));
        }
        CHECK(stores == e, "%s: job %zu stores %d rows, e = %d", what, b, stores, e);
        next = job.first + job.j;
        ++b;
    }
    CHECK(b == p.jobs.size(), "%s: %zu jobs, want %zu", what, p.jobs.size(), b);
    CHECK(next == p.entries.size(), "%s: %zu entries, jobs cover %u", what, p.entries.size(), next);
    CHECK(p.intact == intact, "%s: intact list (%zu, want %zu)", what, p.intact.size(), intact.size());
    CHECK(p.saturated == saturated, "%s: saturated %zu, want %zu", what, p.saturated, saturated);
    CHECK(p.max_j == (b ? static_cast<uint32_t>(m) : 0u), "%s: max_j %u", what, p.max_j);
}

static std::vector<uint32_t> all(size_t stripes) {
    std::vector<uint32_t> o(stripes);
    for (size_t i = 0; i < stripes; ++i) o[i] = static_cast<uint32_t>(i);
    return o;
}

static bool empty(const rsmi::CheckPlan& p) {
    return p.intact.empty() && p.jobs.empty() && p.entries.empty() && p.flags.empty() && p.saturated == 0 &&
           p.max_j == 0;
}

static void refused(const char* what, int k, int n, size_t stripes, const uint8_t* er, const uint32_t* list,
                    size_t count, int want) {
    for (int ptrs = 0; ptrs < 2; ++ptrs) {
        rsmi::CheckPlan p;
        p.intact.push_back(3);  // stale contents must not survive a refusal
        p.jobs.push_back(rsmi::ReadJob{7, 0, 1});
        p.entries.push_back(rsmi::ReadEntry{16, 0, 0});
        p.flags.assign(3, 1);
        p.saturated = 2;
        p.max_j = 9;
        const int rc = plan(ptrs != 0, k, n, stripes, er, list, count, &p);
        CHECK(rc == want, "%s (ptrs %d): status %d, want %d", what, ptrs, rc, want);
        CHECK(empty(p), "%s (ptrs %d): plan not empty", what, ptrs);
    }
}

int main() {
    const int k = 10, n = 14;
    // the split, C by Rebuild's rule, rows, store bits and addresses by hand
    {
        // 0 intact | 1: data 3 gone | 2: parity 13 gone | 3: 0, 5, 11 gone | 4: four gone | 5 intact | 6: 2, 12 gone
        const std::vector<uint8_t> er = flags(
            7, n, {{1, 3}, {2, 13}, {3, 0}, {3, 5}, {3, 11}, {4, 1}, {4, 2}, {4, 10}, {4, 13}, {6, 2}, {6, 12}});
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_repairs(k, n, 7, er.data(), nullptr, 0, kLay, &p) == RS_OK, "split");
        CHECK((p.intact == std::vector<uint32_t>{0, 5}), "split: intact");
        CHECK(p.saturated == 1 && p.jobs.size() == 5 && p.entries.size() == 20 && p.max_j == 4,
              "split: %zu saturated, %zu jobs, %zu entries, max_j %u", p.saturated, p.jobs.size(), p.entries.size(),
              p.max_j);
        if (p.jobs.size() == 5 && p.entries.size() == 20) {
            const uint64_t S = rsmi::kRepairStore, C = rsmi::kRepairCompare;
            struct Want {
                uint32_t stripe;
                int id[4];
                uint64_t st[4];
            };
            const Want want[5] = {
                {1, {3, 10, 11, 12}, {S, C, C, C}},   // X = {3}; C takes 13; U = {10, 11, 12}
                {2, {10, 11, 12, 13}, {C, C, C, S}},  // X = {13}; C = the data; U = {10, 11, 12}
                {3, {0, 5, 10, 11}, {S, S, C, S}},    // X = {0, 5, 11}; C takes 13, 12; U = {10}: a mixed group
                {4, {1, 2, 10, 13}, {S, S, S, S}},    // saturated: every row stored
                {6, {2, 10, 11, 12}, {S, C, C, S}},   // X = {2, 12}; C takes 13; U = {10, 11}
            };
            for (int b = 0; b < 5; ++b) {
                CHECK(p.jobs[b].stripe == want[b].stripe && p.jobs[b].first == 4u * b && p.jobs[b].j == 4, "split: job %d", b);
                for (int t = 0; t < 4; ++t) {
                    const rsmi::ReadEntry& en = p.entries[4 * b + t];
                    const int id = want[b].id[t];
                    const uint64_t at = id < k ? kLay.data + want[b].stripe * kLay.data_ss + id * kLay.pitch
                                               : kLay.parity + want[b].stripe * kLay.parity_ss + (id - k) * kLay.pitch;
                    CHECK(en.dst == at && en.row == static_cast<uint32_t>(t) && en.pad == want[b].st[t],
                          "split: job %d entry %d", b, t);
                    CHECK(p.flags[b * n + id] == 1, "split: job %d flag %d", b, id);
                }
            }
        }
        model("split", false, k, n, er, all(7), p);
        CHECK(rsmi::plan_repairs_ptrs(k, n, 7, er.data(), nullptr, 0, &p) == RS_OK, "split ptrs");
        if (p.entries.size() == 20) {
            const uint64_t ids3[4] = {0, 5, 10, 11};
            for (int t = 0; t < 4; ++t) CHECK(p.entries[8 + t].dst == ids3[t], "split ptrs: stripe 3 entry %d", t);
        }
        model("split ptrs", true, k, n, er, all(7), p);
        // a stripe list: only the listed stripes are planned, and only their flags examined
        std::vector<uint8_t> er2 = er;
        for (int i = 0; i < n; ++i) er2[2 * n + i] = 1;  // unlisted: fully erased
        const std::vector<uint32_t> list = {0, 3, 4, 6};
        for (int ptrs = 0; ptrs < 2; ++ptrs) {
            CHECK(plan(ptrs != 0, k, n, 7, er2.data(), list.data(), list.size(), &p) == RS_OK, "list");
            CHECK((p.intact == std::vector<uint32_t>{0}) && p.jobs.size() == 3 && p.saturated == 1, "list: split");
            model("list", ptrs != 0, k, n, er2, list, p);
            // an empty list plans nothing
            CHECK(plan(ptrs != 0, k, n, 7, er.data(), list.data(), 0, &p) == RS_OK && empty(p), "empty list");
        }
        const uint32_t bad1[2] = {3, 3}, bad2[2] = {4, 1}, bad3[1] = {7};
        refused("list repeats", k, n, 7, er.data(), bad1, 2, RS_EINVAL);
        refused("list descends", k, n, 7, er.data(), bad2, 2, RS_EINVAL);
        refused("list out of range", k, n, 7, er.data(), bad3, 1, RS_EINVAL);
    }
    // e > m is not enough, also after good jobs were planned
    {
        std::vector<uint8_t> er = flags(3, n, {{0, 4}, {1, 0}, {1, 1}, {1, 2}, {1, 3}});
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_repairs(k, n, 3, er.data(), nullptr, 0, kLay, &p) == RS_OK && p.jobs.size() == 2 &&
                  p.saturated == 1 && p.intact.size() == 1,
              "e == m");
        er[2 * n + 13] = er[2 * n + 12] = er[2 * n + 11] = er[2 * n + 10] = er[2 * n + 9] = 1;
        refused("e == m + 1 after good jobs", k, n, 3, er.data(), nullptr, 0, RS_ENOT_ENOUGH);
        std::vector<uint8_t> gone(n, 1);
        refused("everything gone", k, n, 1, gone.data(), nullptr, 0, RS_ENOT_ENOUGH);
    }
    // flag values other than 0 / 1 count as set and come out as 1
    {
        std::vector<uint8_t> er(2 * n, 0);
        er[0 * n + 7] = 255;
        er[0 * n + 11] = 2;
        er[1 * n + 0] = 128;
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_repairs(k, n, 2, er.data(), nullptr, 0, kLay, &p) == RS_OK && p.jobs.size() == 2, "non-0/1 flags");
        model("non-0/1 flags", false, k, n, er, all(2), p);
    }
    // k == n: no parity, so every stripe is intact or has too many erasures
    {
        std::vector<uint8_t> er(3 * 6, 0);
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_repairs(6, 6, 3, er.data(), nullptr, 0, kLay, &p) == RS_OK && p.intact.size() == 3 &&
                  p.jobs.empty() && p.saturated == 0 && p.max_j == 0,
              "k == n");
        er[1 * 6 + 2] = 1;
        refused("k == n, one erasure", 6, 6, 3, er.data(), nullptr, 0, RS_ENOT_ENOUGH);
    }
    // m == 1: a stripe is intact or saturated, and the saturated one is a job of one stored row
    {
        const std::vector<uint8_t> er = flags(3, 5, {{1, 4}, {2, 0}});
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_repairs(4, 5, 3, er.data(), nullptr, 0, kLay, &p) == RS_OK && p.intact.size() == 1 &&
                  p.jobs.size() == 2 && p.saturated == 2 && p.entries.size() == 2 &&
                  p.entries[0].pad == rsmi::kRepairStore && p.entries[1].pad == rsmi::kRepairStore &&
                  p.entries[1].dst == kLay.data + 2 * kLay.data_ss,
              "m == 1");
        model("m == 1", false, 4, 5, er, all(3), p);
    }
    // argument refusals; stripes == 0 is an empty plan whatever the pointers
    {
        const std::vector<uint8_t> er(n, 0);
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_repairs(k, n, 1, er.data(), nullptr, 0, kLay, nullptr) == RS_EINVAL, "NULL plan");
        CHECK(rsmi::plan_repairs_ptrs(k, n, 1, er.data(), nullptr, 0, nullptr) == RS_EINVAL, "NULL plan ptrs");
        refused("NULL erased", k, n, 1, nullptr, nullptr, 0, RS_EINVAL);
        refused("k == 0", 0, n, 1, er.data(), nullptr, 0, RS_EINVAL);
        refused("n < k", k, 9, 1, er.data(), nullptr, 0, RS_EINVAL);
        refused("n > 256", k, 257, 1, er.data(), nullptr, 0, RS_EINVAL);
        refused("2^32 stripes", k, n, size_t(1) << 32, er.data(), nullptr, 0, RS_EINVAL);
        p.max_j = 3;
        CHECK(rsmi::plan_repairs(k, n, 0, nullptr, nullptr, 0, kLay, &p) == RS_OK && empty(p), "stripes == 0");
        p.max_j = 3;
        CHECK(rsmi::plan_repairs_ptrs(k, n, 0, nullptr, nullptr, 0, &p) == RS_OK && empty(p), "stripes == 0 ptrs");
    }
    // plan_checks keeps its behaviour next to its sibling: saturated stripes get no job, entries are U only
    {
        const std::vector<uint8_t> er = flags(3, n, {{0, 4}, {1, 0}, {1, 1}, {1, 2}, {1, 3}});
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_checks(k, n, 3, er.data(), nullptr, 0, kLay, &p) == RS_OK && p.jobs.size() == 1 &&
                  p.jobs[0].j == 3 && p.entries.size() == 3 && p.entries[0].pad == 0 && p.entries[0].row == 1 &&
                  p.saturated == 1 && p.max_j == 3,
              "plan_checks unchanged");
    }
    // fixed-seed sweep against the model, over several (k, n)
    for (int rep = 0; rep < 300; ++rep) {
        const int kk = 1 + static_cast<int>(rnd() % 64);
        const int nn = kk + static_cast<int>(rnd() % 20);
        const int mm = nn - kk;
        const size_t stripes = 1 + rnd() % 50;
        std::vector<uint8_t> er(stripes * nn, 0);
        for (size_t s = 0; s < stripes; ++s) {
            int e = (mm && rnd() % 4) ? static_cast<int>(rnd() % (mm + 1)) : 0;
            if (mm && rnd() % 8 == 0) e = mm;
            for (int placed = 0; placed < e;) {
                const uint32_t id = rnd() % nn;
                if (!er[s * nn + id]) er[s * nn + id] = static_cast<uint8_t>(1 + rnd() % 255), ++placed;
            }
        }
        std::vector<uint32_t> list = {static_cast<uint32_t>(rnd() % stripes)};  // never empty: a NULL list means all
        for (size_t s = list[0] + 1; s < stripes; ++s)
            if (rnd() % 2) list.push_back(static_cast<uint32_t>(s));
        for (int ptrs = 0; ptrs < 2; ++ptrs) {
            rsmi::CheckPlan p;
            const int rc = plan(ptrs != 0, kk, nn, stripes, er.data(), nullptr, 0, &p);
            CHECK(rc == RS_OK, "sweep %d: status %d", rep, rc);
            model("sweep", ptrs != 0, kk, nn, er, all(stripes), p);
            const int rl = plan(ptrs != 0, kk, nn, stripes, er.data(), list.data(), list.size(), &p);
            CHECK(rl == RS_OK, "sweep %d: list status %d", rep, rl);
            model("sweep list", ptrs != 0, kk, nn, er, list, p);
        }
        // one stripe pushed past m: refused whatever came before it
        const size_t victim = rnd() % stripes;
        int e = 0;
        for (int id = 0; id < nn && e <= mm; ++id) e += er[victim * nn + id] != 0;
        for (int id = 0; id < nn && e <= mm; ++id)
            if (!er[victim * nn + id]) er[victim * nn + id] = 1, ++e;
        refused("sweep: too many", kk, nn, stripes, er.data(), nullptr, 0, RS_ENOT_ENOUGH);
    }
    std::printf("plan_repairs: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_repairs_standalone_sanitized(tmp_path):
    src = tmp_path / "repair_plan_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "repair_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "check_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_repairs: 0 failures" in run.stdout


def test_checked_repair_entry_points_are_exported():
    import rsmi
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    for name in ("rs_reconstruct_checked", "rs_reconstruct_checked_ptrs"):
        assert name in rsmi.EXPORTS
        assert hasattr(lib, name)
    assert rsmi.FEC.STAT_REPAIR_CHECKED == 26
    assert hasattr(rsmi.FEC, "reconstruct_checked") and hasattr(rsmi.FEC, "reconstruct_checked_ptrs")


def test_null_context_is_rejected_without_a_device():
    """Both calls refuse a NULL context with RS_EINVAL before touching HIP;
    callable on a CPU-only machine."""
    import rsmi
    lib = rsmi.load()
    flags = ctypes.create_string_buffer(14)
    fp = ctypes.cast(flags, ctypes.c_void_p)
    assert lib.rs_reconstruct_checked(None, None, 0, None, 0, 16, 16, 1, fp, None, None) == rsmi.RS_EINVAL
    assert lib.rs_reconstruct_checked(None, None, 0, None, 0, 16, 16, 0, None, None, None) == rsmi.RS_EINVAL
    assert lib.rs_reconstruct_checked_ptrs(None, None, 16, 1, fp, None, None) == rsmi.RS_EINVAL
    assert lib.rs_reconstruct_checked_ptrs(None, None, 16, 0, None, None, None) == rsmi.RS_EINVAL


def test_wrong_flag_count_raises_before_the_call():
    """The binding checks len(erased) == stripes * n itself, before it touches
    the handle: no context is needed to see it."""
    import rsmi
    f = object.__new__(rsmi.FEC)
    f.k, f.n, f._h = 10, 14, None
    for bad in (b"", bytes(13), bytes(15), bytes(3 * 14)):
        with pytest.raises(rsmi.RSError) as ei:
            f.reconstruct_checked(0, 0, 0, 0, 16, 16, 1, bad, 0)
        assert ei.value.code == rsmi.RS_EINVAL
        with pytest.raises(rsmi.RSError) as ei:
            f.reconstruct_checked_ptrs(0, 16, 1, bad, 0)
        assert ei.value.code == rsmi.RS_EINVAL

"""CPU: the pointer-mode planner of rs_verify_ptrs / rs_correct_columns_ptrs
(csrc/check_plan.cpp, rsmi::plan_checks_ptrs) and the parts of the two calls
that need no GPU.

The planner checks run in a stand-alone C++ program (its own main) built from
csrc/check_plan.cpp with -fsanitize=address,undefined and run directly, as
tests/test_check_plan.py does for plan_checks."""
import ctypes
import os
import subprocess

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static bool same_jobs(const rsmi::CheckPlan& a, const rsmi::CheckPlan& b) {
    if (a.jobs.size() != b.jobs.size()) return false;
    for (size_t i = 0; i < a.jobs.size(); ++i)
        if (a.jobs[i].stripe != b.jobs[i].stripe || a.jobs[i].first != b.jobs[i].first || a.jobs[i].j != b.jobs[i].j)
            return false;
    return true;
}

// One code: random erasure sets, the pointer plan against a model written from
// the definition, and its splits against the strided plan for the same flags.
static void sweep(int k, int n, int reps) {
    const int m = n - k;
    for (int rep = 0; rep < reps; ++rep) {
        const size_t stripes = 1 + rnd() % 12;
        std::vector<uint8_t> er(stripes * n, 0);
        for (size_t s = 0; s < stripes; ++s) {
            int e = rnd() % 4 ? static_cast<int>(rnd() % (m + 1)) : 0;
            if (rnd() % 8 == 0) e = m;
            for (int placed = 0; placed < e;) {
                const uint32_t id = rnd() % n;
                if (!er[s * n + id]) er[s * n + id] = static_cast<uint8_t>(1 + rnd() % 255), ++placed;
            }
        }
        rsmi::CheckPlan p, q;
        CHECK(rsmi::plan_checks_ptrs(k, n, stripes, er.data(), nullptr, 0, &p) == RS_OK, "RS(%d,%d): status", k, n);
        CHECK(rsmi::plan_checks(k, n, stripes, er.data(), nullptr, 0, kLay, &q) == RS_OK, "RS(%d,%d): strided", k, n);
        // the intact, saturated and job splits are the strided plan's
        CHECK(p.intact == q.intact && p.saturated == q.saturated && same_jobs(p, q) && p.flags == q.flags &&
                  p.max_j == q.max_j && p.entries.size() == q.entries.size(),
              "RS(%d,%d) rep %d: splits differ from the strided plan", k, n, rep);
        if (p.entries.size() != q.entries.size()) continue;
        for (size_t b = 0; b < p.jobs.size(); ++b) {
            const rsmi::ReadJob& job = p.jobs[b];
            const uint8_t* fl = er.data() + job.stripe * n;
            const uint8_t* xf = &p.flags[b * n];
            // present \ Rebuild's choice, in id order
            const std::vector<int> c = rebuild_choice(k, n, fl);
            std::vector<int> u;
            for (int i = 0; i < n; ++i)
                if (!fl[i] && !std::binary_search(c.begin(), c.end(), i)) u.push_back(i);
            CHECK(u.size() == job.j, "RS(%d,%d): job %zu has j %u, want %zu", k, n, b, job.j, u.size());
            if (u.size() != job.j || static_cast<size_t>(job.first) + job.j > p.entries.size()) continue;
            for (uint32_t t = 0; t < job.j; ++t) {
                const rsmi::ReadEntry& en = p.entries[job.first + t];
                const int id = u[t];
                uint32_t rank = 0;  // rank of the id in X' = erased + U
                for (int i = 0; i < id; ++i) rank += xf[i] != 0;
                CHECK(en.dst == static_cast<uint64_t>(id), "RS(%d,%d): job %zu entry %u carries %llx, want id %d", k, n, b,
                      t, static_cast<unsigned long long>(en.dst), id);
                CHECK(en.dst < static_cast<uint64_t>(n), "RS(%d,%d): entry is no shard id", k, n);
                CHECK(en.row == rank && en.pad == 0, "RS(%d,%d): job %zu entry %u: row %u, want %u", k, n, b, t, en.row,
                      rank);
                CHECK(en.row == q.entries[job.first + t].row, "RS(%d,%d): row differs from the strided plan's", k, n);
                CHECK(xf[id] == 1 && !fl[id], "RS(%d,%d): entry %d is not in X' minus X", k, n, id);
            }
        }
        // a stripe list plans the same subset
        std::vector<uint32_t> list = {static_cast<uint32_t>(rnd() % stripes)};
        for (size_t s = list[0] + 1; s < stripes; ++s)
            if (rnd() % 2) list.push_back(static_cast<uint32_t>(s));
        CHECK(rsmi::plan_checks_ptrs(k, n, stripes, er.data(), list.data(), list.size(), &p) == RS_OK &&
                  rsmi::plan_checks(k, n, stripes, er.data(), list.data(), list.size(), kLay, &q) == RS_OK &&
                  p.intact == q.intact && p.saturated == q.saturated && same_jobs(p, q) && p.flags == q.flags,
              "RS(%d,%d) rep %d: listed plan", k, n, rep);
        // one stripe past m: refused, the plan left empty
        const size_t victim = rnd() % stripes;
        int e = 0;
        for (int id = 0; id < n; ++id) e += er[victim * n + id] != 0;
        for (int id = 0; id < n && e <= m; ++id)
            if (!er[victim * n + id]) er[victim * n + id] = 1, ++e;
        CHECK(rsmi::plan_checks_ptrs(k, n, stripes, er.data(), nullptr, 0, &p) == RS_ENOT_ENOUGH && p.jobs.empty() &&
                  p.entries.empty() && p.intact.empty() && p.flags.empty() && p.saturated == 0 && p.max_j == 0,
              "RS(%d,%d): too many erasures", k, n);
    }
}

int main() {
    sweep(4, 6, 200);
    sweep(10, 14, 200);
    sweep(64, 80, 60);
    sweep(240, 256, 30);
    // The strided plan of a fixed input, every byte of it, from CheckLayout:
    // RS(10,14), 0 intact | 1: data 3 gone | 2: four gone | 3: 0, 5, 11 gone | 4: 2, 12 gone
    {
        const int k = 10, n = 14;
        std::vector<uint8_t> er(5 * n, 0);
        const int gone[][2] = {{1, 3}, {2, 1}, {2, 2}, {2, 10}, {2, 13}, {3, 0}, {3, 5}, {3, 11}, {4, 2}, {4, 12}};
        for (const auto& g : gone) er[g[0] * n + g[1]] = 1;
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_checks(k, n, 5, er.data(), nullptr, 0, kLay, &p) == RS_OK, "fixed: status");
        auto at = [&](uint64_t s, int id) { return kLay.parity + s * kLay.parity_ss + static_cast<uint64_t>(id - k) * kLay.pitch; };
        const rsmi::ReadJob jobs[3] = {{1, 0, 3}, {3, 3, 1}, {4, 4, 2}};
        const rsmi::ReadEntry ent[6] = {{at(1, 10), 1, 0}, {at(1, 11), 2, 0}, {at(1, 12), 3, 0},
                                        {at(3, 10), 2, 0}, {at(4, 10), 1, 0}, {at(4, 11), 2, 0}};
        const uint8_t xf[3][14] = {{0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0},
                                   {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1, 0, 0},
                                   {0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 0}};
        CHECK((p.intact == std::vector<uint32_t>{0}) && p.saturated == 1 && p.max_j == 3, "fixed: splits");
        CHECK(p.jobs.size() == 3 && std::memcmp(p.jobs.data(), jobs, sizeof(jobs)) == 0, "fixed: job bytes");
        CHECK(p.entries.size() == 6 && std::memcmp(p.entries.data(), ent, sizeof(ent)) == 0, "fixed: entry bytes");
        CHECK(p.flags.size() == 3 * 14 && std::memcmp(p.flags.data(), xf, sizeof(xf)) == 0, "fixed: flag bytes");
        // and the pointer plan of the same input differs in the entries' dst only
        rsmi::CheckPlan q;
        CHECK(rsmi::plan_checks_ptrs(k, n, 5, er.data(), nullptr, 0, &q) == RS_OK, "fixed: ptrs status");
        const uint64_t ids[6] = {10, 11, 12, 10, 10, 11};
        CHECK(q.entries.size() == 6, "fixed: ptrs entries");
        for (size_t i = 0; i < q.entries.size() && i < 6; ++i)
            CHECK(q.entries[i].dst == ids[i] && q.entries[i].row == ent[i].row && q.entries[i].pad == 0, "fixed: ptrs entry %zu", i);
        CHECK(same_jobs(p, q) && p.flags == q.flags && p.intact == q.intact, "fixed: ptrs splits");
    }
    // refusals, as plan_checks
    {
        const std::vector<uint8_t> er(14, 0);
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_checks_ptrs(10, 14, 1, er.data(), nullptr, 0, nullptr) == RS_EINVAL, "NULL plan");
        CHECK(rsmi::plan_checks_ptrs(10, 14, 1, nullptr, nullptr, 0, &p) == RS_EINVAL, "NULL erased");
        CHECK(rsmi::plan_checks_ptrs(10, 14, size_t(1) << 32, er.data(), nullptr, 0, &p) == RS_EINVAL, "2^32 stripes");
        CHECK(rsmi::plan_checks_ptrs(10, 14, 0, nullptr, nullptr, 0, &p) == RS_OK && p.jobs.empty(), "stripes == 0");
    }
    std::printf("plan_checks_ptrs: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_checks_ptrs_standalone_sanitized(tmp_path):
    src = tmp_path / "check_plan_ptrs_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "check_plan_ptrs_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "check_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_checks_ptrs: 0 failures" in run.stdout


def test_ptrs_entry_points_are_exported():
    import rsmi
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    for name in ("rs_verify_ptrs", "rs_correct_columns_ptrs"):
        assert name in rsmi.EXPORTS
        assert hasattr(lib, name)
    assert hasattr(rsmi.FEC, "verify_ptrs") and hasattr(rsmi.FEC, "correct_columns_ptrs")


def test_null_context_is_rejected_without_a_device():
    """Both calls refuse a NULL context with RS_EINVAL before touching HIP;
    callable on a CPU-only machine."""
    import rsmi
    lib = rsmi.load()
    flags = ctypes.create_string_buffer(14)
    fp = ctypes.cast(flags, ctypes.c_void_p)
    st = (ctypes.c_int * 1)()
    assert lib.rs_verify_ptrs(None, None, 16, 1, fp, None, None) == rsmi.RS_EINVAL
    assert lib.rs_verify_ptrs(None, None, 16, 0, None, None, None) == rsmi.RS_EINVAL
    assert lib.rs_correct_columns_ptrs(None, None, 16, 1, fp, st, None, None) == rsmi.RS_EINVAL
    assert lib.rs_correct_columns_ptrs(None, None, 0, 1, None, None, None, None) == rsmi.RS_EINVAL

"""CPU: the planner of rs_verify_degraded / rs_correct_degraded
(csrc/check_plan.cpp, rsmi::plan_checks) and the parts of the binding that
need no GPU.

The planner checks run in a stand-alone C++ program (its own main) built from
csrc/check_plan.cpp with -fsanitize=address,undefined and run directly."""
import ctypes
import os
import subprocess

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")

PROGRAM = r"""
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "check_plan.hpp"

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

// The whole plan against a brute-force model.  `order` lists the planned
// stripes (all of them, or the caller's list).
static void model(const char* what, int k, int n, const std::vector<uint8_t>& er, const std::vector<uint32_t>& order,
                  const rsmi::CheckPlan& p) {
    const int m = n - k;
    std::vector<uint32_t> intact;
    size_t saturated = 0, b = 0;
    uint32_t next = 0, max_j = 0;
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
        if (e == m) {
            ++saturated;
            continue;
        }
        if (b >= p.jobs.size()) {
            CHECK(false, "%s: no job for stripe %u", what, s);
            return;
        }
        const rsmi::ReadJob& job = p.jobs[b];
        const uint8_t* xf = &p.flags[b * n];
        CHECK(job.stripe == s, "%s: job %zu is stripe %llu, want %u", what, b,
              static_cast<unsigned long long>(job.stripe), s);
        CHECK(job.first == next, "%s: job %zu starts at %u, not %u", what, b, job.first, next);
        CHECK(job.j == static_cast<uint32_t>(m - e), "%s: job %zu has j %u, want %d", what, b, job.j, m - e);
        // X' holds exactly m flags, all 0 / 1, contains X, and leaves exactly Rebuild's choice
        int cnt = 0;
        std::vector<int> left;
        for (int i = 0; i < n; ++i) {
            CHECK(xf[i] <= 1, "%s: compact flag %d of job %zu is %u", what, i, b, xf[i]);
            cnt += xf[i] != 0;
            if (fl[i]) CHECK(xf[i] == 1, "%s: X' of job %zu lacks erased id %d", what, b, i);
            if (!xf[i]) left.push_back(i);
        }
        CHECK(cnt == m, "%s: X' of job %zu has %d flags, want %d", what, b, cnt, m);
        CHECK(left == rebuild_choice(k, n, fl), "%s: survivors of job %zu are not Rebuild's", what, b);
        // entries: U = X' minus X in id order, row = brute-force rank in X', address of the stored shard
        std::vector<int> u;
        for (int i = 0; i < n; ++i)
            if (xf[i] && !fl[i]) u.push_back(i);
        CHECK(u.size() == job.j, "%s: job %zu: |U| = %zu, j = %u", what, b, u.size(), job.j);
        if (static_cast<size_t>(job.first) + job.j > p.entries.size() || u.size() != job.j) {
            CHECK(false, "%s: job %zu runs past the entry table", what, b);
            return;
        }
        for (uint32_t t = 0; t < job.j; ++t) {
            const rsmi::ReadEntry& en = p.entries[job.first + t];
            const int id = u[t];
            uint32_t rank = 0;
            for (int i = 0; i < id; ++i) rank += xf[i] != 0;
            CHECK(en.row == rank && en.pad == 0, "%s: job %zu entry %u: row %u, want %u", what, b, t, en.row, rank);
            CHECK(id >= k, "%s: job %zu: data shard %d in U", what, b, id);
            const uint64_t at = id < k ? kLay.data + s * kLay.data_ss + static_cast<uint64_t>(id) * kLay.pitch
                                       : kLay.parity + s * kLay.parity_ss + static_cast<uint64_t>(id - k) * kLay.pitch;
            CHECK(en.dst == at, "%s: job %zu entry %u: address %llx, want %llx", what, b, t,
                  static_cast<unsigned long long>(en.dst), static_cast<unsigned long long>(at));
        }
        next = job.first + job.j;
        max_j = std::max(max_j, job.j);
        ++b;
    }
    CHECK(b == p.jobs.size(), "%s: %zu jobs, want %zu", what, p.jobs.size(), b);
    CHECK(next == p.entries.size(), "%s: %zu entries, jobs cover %u", what, p.entries.size(), next);
    CHECK(p.intact == intact, "%s: intact list (%zu, want %zu)", what, p.intact.size(), intact.size());
    CHECK(p.saturated == saturated, "%s: saturated %zu, want %zu", what, p.saturated, saturated);
    CHECK(p.max_j == max_j, "%s: max_j %u, want %u", what, p.max_j, max_j);
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
    rsmi::CheckPlan p;
    p.intact.push_back(3);  // stale contents must not survive a refusal
    p.jobs.push_back(rsmi::ReadJob{7, 0, 1});
    p.entries.push_back(rsmi::ReadEntry{16, 0, 0});
    p.flags.assign(3, 1);
    p.saturated = 2;
    p.max_j = 9;
    const int rc = rsmi::plan_checks(k, n, stripes, er, list, count, kLay, &p);
    CHECK(rc == want, "%s: status %d, want %d", what, rc, want);
    CHECK(empty(p), "%s: plan not empty", what);
}

int main() {
    const int k = 10, n = 14;
    // the three-way split, C by Rebuild's rule, rows and addresses by hand
    {
        // 0 intact | 1: data 3 gone | 2: parity 13 gone | 3: 0, 5, 11 gone | 4: four gone | 5 intact | 6: 2, 12 gone
        const std::vector<uint8_t> er = flags(
            7, n, {{1, 3}, {2, 13}, {3, 0}, {3, 5}, {3, 11}, {4, 1}, {4, 2}, {4, 10}, {4, 13}, {6, 2}, {6, 12}});
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_checks(k, n, 7, er.data(), nullptr, 0, kLay, &p) == RS_OK, "split");
        CHECK((p.intact == std::vector<uint32_t>{0, 5}), "split: intact");
        CHECK(p.saturated == 1 && p.jobs.size() == 4 && p.entries.size() == 3 + 3 + 1 + 2 && p.max_j == 3,
              "split: %zu saturated, %zu jobs, %zu entries, max_j %u", p.saturated, p.jobs.size(), p.entries.size(),
              p.max_j);
        if (p.jobs.size() == 4 && p.entries.size() == 9) {
            // stripe 1: X = {3}; C = data minus 3, plus parity 13; U = {10, 11, 12}; X' = {3, 10, 11, 12}
            CHECK(p.jobs[0].stripe == 1 && p.jobs[0].j == 3, "split: job 0");
            const uint32_t rows1[3] = {1, 2, 3};
            for (int t = 0; t < 3; ++t)
                CHECK(p.entries[t].row == rows1[t] &&
                          p.entries[t].dst == kLay.parity + 1 * kLay.parity_ss + static_cast<uint64_t>(t) * kLay.pitch,
                      "split: stripe 1 entry %d", t);
            for (int i = 0; i < n; ++i)
                CHECK(p.flags[0 * n + i] == (i == 3 || (i >= 10 && i <= 12) ? 1 : 0), "split: stripe 1 flag %d", i);
            // stripe 2: X = {13}; C = the data; U = {10, 11, 12}; X' = all parity: rows 0, 1, 2
            CHECK(p.jobs[1].stripe == 2 && p.jobs[1].j == 3 && p.entries[3].row == 0 && p.entries[5].row == 2,
                  "split: job 1");
            // stripe 3: X = {0, 5, 11}; C takes 13 and 12; U = {10}; X' = {0, 5, 10, 11}: row 2
            CHECK(p.jobs[2].stripe == 3 && p.jobs[2].j == 1 && p.entries[6].row == 2 &&
                      p.entries[6].dst == kLay.parity + 3 * kLay.parity_ss,
                  "split: job 2");
            // stripe 6: X = {2, 12}; C takes 13; U = {10, 11}; X' = {2, 10, 11, 12}: rows 1, 2
            CHECK(p.jobs[3].stripe == 6 && p.jobs[3].j == 2 && p.entries[7].row == 1 && p.entries[8].row == 2 &&
                      p.entries[8].dst == kLay.parity + 6 * kLay.parity_ss + kLay.pitch,
                  "split: job 3");
        }
        model("split", k, n, er, all(7), p);
        // a stripe list: only the listed stripes are planned, and only their flags examined
        std::vector<uint8_t> er2 = er;
        for (int i = 0; i < n; ++i) er2[2 * n + i] = 1;  // unlisted: fully erased
        const std::vector<uint32_t> list = {0, 3, 4, 6};
        CHECK(rsmi::plan_checks(k, n, 7, er2.data(), list.data(), list.size(), kLay, &p) == RS_OK, "list");
        CHECK((p.intact == std::vector<uint32_t>{0}) && p.jobs.size() == 2 && p.saturated == 1, "list: split");
        model("list", k, n, er2, list, p);
        const uint32_t bad1[2] = {3, 3}, bad2[2] = {4, 1}, bad3[1] = {7};
        refused("list repeats", k, n, 7, er.data(), bad1, 2, RS_EINVAL);
        refused("list descends", k, n, 7, er.data(), bad2, 2, RS_EINVAL);
        refused("list out of range", k, n, 7, er.data(), bad3, 1, RS_EINVAL);
        // an empty list plans nothing
        CHECK(rsmi::plan_checks(k, n, 7, er.data(), list.data(), 0, kLay, &p) == RS_OK && empty(p), "empty list");
    }
    // e == m produces no job; e > m is not enough, also after good jobs were planned
    {
        std::vector<uint8_t> er = flags(3, n, {{0, 4}, {1, 0}, {1, 1}, {1, 2}, {1, 3}});
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_checks(k, n, 3, er.data(), nullptr, 0, kLay, &p) == RS_OK && p.jobs.size() == 1 &&
                  p.saturated == 1 && p.intact.size() == 1,
              "e == m");
        er[2 * n + 13] = er[2 * n + 12] = er[2 * n + 11] = er[2 * n + 10] = er[2 * n + 9] = 1;
        refused("e == m + 1 after a good job", k, n, 3, er.data(), nullptr, 0, RS_ENOT_ENOUGH);
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
        CHECK(rsmi::plan_checks(k, n, 2, er.data(), nullptr, 0, kLay, &p) == RS_OK && p.jobs.size() == 2 &&
                  p.jobs[0].j == 2 && p.jobs[1].j == 3,
              "non-0/1 flags");
        model("non-0/1 flags", k, n, er, all(2), p);
    }
    // k == n: no parity, so every stripe is intact or has too many erasures
    {
        std::vector<uint8_t> er(3 * 6, 0);
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_checks(6, 6, 3, er.data(), nullptr, 0, kLay, &p) == RS_OK && p.intact.size() == 3 &&
                  p.jobs.empty() && p.saturated == 0,
              "k == n");
        er[1 * 6 + 2] = 1;
        refused("k == n, one erasure", 6, 6, 3, er.data(), nullptr, 0, RS_ENOT_ENOUGH);
    }
    // m == 1: one erasure saturates the stripe
    {
        const std::vector<uint8_t> er = flags(2, 5, {{1, 4}});
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_checks(4, 5, 2, er.data(), nullptr, 0, kLay, &p) == RS_OK && p.intact.size() == 1 &&
                  p.jobs.empty() && p.saturated == 1,
              "m == 1");
    }
    // argument refusals; stripes == 0 is an empty plan whatever the pointers
    {
        const std::vector<uint8_t> er(n, 0);
        rsmi::CheckPlan p;
        CHECK(rsmi::plan_checks(k, n, 1, er.data(), nullptr, 0, kLay, nullptr) == RS_EINVAL, "NULL plan");
        refused("NULL erased", k, n, 1, nullptr, nullptr, 0, RS_EINVAL);
        refused("k == 0", 0, n, 1, er.data(), nullptr, 0, RS_EINVAL);
        refused("n < k", k, 9, 1, er.data(), nullptr, 0, RS_EINVAL);
        refused("n > 256", k, 257, 1, er.data(), nullptr, 0, RS_EINVAL);
        refused("2^32 stripes", k, n, size_t(1) << 32, er.data(), nullptr, 0, RS_EINVAL);
        p.max_j = 3;
        CHECK(rsmi::plan_checks(k, n, 0, nullptr, nullptr, 0, kLay, &p) == RS_OK && empty(p), "stripes == 0");
    }
    // fixed-seed sweep against the model
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
        rsmi::CheckPlan p;
        const int rc = rsmi::plan_checks(kk, nn, stripes, er.data(), nullptr, 0, kLay, &p);
        CHECK(rc == RS_OK, "sweep %d: status %d", rep, rc);
        model("sweep", kk, nn, er, all(stripes), p);
        std::vector<uint32_t> list = {static_cast<uint32_t>(rnd() % stripes)};  // never empty: a NULL list means all
        for (size_t s = list[0] + 1; s < stripes; ++s)
            if (rnd() % 2) list.push_back(static_cast<uint32_t>(s));
        const int rl = rsmi::plan_checks(kk, nn, stripes, er.data(), list.data(), list.size(), kLay, &p);
        CHECK(rl == RS_OK, "sweep %d: list status %d", rep, rl);
        model("sweep list", kk, nn, er, list, p);
        // one stripe pushed past m: refused whatever came before it
        const size_t victim = rnd() % stripes;
        int e = 0;
        for (int id = 0; id < nn && e <= mm; ++id) e += er[victim * nn + id] != 0;
        for (int id = 0; id < nn && e <= mm; ++id)
            if (!er[victim * nn + id]) er[victim * nn + id] = 1, ++e;
        refused("sweep: too many", kk, nn, stripes, er.data(), nullptr, 0, RS_ENOT_ENOUGH);
    }
    std::printf("plan_checks: %d failures\n", failures);
    return failures ? 1 : 0;
}
"""


def test_plan_checks_standalone_sanitized(tmp_path):
    src = tmp_path / "check_plan_test.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "check_plan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", CSRC, str(src), os.path.join(CSRC, "check_plan.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "plan_checks: 0 failures" in run.stdout


def test_degraded_entry_points_are_exported():
    import rsmi
    lib = ctypes.CDLL(rsmi.LIB_PATH)
    for name in ("rs_verify_degraded", "rs_correct_degraded"):
        assert name in rsmi.EXPORTS
        assert hasattr(lib, name)
    assert (rsmi.FEC.STAT_CHECK_STRIPES, rsmi.FEC.STAT_SCRUB_REGENERATED) == (16, 17)
    assert hasattr(rsmi.FEC, "verify_degraded") and hasattr(rsmi.FEC, "correct_degraded")


def test_null_context_is_rejected_without_a_device():
    """Both calls refuse a NULL context with RS_EINVAL before touching HIP;
    callable on a CPU-only machine."""
    import rsmi
    lib = rsmi.load()
    flags = ctypes.create_string_buffer(14)
    fp = ctypes.cast(flags, ctypes.c_void_p)
    st = (ctypes.c_int * 1)()
    assert lib.rs_verify_degraded(None, None, 0, None, 0, 16, 16, 1, fp, None, None) == rsmi.RS_EINVAL
    assert lib.rs_verify_degraded(None, None, 0, None, 0, 16, 16, 0, None, None, None) == rsmi.RS_EINVAL
    assert lib.rs_correct_degraded(None, None, 0, None, 0, 16, 16, 1, fp, st, None, None) == rsmi.RS_EINVAL
    assert lib.rs_correct_degraded(None, None, 0, None, 0, 16, 16, 0, None, None, None, None) == rsmi.RS_EINVAL

// column_decode.cpp -- host side of rs_correct_columns: the per-erasure-set
// tables the kernel reads, and the host twin of its per-column decode.
#include "column_decode.hpp"

#include <cstring>
#include <vector>

#include "gf256.hpp"

namespace rsmi {

int column_tables(int n, const uint8_t* erased, uint8_t* out) {
    const Field& f = field();
    const size_t np = column_table_pitch(n);
    std::memset(out, 0, column_table_bytes(n));
    uint8_t* ids = out;
    uint8_t* x = out + np;
    uint8_t* u = out + 2 * np;
    uint8_t* W = out + 3 * np;
    int r = 0;
    for (int id = 0; id < n; ++id) {
        if (erased && erased[id]) continue;
        ids[r] = static_cast<uint8_t>(id);
        x[r] = eval_point(id);
        ++r;
    }
    for (int i = 0; i < r; ++i) {
        uint8_t prod = 1;
        for (int j = 0; j < r; ++j)
            if (j != i) prod = f.mul[prod][x[i] ^ x[j]];
        u[i] = f.inv[prod];
        uint8_t p = u[i];
        for (int t = 0; t < kColumnMaxSyn; ++t) {
            W[t * np + i] = p;
            p = f.mul[p][x[i]];
        }
    }
    return r;
}

int column_correct(int k, int n, const int* nums, uint8_t* ys, int r) {
    const Field& f = field();
    const int d = r - k;
    if (d <= 0) return 0;
    if (d > kColumnMaxSyn || n > 256) return -1;
    // The present set's tables, in the order of nums.
    std::vector<uint8_t> erased(n, 1), tab(column_table_bytes(n));
    for (int i = 0; i < r; ++i) erased[nums[i]] = 0;
    column_tables(n, erased.data(), tab.data());
    const size_t np = column_table_pitch(n);
    const uint8_t* ids = tab.data();
    const uint8_t* W = tab.data() + 3 * np;
    std::vector<int> at(n, -1);  // share number -> index into ys
    for (int i = 0; i < r; ++i) at[nums[i]] = i;
    uint8_t ws[kColumnWork] = {0};
    for (int t = 0; t < d; ++t) {
        uint8_t s = 0;
        for (int i = 0; i < r; ++i) s ^= f.mul[W[t * np + i]][ys[at[ids[i]]]];
        ws[kColumnWsS + t] = s;
    }
    const ColumnGf g{f.exp, f.log};
    const int nu = column_decode_core(g, tab.data() + np, tab.data() + 2 * np, r, d, ws);
    if (nu < 0) return -1;
    for (int a = 0; a < nu; ++a) ys[at[ids[ws[kColumnWsPos + a]]]] ^= ws[kColumnWsX + a];
    return nu;
}

}  // namespace rsmi

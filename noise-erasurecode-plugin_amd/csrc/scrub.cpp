// scrub.cpp -- see scrub.hpp.
#include "scrub.hpp"

#include "gf256.hpp"

namespace rsmi {

int scrub_locate(int k, int n, uint8_t* known, const uint8_t* ys) {
    if (k < 1 || n < k || n > 256 || !known || !ys) return -1;
    int nums[256];
    uint8_t recv[256], cw[256];
    int r = 0;
    for (int i = 0; i < n; ++i)
        if (!known[i]) {
            nums[r] = i;
            recv[r] = ys[i];
            ++r;
        }
    if (r - k < 2) return -1;  // radius 0: an error can be seen but not located
    if (bw_column(k, n, nums, recv, r, cw) < 0) return -1;
    int found = 0;
    for (int i = 0; i < r; ++i)
        if (cw[nums[i]] != recv[i]) {
            known[nums[i]] = 1;
            ++found;
        }
    return found;
}

}  // namespace rsmi

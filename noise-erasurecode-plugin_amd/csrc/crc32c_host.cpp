// crc32c_host.cpp -- rs_crc32c_host: the host reference of the sector
// checksums (CRC-32C, RFC 3720), slice-by-8.  No context, no HIP: callable on
// a machine without a GPU, like rs_blake2b_host.
#include <cstring>

#include "../../include/rsmi.h"
#include "crc32c_math.hpp"

namespace {

const rsmi::CrcTables kTab = rsmi::make_crc_tables();

uint32_t crc32c(const uint8_t* p, size_t len) {
    const auto& T = kTab.slice;
    uint32_t crc = 0xFFFFFFFFu;
    while (len >= 8) {
        uint32_t lo, hi;
        std::memcpy(&lo, p, 4);
        std::memcpy(&hi, p + 4, 4);
        lo ^= crc;
        crc = T[7][lo & 0xFFu] ^ T[6][(lo >> 8) & 0xFFu] ^ T[5][(lo >> 16) & 0xFFu] ^ T[4][lo >> 24] ^
              T[3][hi & 0xFFu] ^ T[2][(hi >> 8) & 0xFFu] ^ T[1][(hi >> 16) & 0xFFu] ^ T[0][hi >> 24];
        p += 8;
        len -= 8;
    }
    for (; len > 0; --len) crc = T[0][(crc ^ *p++) & 0xFFu] ^ (crc >> 8);
    return crc ^ 0xFFFFFFFFu;
}

}  // namespace

extern "C" int rs_crc32c_host(int count, const uint8_t* const* bufs, const size_t* lens, uint32_t* out) {
    if (count < 0) return RS_EINVAL;
    if (count == 0) return RS_OK;
    if (!bufs || !lens || !out) return RS_EINVAL;
    for (int i = 0; i < count; ++i)
        if (!bufs[i] && lens[i] > 0) return RS_EINVAL;
    for (int i = 0; i < count; ++i) out[i] = crc32c(bufs[i], lens[i]);
    return RS_OK;
}

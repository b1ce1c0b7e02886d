// scrub.hpp -- host-side locate step of rs_correct_stripes (the scrub of
// device-resident stripes): which shards of a stripe hold wrong bytes, from
// one inconsistent byte column.  Pure host code: no HIP, no context.
#pragma once

#include <cstdint>

namespace rsmi {

// One locate round for one stripe.  known[n]: shards already treated as erased.
// ys[n]: the stripe's bytes at one inconsistent column.
// Runs bw_column on the shares not in `known` (errors-and-erasures: radius
// floor((n - |known| - k) / 2)).
// Returns the number of newly located shards, set in known[], or -1 when there
// is no codeword in the radius or the radius is 0 (known[] is then unchanged).
int scrub_locate(int k, int n, uint8_t* known, const uint8_t* ys);

}  // namespace rsmi

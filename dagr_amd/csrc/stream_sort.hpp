// stream_sort.hpp -- what the stream's front stages (downsample.hip, stream_denoise.hip) share around the library's radix
// sort of (uint32 key, int32 arrival index) pairs: the number of key bits and the size of the sort's temporary storage.
#pragma once
#include "common.hpp"

#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>

namespace dagr {

// bits that hold every key up to and including `sentinel`
inline int key_bits(int64_t sentinel) {
    int bits = 1;
    while (bits < 32 && (sentinel >> bits) != 0) ++bits;
    return bits;
}

// the sort's temporary storage for a push of n events (0 if the library cannot say, e.g. without a device)
inline size_t sort_tmp_bytes(int64_t n, int bits) {
    size_t bytes = 0;
    if (rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr,
                                  (int32_t *)nullptr, (size_t)n, 0u, (unsigned)bits, (hipStream_t)0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return bytes;
}

// ... for every push of up to max_push events (at least 256 bytes).  The library picks its algorithm by size, so the
// largest push need not ask for the most: max_push and every power of two below it.
inline size_t sort_tmp_bytes_upto(int64_t max_push, int bits) {
    size_t bytes = 256;
    for (int64_t n = max_push; n >= 1; n = (n & (n - 1)) ? (int64_t)1 << (63 - __builtin_clzll((unsigned long long)n)) : n / 2)
        bytes = std::max(bytes, sort_tmp_bytes(n, bits));
    return bytes;
}

}  // namespace dagr

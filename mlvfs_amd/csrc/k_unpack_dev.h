// k_unpack_dev.h -- the bit-stream side of a packed MLV payload (mlvfs/raw.h:41-79), shared by the kernels that read one:
// k_unpack.hip, k_cal.hip and k_mlvpack.hip.  Pixel i is bits [i*bpp, (i+1)*bpp) of an MSB-first bit stream stored as little-endian 16-bit words.
#pragma once
#include "common.h"

namespace mlv {

// Swap the two 16-bit words of a little-endian dword: gives 32 stream bits in
// MSB-first order.
__device__ __forceinline__ uint32_t stream_word(uint32_t le_dword) { return (le_dword << 16) | (le_dword >> 16); }

// 16 pixels of BPP bits (BPP even) from BPP / 2 MSB-first 32-bit stream words
template <int BPP>
__device__ __forceinline__ void unpack_x16(const uint32_t (&s)[BPP / 2], uint32_t (&px)[16])
{
    constexpr uint32_t mask = (1u << BPP) - 1u;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int bit = BPP * k, wi = bit >> 5, sh = bit & 31;
        if (sh + BPP <= 32) {
            px[k] = (s[wi] >> (32 - BPP - sh)) & mask;
        } else {
            const uint64_t two = ((uint64_t)s[wi] << 32) | s[wi + 1];
            px[k] = (uint32_t)(two >> (64 - BPP - sh)) & mask;
        }
    }
}

}  // namespace mlv

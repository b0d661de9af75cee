// k_unpack_dev.h -- the bit-stream side of a packed MLV payload (mlvfs/raw.h:41-79), shared by the kernels that read one:
// k_unpack.hip, k_cal.hip and k_mlvpack.hip.  Pixel i is bits [i*bpp, (i+1)*bpp) of an MSB-first bit stream stored as little-endian 16-bit words.
// Also what their 16-pixels-per-lane ("x16") forms share: the lane's pixels as two 128-bit words, and the launchers' rule for taking that form.
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

// a lane's 16 pixels in registers <-> the two 128-bit words they are as 16-bit values in memory (pixel 2i low, 2i + 1 high, in dword i)
__device__ __forceinline__ void join_x16(const uint32_t (&px)[16], uint4 &lo, uint4 &hi)
{
    lo.x = px[0] | (px[1] << 16);   lo.y = px[2] | (px[3] << 16);
    lo.z = px[4] | (px[5] << 16);   lo.w = px[6] | (px[7] << 16);
    hi.x = px[8] | (px[9] << 16);   hi.y = px[10] | (px[11] << 16);
    hi.z = px[12] | (px[13] << 16); hi.w = px[14] | (px[15] << 16);
}

__device__ __forceinline__ void split_x16(uint4 lo, uint4 hi, uint32_t (&px)[16])
{
    const uint32_t in[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
#pragma unroll
    for (int i = 0; i < 8; i++) { px[2 * i] = in[i] & 0xFFFFu; px[2 * i + 1] = in[i] >> 16; }
}

// ---- the host side of the x16 forms -------------------------------------------------------------------------------------------
// the depths of ML's raw video: the only ones the x16 kernels are instantiated for
inline bool fast_depth(int bpp) { return bpp == 14 || bpp == 12 || bpp == 10; }

// What every x16 form asks of a batch: whole groups of 16 pixels, and both buffers aligned for the lane's accesses -- 16 bytes where
// 16-bit frames move as 128-bit words, 4 where a packed stream moves as dwords.  A stride counts only where a second frame exists.
inline bool fits_x16(uint32_t npix, int nframes, const void *in, size_t in_stride, size_t in_align, const void *out, size_t out_stride, size_t out_align)
{
    return npix % 16 == 0 && (uintptr_t)in % in_align == 0 && (uintptr_t)out % out_align == 0 &&
           (nframes == 1 || (in_stride % in_align == 0 && out_stride % out_align == 0));
}

// blocks of 256 lanes for `items` grid-stride items, `cap` at the most
inline uint32_t grid_x(uint32_t items, uint32_t cap) { const uint32_t n = (items + 255) / 256; return n < cap ? n : cap; }

}  // namespace mlv

// k_unpack.hip -- packed MLV payload -> 16-bit pixels (replaces the loop of
// dng_get_image_data_inline, mlvfs/dng.c:813-843).
//
// Format (mlvfs/raw.h:41-79): pixel i is bits [i*bpp, (i+1)*bpp) of an MSB-first
// bit stream stored as little-endian 16-bit words.
//
// HBM-bound: 14/8 B read + 2 B written per pixel = 3.75 B/px.
//   k_unpack_x16<14 | 12 | 10> : one lane = 16 pixels = 7 / 6 / 5 coalesced dword loads
//                (always 4-byte aligned: 16 px * bpp bits) and two 128-bit stores.
//                Frames are batched in grid.y.
//   k_unpack_generic : any bpp in 1..16, any length; one lane = one pixel.
#include "clip.h"
#include "k_unpack_dev.h"

namespace mlv {

// one lane = 16 pixels = BPP / 2 coalesced dword loads (always 4-byte aligned: 16 px * BPP bits) and two 128-bit stores:
// 14 bits, and the reduced depths of ML's raw video (12, 10), which took the pixel-per-lane kernel until the end of round 3
template <int BPP>
__global__ __launch_bounds__(256) void k_unpack_x16(const uint8_t *__restrict__ packed, size_t packed_stride,
                                                    uint8_t *__restrict__ out, size_t out_stride, uint32_t groups)
{
    constexpr int NW = BPP / 2;
    const uint32_t *src = (const uint32_t *)(packed + (size_t)blockIdx.y * packed_stride);
    uint4 *dst = (uint4 *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint32_t s[NW], px[16];
#pragma unroll
        for (int i = 0; i < NW; i++) s[i] = stream_word(src[(size_t)g * NW + i]);
        unpack_x16<BPP>(s, px);
        uint4 lo, hi;
        join_x16(px, lo, hi);
        dst[(size_t)g * 2] = lo;
        dst[(size_t)g * 2 + 1] = hi;
    }
}

__global__ __launch_bounds__(256) void k_unpack_generic(const uint8_t *__restrict__ packed, size_t packed_stride,
                                                        uint8_t *__restrict__ out, size_t out_stride,
                                                        uint32_t first_px, uint32_t npix, int bpp)
{
    const uint16_t *src = (const uint16_t *)(packed + (size_t)blockIdx.y * packed_stride);
    uint16_t *dst = (uint16_t *)(out + (size_t)blockIdx.y * out_stride);
    const uint32_t mask = (1u << bpp) - 1u;
    const uint32_t first_word = first_px * (uint32_t)bpp / 16;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x) {
        const uint32_t bit = (first_px + k) * (uint32_t)bpp;
        const uint32_t wi = bit / 16 - first_word, sh = bit % 16;
        const uint32_t two = ((uint32_t)src[wi] << 16) | src[wi + 1];
        dst[k] = (uint16_t)((two >> (32 - bpp - sh)) & mask);
    }
}

// host launcher: d_packed points at the word that holds the first requested pixel
int launch_unpack(const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride, uint32_t first_px,
                  uint32_t npix, int bpp, int nframes, hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    if (bpp < 1 || bpp > 16) { set_error("unsupported bits_per_pixel %d", bpp); return MLVFS_AMD_ERR_ARG; }
    if (fast_depth(bpp) && first_px == 0 && fits_x16(npix, nframes, d_packed, packed_stride, 4, d_out, out_stride, 16)) {
        const uint32_t groups = npix / 16;
        auto kern = bpp == 14 ? k_unpack_x16<14> : (bpp == 12 ? k_unpack_x16<12> : k_unpack_x16<10>);
        hipLaunchKernelGGL(kern, dim3(grid_x(groups, 8192), nframes), dim3(256), 0, stream, (const uint8_t *)d_packed, packed_stride,
                           (uint8_t *)d_out, out_stride, groups);
    } else {
        hipLaunchKernelGGL(k_unpack_generic, dim3(grid_x(npix, 16384), nframes), dim3(256), 0, stream, (const uint8_t *)d_packed, packed_stride,
                           (uint8_t *)d_out, out_stride, first_px, npix, bpp);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}


// the first launch of any kernel of this file loads the file's code object (HIP loads them lazily): the device context asks for a
// kernel's attributes when it is created, so that a clip's first frame does not pay for it (runtime.cpp: get_device)
void preload_k_unpack() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)k_unpack_x16<14>); (void)hipGetLastError(); }

}  // namespace mlv

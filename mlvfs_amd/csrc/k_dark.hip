// k_dark.hip -- dark-frame subtraction and dark-frame averaging on 16-bit frames in HBM (csrc/dark.cpp).
//
// The reference has no dark-frame code; the definition is this project's (what `mlv_dump -s` / `-a` do a frame at a time on a host
// core).  A dark frame is a plane of w x h 16-bit values with a pedestal black_d, the black level of the clip it was averaged from:
//     out     = clamp(px - dark + black_d, 0, 2^bpp - 1)                     in 32-bit signed arithmetic
//     dark[p] = (sum over the n frames of px_f[p] + n / 2) / n               32-bit unsigned sums, n <= 65536: no overflow
// The plane is applied by position in the stored frame (xRes x yRes): the frame's panPosX/Y and cropPosX/Y are ignored.
//
// All HBM-bound.  One lane moves 16 bytes per load; the lanes of a wave are contiguous; frames are batched in grid.y.  The dark plane
// is read by every frame of a batch (9.5 MB at 3584x1320: it stays in the last-level cache).
//   k_dark_sub_x16       in place; one lane = 16 pixels (two runs of 8, half a frame apart) = two 128-bit loads of the frame, two of
//                        the plane, two 128-bit stores, each contiguous across the wave
//   k_dark_sub_generic   any size, 2-byte alignment; one lane = one pixel
//   k_dark_unpack_x16<14 | 12 | 10>   k_unpack_x16's unpack and the subtraction in one pass: packed stream in, subtracted frames out
//   k_dark_accum_x16 / k_dark_accum_generic   a batch of frames added to a uint32 plane: a lane owns its pixels, walks the batch's frames
//                        with the sums in registers and makes one read-modify-write of the plane
//   k_dark_mean          the rounded mean of the sums as 16-bit values
// Pad bytes between frames are never touched.
#include "clip.h"
#include "k_unpack_dev.h"

namespace mlv {

__device__ __forceinline__ uint32_t dark_px(uint32_t px, uint32_t dk, int black_d, int top)
{
    const int v = (int)px - (int)dk + black_d;
    return (uint32_t)min(max(v, 0), top);
}

// two pixels in a dword
__device__ __forceinline__ uint32_t dark_px2(uint32_t p, uint32_t d, int black_d, int top)
{
    return dark_px(p & 0xFFFFu, d & 0xFFFFu, black_d, top) | (dark_px(p >> 16, d >> 16, black_d, top) << 16);
}

__device__ __forceinline__ uint4 dark_px8(uint4 p, uint4 d, int black_d, int top)
{
    uint4 r;
    r.x = dark_px2(p.x, d.x, black_d, top); r.y = dark_px2(p.y, d.y, black_d, top);
    r.z = dark_px2(p.z, d.z, black_d, top); r.w = dark_px2(p.w, d.w, black_d, top);
    return r;
}

// a lane's 16 pixels are two runs of 8, `groups` runs apart: the lanes of a wave are 16 bytes apart in every load and store
__global__ __launch_bounds__(256) void k_dark_sub_x16(uint8_t *__restrict__ frames, size_t stride, const uint4 *__restrict__ dark,
                                                      uint32_t groups, int black_d, int top)
{
    uint4 *f = (uint4 *)(frames + (size_t)blockIdx.y * stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        const uint4 a = f[g], b = f[(size_t)g + groups];
        const uint4 da = dark[g], db = dark[(size_t)g + groups];
        f[g] = dark_px8(a, da, black_d, top);
        f[(size_t)g + groups] = dark_px8(b, db, black_d, top);
    }
}

__global__ __launch_bounds__(256) void k_dark_sub_generic(uint8_t *__restrict__ frames, size_t stride, const uint16_t *__restrict__ dark,
                                                          uint32_t npix, int black_d, int top)
{
    uint16_t *f = (uint16_t *)(frames + (size_t)blockIdx.y * stride);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x)
        f[k] = (uint16_t)dark_px(f[k], dark[k], black_d, top);
}

template <int BPP>
__global__ __launch_bounds__(256) void k_dark_unpack_x16(const uint8_t *__restrict__ packed, size_t packed_stride, uint8_t *__restrict__ out,
                                                         size_t out_stride, const uint4 *__restrict__ dark, uint32_t groups, int black_d)
{
    constexpr int NW = BPP / 2;
    constexpr int top = (1 << BPP) - 1;
    const uint32_t *src = (const uint32_t *)(packed + (size_t)blockIdx.y * packed_stride);
    uint4 *dst = (uint4 *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint32_t s[NW], px[16];
#pragma unroll
        for (int i = 0; i < NW; i++) s[i] = stream_word(src[(size_t)g * NW + i]);
        const uint4 da = dark[(size_t)g * 2], db = dark[(size_t)g * 2 + 1];
        unpack_x16<BPP>(s, px);
        uint4 lo, hi;
        lo.x = px[0] | (px[1] << 16);   lo.y = px[2] | (px[3] << 16);
        lo.z = px[4] | (px[5] << 16);   lo.w = px[6] | (px[7] << 16);
        hi.x = px[8] | (px[9] << 16);   hi.y = px[10] | (px[11] << 16);
        hi.z = px[12] | (px[13] << 16); hi.w = px[14] | (px[15] << 16);
        dst[(size_t)g * 2] = dark_px8(lo, da, black_d, top);
        dst[(size_t)g * 2 + 1] = dark_px8(hi, db, black_d, top);
    }
}

__device__ __forceinline__ void add_px8(uint4 (&s)[2], uint4 p)
{
    s[0].x += p.x & 0xFFFFu; s[0].y += p.x >> 16; s[0].z += p.y & 0xFFFFu; s[0].w += p.y >> 16;
    s[1].x += p.z & 0xFFFFu; s[1].y += p.z >> 16; s[1].z += p.w & 0xFFFFu; s[1].w += p.w >> 16;
}

// sums: one uint32 per pixel; the lane's 16 sums are four 128-bit words
__global__ __launch_bounds__(256) void k_dark_accum_x16(const uint8_t *__restrict__ frames, size_t stride, int nframes, uint4 *__restrict__ sums,
                                                        uint32_t groups)
{
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint4 lo[2], hi[2];
        lo[0] = sums[(size_t)g * 4];     lo[1] = sums[(size_t)g * 4 + 1];
        hi[0] = sums[(size_t)g * 4 + 2]; hi[1] = sums[(size_t)g * 4 + 3];
        for (int f = 0; f < nframes; f++) {
            const uint4 *src = (const uint4 *)(frames + (size_t)f * stride);
            add_px8(lo, src[(size_t)g * 2]);
            add_px8(hi, src[(size_t)g * 2 + 1]);
        }
        sums[(size_t)g * 4] = lo[0];     sums[(size_t)g * 4 + 1] = lo[1];
        sums[(size_t)g * 4 + 2] = hi[0]; sums[(size_t)g * 4 + 3] = hi[1];
    }
}

__global__ __launch_bounds__(256) void k_dark_accum_generic(const uint8_t *__restrict__ frames, size_t stride, int nframes,
                                                            uint32_t *__restrict__ sums, uint32_t npix)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x) {
        uint32_t s = sums[k];
        for (int f = 0; f < nframes; f++) s += ((const uint16_t *)(frames + (size_t)f * stride))[k];
        sums[k] = s;
    }
}

// n in 1..65536: sums[k] + n / 2 < 2^32
__global__ __launch_bounds__(256) void k_dark_mean(const uint32_t *__restrict__ sums, uint16_t *__restrict__ dark, uint32_t npix, uint32_t n)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x)
        dark[k] = (uint16_t)((sums[k] + n / 2) / n);
}

static uint32_t dark_grid_x(uint32_t items, uint32_t cap) { return std::min<uint32_t>((items + 255) / 256, cap); }

// the plane is the library's own allocation (16-byte aligned); the callers have checked the geometry
int launch_dark_sub(void *d_frames, size_t stride, uint32_t npix, int nframes, const DarkFrameDev &dark, hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    const bool fast = npix % 16 == 0 && ((uintptr_t)d_frames % 16 == 0) && ((uintptr_t)dark.d_plane % 16 == 0) && (nframes == 1 || stride % 16 == 0);
    if (fast) {
        const uint32_t groups = npix / 16;
        const dim3 grid(dark_grid_x(groups, 8192), nframes);
        hipLaunchKernelGGL(k_dark_sub_x16, grid, dim3(256), 0, stream, (uint8_t *)d_frames, stride, (const uint4 *)dark.d_plane, groups, dark.black,
                           dark.top);
    } else {
        const dim3 grid(dark_grid_x(npix, 16384), nframes);
        hipLaunchKernelGGL(k_dark_sub_generic, grid, dim3(256), 0, stream, (uint8_t *)d_frames, stride, dark.d_plane, npix, dark.black, dark.top);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// packed payloads -> subtracted 16-bit frames: one pass where k_unpack_x16 would run, else launch_unpack + launch_dark_sub
int launch_dark_unpack(const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride, uint32_t npix, int bpp, int nframes,
                       const DarkFrameDev &dark, hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    const bool fast = (bpp == 14 || bpp == 12 || bpp == 10) && dark.top == (1 << bpp) - 1 && npix % 16 == 0 && ((uintptr_t)d_packed % 4 == 0) &&
                      ((uintptr_t)d_out % 16 == 0) && ((uintptr_t)dark.d_plane % 16 == 0) &&
                      (nframes == 1 || (packed_stride % 4 == 0 && out_stride % 16 == 0));
    if (!fast) {
        if (int rc = launch_unpack(d_packed, packed_stride, d_out, out_stride, 0, npix, bpp, nframes, stream)) return rc;
        return launch_dark_sub(d_out, out_stride, npix, nframes, dark, stream);
    }
    const uint32_t groups = npix / 16;
    const dim3 grid(dark_grid_x(groups, 8192), nframes);
    auto kern = bpp == 14 ? k_dark_unpack_x16<14> : (bpp == 12 ? k_dark_unpack_x16<12> : k_dark_unpack_x16<10>);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, (const uint8_t *)d_packed, packed_stride, (uint8_t *)d_out, out_stride,
                       (const uint4 *)dark.d_plane, groups, dark.black);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// d_sums: npix uint32, 16-byte aligned (the library's own allocation)
int launch_dark_accum(const void *d_frames, size_t stride, uint32_t npix, int nframes, uint32_t *d_sums, hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    const bool fast = npix % 16 == 0 && ((uintptr_t)d_frames % 16 == 0) && ((uintptr_t)d_sums % 16 == 0) && (nframes == 1 || stride % 16 == 0);
    if (fast) {
        const uint32_t groups = npix / 16;
        hipLaunchKernelGGL(k_dark_accum_x16, dim3(dark_grid_x(groups, 8192)), dim3(256), 0, stream, (const uint8_t *)d_frames, stride, nframes,
                           (uint4 *)d_sums, groups);
    } else {
        hipLaunchKernelGGL(k_dark_accum_generic, dim3(dark_grid_x(npix, 16384)), dim3(256), 0, stream, (const uint8_t *)d_frames, stride, nframes,
                           d_sums, npix);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

int launch_dark_mean(const uint32_t *d_sums, uint16_t *d_dark, uint32_t npix, uint32_t n, hipStream_t stream)
{
    if (npix == 0) return MLVFS_AMD_OK;
    if (n < 1 || n > 65536) { set_error("dark: a mean of %u frames", n); return MLVFS_AMD_ERR_ARG; }
    hipLaunchKernelGGL(k_dark_mean, dim3(dark_grid_x(npix, 16384)), dim3(256), 0, stream, d_sums, d_dark, npix, n);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

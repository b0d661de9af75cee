// k_proxy.hip -- half-size Bayer proxies: the frames the mount serves, binned 2x2 within each colour of the CFA (include/mlvfs_amd.h,
// "half-size Bayer proxies").  A W x H frame becomes W' x H' = 2 * (W / 4) x 2 * (H / 4); output pixel (Y, X) is
//     (in(y0, x0) + in(y0, x0 + 2) + in(y0 + 2, x0) + in(y0 + 2, x0 + 2) + 2) >> 2,    y0 = 4 * (Y >> 1) + (Y & 1),  x0 = 4 * (X >> 1) + (X & 1)
// summed in 32 bits (four times 65535 plus 2 takes 18).  Columns and rows behind the last whole 4x4 block are never read.
//
// One element-wise pass, HBM-bound: 2 B read per source pixel, 0.5 B written.  Frames are batched in grid.y, the lanes of a wave are
// contiguous in the source and in the destination, no LDS, no scratch, never in place.
//   k_bin2_x16     : W % 16 == 0, bases and strides 16-byte aligned.  One lane = 16 consecutive pixels (two 128-bit loads) of each of
//                    the four rows of one block row; rows 0 and 2 make 8 pixels of output row 2r, rows 1 and 3 make 8 of row 2r + 1:
//                    two 128-bit stores.  The even and odd halves of a dword are the two column parities, and the two dwords of a
//                    block add half by half.  A wave reads 2 KiB contiguous from each of four rows and writes 1 KiB to each of two.
//   k_bin2_generic : any W, H >= 4, 2-byte alignment; one lane = one output pixel.
// Bytes between frames and behind W' * H' * 2 are never touched.
#include "clip.h"

namespace mlv {

// dwords a0, a1 (row y0) and b0, b1 (row y0 + 2) of one 4-pixel block -> the block's two output pixels of that row parity
__device__ __forceinline__ uint32_t bin2_block(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1)
{
    const uint32_t even = (a0 & 0xFFFFu) + (a1 & 0xFFFFu) + (b0 & 0xFFFFu) + (b1 & 0xFFFFu) + 2u;
    const uint32_t odd = (a0 >> 16) + (a1 >> 16) + (b0 >> 16) + (b1 >> 16) + 2u;
    return (even >> 2) | ((odd >> 2) << 16);
}

// 16 pixels of rows y0 and y0 + 2 -> 8 output pixels
__device__ __forceinline__ uint4 bin2_rows(const uint4 &a_lo, const uint4 &a_hi, const uint4 &b_lo, const uint4 &b_hi)
{
    uint4 o;
    o.x = bin2_block(a_lo.x, a_lo.y, b_lo.x, b_lo.y);
    o.y = bin2_block(a_lo.z, a_lo.w, b_lo.z, b_lo.w);
    o.z = bin2_block(a_hi.x, a_hi.y, b_hi.x, b_hi.y);
    o.w = bin2_block(a_hi.z, a_hi.w, b_hi.z, b_hi.w);
    return o;
}

// groups = W / 16 * (H / 4) per frame: block rows in order, 16-pixel groups of a row in order.  row16 = W / 8: uint4s per source row.
__global__ __launch_bounds__(256) void k_bin2_x16(const uint8_t *__restrict__ frames, size_t stride, uint8_t *__restrict__ out, size_t out_stride,
                                                  uint32_t groups, uint32_t groups_per_row, uint32_t row16)
{
    const uint4 *src = (const uint4 *)(frames + (size_t)blockIdx.y * stride);
    uint4 *dst = (uint4 *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        const uint32_t br = g / groups_per_row, gx = g - br * groups_per_row;
        const uint4 *p = src + (size_t)br * 4 * row16 + (size_t)gx * 2;
        const uint4 r0l = p[0], r0h = p[1];
        const uint4 r1l = p[row16], r1h = p[row16 + 1];
        const uint4 r2l = p[2 * (size_t)row16], r2h = p[2 * (size_t)row16 + 1];
        const uint4 r3l = p[3 * (size_t)row16], r3h = p[3 * (size_t)row16 + 1];
        // an output row is W' = W / 2 pixels = groups_per_row uint4s
        uint4 *q = dst + (size_t)br * 2 * groups_per_row + gx;
        q[0] = bin2_rows(r0l, r0h, r2l, r2h);
        q[groups_per_row] = bin2_rows(r1l, r1h, r3l, r3h);
    }
}

// npix = W' * H' output pixels per frame
__global__ __launch_bounds__(256) void k_bin2_generic(const uint8_t *__restrict__ frames, size_t stride, uint8_t *__restrict__ out,
                                                      size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw)
{
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint16_t *dst = (uint16_t *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x) {
        const uint32_t Y = k / pw, X = k - Y * pw;
        const uint32_t y0 = 4u * (Y >> 1) + (Y & 1u), x0 = 4u * (X >> 1) + (X & 1u);
        const uint16_t *p = src + (size_t)y0 * w + x0;
        const uint32_t sum = (uint32_t)p[0] + p[2] + p[2 * (size_t)w] + p[2 * (size_t)w + 2] + 2u;
        dst[k] = (uint16_t)(sum >> 2);
    }
}

// d_out != d_frames, the ranges apart (the callers check); w, h >= 4
int launch_bin2(const void *d_frames, size_t stride, void *d_out, size_t out_stride, int w, int h, int nframes, hipStream_t stream)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    int pw, ph;
    if (!proxy_geom(w, h, &pw, &ph)) { set_error("a proxy takes frames of 4x4 up to 2^27 pixels, not %dx%d", w, h); return MLVFS_AMD_ERR_ARG; }
    const bool fast = w % 16 == 0 && ((uintptr_t)d_frames % 16 == 0) && ((uintptr_t)d_out % 16 == 0) &&
                      (nframes == 1 || (stride % 16 == 0 && out_stride % 16 == 0));
    if (fast) {
        const uint32_t gpr = (uint32_t)w / 16, groups = gpr * (uint32_t)(h / 4);
        hipLaunchKernelGGL(k_bin2_x16, dim3(std::min<uint32_t>((groups + 255) / 256, 8192), nframes), dim3(256), 0, stream,
                           (const uint8_t *)d_frames, stride, (uint8_t *)d_out, out_stride, groups, gpr, (uint32_t)w / 8);
    } else {
        const uint32_t npix = (uint32_t)pw * (uint32_t)ph;
        hipLaunchKernelGGL(k_bin2_generic, dim3(std::min<uint32_t>((npix + 255) / 256, 16384), nframes), dim3(256), 0, stream,
                           (const uint8_t *)d_frames, stride, (uint8_t *)d_out, out_stride, npix, (uint32_t)w, (uint32_t)pw);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

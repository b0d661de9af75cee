// k_render.hip -- rendered half-size sRGB frames: the frames the mount serves, developed to 8-bit RGB at half size (include/mlvfs_amd.h,
// "rendered half-size sRGB frames").  A W x H RGGB frame becomes W' x H' = W / 2 x H / 2 pixels of 3 bytes; per pixel
//     c0 = in(2Y, 2X)   c1 = (in(2Y, 2X + 1) + in(2Y + 1, 2X) + 1) >> 1   c2 = in(2Y + 1, 2X + 1)        c'_j = max(c_j - black, 0)
//     n_j = min((c'_j * A_j + 2048) >> 12, 65535)                                                        (the product in 64 bits)
//     t_i = clamp((sum_j K[i][j] * n_j + 32768) >> 16, 0, 4095)                                          (64 bits, signed; floor)
//     out_i = LUT[t_i]
// black, A[3], K[9]: 13 int32 per frame in a device array (mlvfs_amd_rgb_params), uniform in a workgroup and read with scalar loads.
//
// One element-wise pass: 2 B read per source pixel, 0.75 B written.  Frames are batched in grid.y, the lanes of a wave are contiguous
// in the source and in the destination, never in place, no scratch; the 4 KiB LUT is staged once per workgroup in LDS (one 128-bit
// load and store per lane) and gathered from by bytes.  The launch caps the workgroups per frame and the lanes stride over the rest,
// so a batch stages the table some two thousand times, not once per 4096 source pixels.
//   k_render2_x16     : W % 16 == 0, source base and stride 16-byte, destination base and stride 8-byte aligned.  One lane = 16 pixels
//                       (two 128-bit loads) of each of the two rows of a superpixel row = 8 output pixels = 24 bytes: three 64-bit
//                       stores.  Output rows have no padding, so group g of a frame lies at byte 24 g: a wave reads 2 KiB contiguous
//                       from each of two rows and writes 1.5 KiB contiguous.
//   k_render2_generic : any W, H >= 2, 2-byte source alignment, 1-byte destination alignment; one lane = one output pixel.
// Bytes between frames and behind 3 * W' * H' are never touched.
#include "clip.h"

#define MLV_SRGB_LUT12_ATTR __device__ __attribute__((aligned(16)))          // stage_lut reads it in 16-byte pieces
#include "srgb_lut12.h"

namespace mlv {

struct RenderParams {          // mlvfs_amd_rgb_params' out[13]
    int32_t black, A[3], K[9];
};

// 256 lanes x 16 bytes
__device__ __forceinline__ void stage_lut(uint8_t *lut)
{
    ((uint4 *)lut)[threadIdx.x] = ((const uint4 *)kSrgbLut12)[threadIdx.x];
    __syncthreads();
}

// what max(c - black, 0) needs for any int32 black with c < 2^16: c' = sat(c + lift - drop) in 32 bits unsigned
struct Black {
    uint32_t lift, drop;
    __device__ explicit Black(int32_t black) : lift(black < 0 ? 0u - (uint32_t)black : 0u), drop(black > 0 ? (uint32_t)black : 0u) {}
    __device__ __forceinline__ uint32_t operator()(uint32_t c) const { const uint32_t v = c + lift; return v > drop ? v - drop : 0u; }
};

__device__ __forceinline__ uint32_t balance(uint32_t c, int32_t A)
{
    const uint64_t v = ((uint64_t)c * (uint32_t)A + 2048u) >> 12;
    return v < 65535u ? (uint32_t)v : 65535u;
}

__device__ __forceinline__ uint32_t tone_index(const int32_t *K, uint32_t n0, uint32_t n1, uint32_t n2)
{
    const int64_t acc = (int64_t)K[0] * (int32_t)n0 + (int64_t)K[1] * (int32_t)n1 + (int64_t)K[2] * (int32_t)n2 + 32768;
    const int64_t t = acc >> 16;
    return t < 0 ? 0u : t > 4095 ? 4095u : (uint32_t)t;
}

// the three bytes of one output pixel in bits 0 .. 23: R, G, B from the low byte up
__device__ __forceinline__ uint32_t develop(uint32_t c0, uint32_t gsum, uint32_t c2, const Black &bl, const RenderParams &p, const uint8_t *lut)
{
    const uint32_t n0 = balance(bl(c0), p.A[0]), n1 = balance(bl((gsum + 1u) >> 1), p.A[1]), n2 = balance(bl(c2), p.A[2]);
    const uint32_t r = lut[tone_index(p.K, n0, n1, n2)], g = lut[tone_index(p.K + 3, n0, n1, n2)], b = lut[tone_index(p.K + 6, n0, n1, n2)];
    return r | (g << 8) | (b << 16);
}

// a dword of row 2Y (R low, G high) and the one below it (G low, B high) -> one output pixel
__device__ __forceinline__ uint32_t develop2(uint32_t top, uint32_t bot, const Black &bl, const RenderParams &p, const uint8_t *lut)
{
    return develop(top & 0xFFFFu, (top >> 16) + (bot & 0xFFFFu), bot >> 16, bl, p, lut);
}

// groups = W / 16 * H' per frame: superpixel rows in order, 16-pixel groups of a row in order.  row16 = W / 8: uint4s per source row.
__global__ __launch_bounds__(256) void k_render2_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                     uint8_t *__restrict__ out, size_t out_stride, uint32_t groups, uint32_t groups_per_row,
                                                     uint32_t row16)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[4096];
    stage_lut(lut);
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const uint4 *src = (const uint4 *)(frames + (size_t)blockIdx.y * stride);
    uint2 *dst = (uint2 *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        const uint32_t Y = g / groups_per_row, gx = g - Y * groups_per_row;
        const uint4 *q = src + (size_t)Y * 2 * row16 + (size_t)gx * 2;
        const uint4 tl = q[0], th = q[1], lo = q[row16], hi = q[row16 + 1];          // top and lower row, 8 pixels each
        const uint32_t p0 = develop2(tl.x, lo.x, bl, p, lut), p1 = develop2(tl.y, lo.y, bl, p, lut);
        const uint32_t p2 = develop2(tl.z, lo.z, bl, p, lut), p3 = develop2(tl.w, lo.w, bl, p, lut);
        const uint32_t p4 = develop2(th.x, hi.x, bl, p, lut), p5 = develop2(th.y, hi.y, bl, p, lut);
        const uint32_t p6 = develop2(th.z, hi.z, bl, p, lut), p7 = develop2(th.w, hi.w, bl, p, lut);
        // four pixels of 24 bits are three dwords
        uint2 *o = dst + (size_t)g * 3;
        o[0] = make_uint2(p0 | (p1 << 24), (p1 >> 8) | (p2 << 16));
        o[1] = make_uint2((p2 >> 16) | (p3 << 8), p4 | (p5 << 24));
        o[2] = make_uint2((p5 >> 8) | (p6 << 16), (p6 >> 16) | (p7 << 8));
    }
}

// npix = W' * H' output pixels per frame
__global__ __launch_bounds__(256) void k_render2_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                         uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[4096];
    stage_lut(lut);
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x) {
        const uint32_t Y = k / pw, X = k - Y * pw;
        const uint16_t *q = src + (size_t)Y * 2 * w + (size_t)X * 2;
        const uint32_t v = develop(q[0], (uint32_t)q[1] + q[w], q[(size_t)w + 1], bl, p, lut);
        uint8_t *o = dst + (size_t)k * 3;
        o[0] = (uint8_t)v;
        o[1] = (uint8_t)(v >> 8);
        o[2] = (uint8_t)(v >> 16);
    }
}

static_assert(sizeof(RenderParams) == 13 * sizeof(int32_t), "mlvfs_amd_rgb_params' layout");

// d_out apart from d_frames (the callers check); w, h >= 2; d_params: 13 int32 per frame, 4-byte aligned
int launch_render2(const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h, int nframes,
                   hipStream_t stream)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    int pw, ph;
    if (!rgb_geom(w, h, &pw, &ph)) { set_error("a rendering takes frames of 2x2 up to 2^27 pixels, not %dx%d", w, h); return MLVFS_AMD_ERR_ARG; }
    const bool fast = w % 16 == 0 && ((uintptr_t)d_frames % 16 == 0) && ((uintptr_t)d_out % 8 == 0) &&
                      (nframes == 1 || (stride % 16 == 0 && out_stride % 8 == 0));
    // the workgroups of a launch share the machine: some two thousand of them in all, each of which stages the table once
    const uint32_t cap = std::max(2048u / (uint32_t)nframes, 64u);
    if (fast) {
        const uint32_t gpr = (uint32_t)w / 16, groups = gpr * (uint32_t)ph;
        hipLaunchKernelGGL(k_render2_x16, dim3(std::min<uint32_t>((groups + 255) / 256, cap), nframes), dim3(256), 0, stream,
                           (const uint8_t *)d_frames, stride, (const RenderParams *)d_params, (uint8_t *)d_out, out_stride, groups, gpr, (uint32_t)w / 8);
    } else {
        const uint32_t npix = (uint32_t)pw * (uint32_t)ph;
        hipLaunchKernelGGL(k_render2_generic, dim3(std::min<uint32_t>((npix + 255) / 256, 4 * cap), nframes), dim3(256), 0, stream,
                           (const uint8_t *)d_frames, stride, (const RenderParams *)d_params, (uint8_t *)d_out, out_stride, npix, (uint32_t)w, (uint32_t)pw);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

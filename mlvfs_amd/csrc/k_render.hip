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
// k_render2_look_x16, k_render2_look_generic: the same bodies with a look as step 4 (k_tone_dev.h); k_look_apply: that step alone.
// k_render2_deep_x16, k_render2_deep_generic: the same bodies with the 16-bit form of steps 3 and 4 and 6 bytes per pixel -- a lane of
// the x16 form writes 48 bytes as three 128-bit stores, so its destination base and stride are 16-byte aligned (one that is only 8-byte
// aligned takes the generic kernel); no table in LDS, no barrier.  k_look16_apply: that step 4 alone.
#include "k_tone_dev.h"

namespace mlv {

// one output pixel as tone() gives it: the three bytes in bits 0 .. 23, R, G, B from the low byte up; deep: the three 16-bit samples
template <Tone TN>
__device__ __forceinline__ auto develop(uint32_t c0, uint32_t gsum, uint32_t c2, const Black &bl, const RenderParams &p, const uint8_t *lut,
                                            const LookArg &lk)
{
    const uint32_t n0 = balance(bl(c0), p.A[0]), n1 = balance(bl((gsum + 1u) >> 1), p.A[1]), n2 = balance(bl(c2), p.A[2]);
    return tone<false, TN>(p, lut, lk, n0, n1, n2);
}

// a dword of row 2Y (R low, G high) and the one below it (G low, B high) -> one output pixel
template <Tone TN>
__device__ __forceinline__ auto develop2(uint32_t top, uint32_t bot, const Black &bl, const RenderParams &p, const uint8_t *lut, const LookArg &lk)
{
    return develop<TN>(top & 0xFFFFu, (top >> 16) + (bot & 0xFFFFu), bot >> 16, bl, p, lut, lk);
}

// groups = W / 16 * H' per frame: superpixel rows in order, 16-pixel groups of a row in order.  row16 = W / 8: uint4s per source row.
template <Tone TN>
__device__ __forceinline__ void render2_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                            uint8_t *__restrict__ out, size_t out_stride, uint32_t groups, uint32_t groups_per_row, uint32_t row16,
                                            uint8_t *lut, const LookArg &lk, uint32_t first, uint32_t step)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const uint4 *src = (const uint4 *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    for (uint32_t g = first; g < groups; g += step) {
        const uint32_t Y = g / groups_per_row, gx = g - Y * groups_per_row;
        const uint4 *q = src + (size_t)Y * 2 * row16 + (size_t)gx * 2;
        const uint4 tl = q[0], th = q[1], lo = q[row16], hi = q[row16 + 1];          // top and lower row, 8 pixels each
        const auto p0 = develop2<TN>(tl.x, lo.x, bl, p, lut, lk), p1 = develop2<TN>(tl.y, lo.y, bl, p, lut, lk);
        const auto p2 = develop2<TN>(tl.z, lo.z, bl, p, lut, lk), p3 = develop2<TN>(tl.w, lo.w, bl, p, lut, lk);
        const auto p4 = develop2<TN>(th.x, hi.x, bl, p, lut, lk), p5 = develop2<TN>(th.y, hi.y, bl, p, lut, lk);
        const auto p6 = develop2<TN>(th.z, hi.z, bl, p, lut, lk), p7 = develop2<TN>(th.w, hi.w, bl, p, lut, lk);
        put_pixels8(dst + (size_t)g * (TN == DEEP ? 48 : 24), p0, p1, p2, p3, p4, p5, p6, p7);
    }
}

__global__ __launch_bounds__(256) void k_render2_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                     uint8_t *__restrict__ out, size_t out_stride, uint32_t groups, uint32_t groups_per_row,
                                                     uint32_t row16)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    render2_x16<PLAIN>(frames, stride, params, out, out_stride, groups, groups_per_row, row16, lut, LookArg(), MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_render2_look_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                          uint8_t *__restrict__ out, size_t out_stride, uint32_t groups, uint32_t groups_per_row,
                                                          uint32_t row16, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    render2_x16<LOOK>(frames, stride, params, out, out_stride, groups, groups_per_row, row16, lut, lk, MLV_GRID_STRIDE);
}

// the 16-bit form: no table in LDS; the destination base and stride 16-byte aligned
__global__ __launch_bounds__(256) void k_render2_deep_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                          uint8_t *__restrict__ out, size_t out_stride, uint32_t groups, uint32_t groups_per_row,
                                                          uint32_t row16, const LookArg lk)
{
    render2_x16<DEEP>(frames, stride, params, out, out_stride, groups, groups_per_row, row16, nullptr, lk, MLV_GRID_STRIDE);
}

// npix = W' * H' output pixels per frame
template <Tone TN>
__device__ __forceinline__ void render2_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw, uint8_t *lut,
                                                const LookArg &lk, uint32_t first, uint32_t step)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    for (uint32_t k = first; k < npix; k += step) {
        const uint32_t Y = k / pw, X = k - Y * pw;
        const uint16_t *q = src + (size_t)Y * 2 * w + (size_t)X * 2;
        put_pixel(dst + (size_t)k * (TN == DEEP ? 6 : 3), develop<TN>(q[0], (uint32_t)q[1] + q[w], q[(size_t)w + 1], bl, p, lut, lk));
    }
}

__global__ __launch_bounds__(256) void k_render2_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                         uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    render2_generic<PLAIN>(frames, stride, params, out, out_stride, npix, w, pw, lut, LookArg(), MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_render2_look_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                              uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw,
                                                              const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    render2_generic<LOOK>(frames, stride, params, out, out_stride, npix, w, pw, lut, lk, MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_render2_deep_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                              uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw,
                                                              const LookArg lk)
{
    render2_generic<DEEP>(frames, stride, params, out, out_stride, npix, w, pw, nullptr, lk, MLV_GRID_STRIDE);
}

// step 4 alone: n triples of indices (masked to 12 bits) -> n triples of bytes
__global__ __launch_bounds__(256) void k_look_apply(const LookArg lk, const uint16_t *__restrict__ t, size_t n, uint8_t *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    stage_lut<LOOK>(lut, lk);
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
        const uint16_t *q = t + k * 3;
        put_pixel(out + k * 3, look_out(lut, lk, q[0] & 4095u, q[1] & 4095u, q[2] & 4095u));
    }
}

// step 4 of the 16-bit routes alone: n triples of 16-bit indices -> n triples of 16-bit samples (2-byte aligned both)
__global__ __launch_bounds__(256) void k_look16_apply(const LookArg lk, const uint16_t *__restrict__ t, size_t n, uint16_t *__restrict__ out)
{
    for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
        const uint16_t *q = t + k * 3;
        const uint2 v = deep_out(lk, q[0], q[1], q[2]);
        uint16_t *o = out + k * 3;
        o[0] = (uint16_t)v.x;
        o[1] = (uint16_t)(v.x >> 16);
        o[2] = (uint16_t)v.y;
    }
}

int launch_look16_apply(const LookArg &lk, const uint16_t *d_t, size_t n, uint16_t *d_out, hipStream_t stream)
{
    if (!n) return MLVFS_AMD_OK;
    hipLaunchKernelGGL(k_look16_apply, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, stream, lk, d_t, n, d_out);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

int launch_look_apply(const LookArg &lk, const uint16_t *d_t, size_t n, uint8_t *d_out, hipStream_t stream)
{
    if (!n) return MLVFS_AMD_OK;
    hipLaunchKernelGGL(k_look_apply, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, stream, lk, d_t, n, d_out);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// d_out apart from d_frames (the callers check); w, h >= 2; d_params: 13 int32 per frame, 4-byte aligned
int launch_render2(const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h, int nframes,
                   hipStream_t stream, const LookArg *lk, bool deep)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    int pw, ph;
    if (!rgb_geom(w, h, &pw, &ph)) return route_refuse("launch_render2", { RenderRoute::HALF }, w, h);
    const size_t oa = deep ? 16 : 8;                                                     // what the fast form's stores need
    const bool fast = w % 16 == 0 && ((uintptr_t)d_frames % 16 == 0) && ((uintptr_t)d_out % oa == 0) &&
                      (nframes == 1 || (stride % 16 == 0 && out_stride % oa == 0));
    // the workgroups of a launch share the machine: some two thousand of them in all, each of which stages the table once
    const uint32_t cap = std::max(2048u / (uint32_t)nframes, 64u);
    if (fast) {
        const uint32_t gpr = (uint32_t)w / 16, groups = gpr * (uint32_t)ph;
        const dim3 grid(std::min<uint32_t>((groups + 255) / 256, cap), nframes);
        launch_tone(k_render2_deep_x16, k_render2_look_x16, k_render2_x16, grid, stream, lk, deep, (const uint8_t *)d_frames, stride,
                    (const RenderParams *)d_params, (uint8_t *)d_out, out_stride, groups, gpr, (uint32_t)w / 8);
    } else {
        const uint32_t npix = (uint32_t)pw * (uint32_t)ph;
        const dim3 grid(std::min<uint32_t>((npix + 255) / 256, 4 * cap), nframes);
        launch_tone(k_render2_deep_generic, k_render2_look_generic, k_render2_generic, grid, stream, lk, deep, (const uint8_t *)d_frames, stride,
                    (const RenderParams *)d_params, (uint8_t *)d_out, out_stride, npix, (uint32_t)w, (uint32_t)pw);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

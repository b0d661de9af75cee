// k_amaze_render.hip -- rendered full-size frames with AMaZE as the demosaic (include/mlvfs_amd.h, "rendered full-size frames demosaiced
// by AMaZE"): the two element-wise passes around amaze_launch (k_amaze.hip, k_amaze_rows.hip), which stays what it is.
//     balance   b(y, x) = min((max(in(y, x) - black, 0) * A_j + 2048) >> 12, 65535)     j = (y & 1) + (x & 1)      raw = float(b), exact
//     AMaZE     (R, G, B) = amaze_demosaic_RT.c on raw, 65535 scale (not here)
//     tone      n_c = (int)(clampf(v_c) + 0.5f), clampf(v) = 0 for NaN and v <= 0, 65535 for v >= 65535, else v (binary32, no contraction);
//               then steps 3 and 4 of the rendered routes from k_tone_dev.h: the sRGB table in LDS, a look, or a deep look
// black, A[3], K[9]: the renderings' 13 int32 per frame (mlvfs_amd_rgb_params), uniform in a workgroup.  Frames are batched in grid.y;
// frame k's plane lies k * plane_stride floats behind the batch's plane pointer.  A frame is W * H contiguous pixels, so both passes
// walk it as one run of 8-pixel groups (fast forms) or of pixels (generic forms) in a grid-stride loop.
//   k_amz_balance_x16     : W % 16 == 0, source base and stride and plane base and stride 16-byte aligned.  A lane loads 8 pixels as one
//                           128-bit load -- a group starts on an even column and lies in one row, so its two A are uniform in it -- and
//                           stores two 128-bit float vectors.  Reads 2 W H bytes, writes 4 W H.
//   k_amz_balance_generic : any W the route takes, 2-byte source and 4-byte plane alignment; one lane = one pixel.
//   k_amz_tone_x16<FORM>  : W % 16 == 0, plane bases and stride 16-byte aligned, destination base and stride 8-byte aligned (16-byte in
//                           the deep form).  A lane loads 8 pixels of each plane as two 128-bit loads and stores k_render1_x16's shapes:
//                           24 bytes as three 64-bit stores, or 48 bytes as three 128-bit stores.  Reads 12 W H bytes, writes 3 or 6 W H.
//   k_amz_tone_generic<FORM> : any alignment the types allow; one lane = one pixel, the 64-bit matrix.
// Bytes between renderings and behind 3 (6) W H are never touched; no scratch memory.
#include "k_tone_dev.h"

namespace mlv {

namespace {                    // this file's device helpers

// step 3 of the route: one AMaZE value to the 16-bit sample the matrix takes.  NaN fails the compare and gives 0; the sum is the
// definition's binary32 sum (the file is built without contraction), so 0.49999997f, whose sum rounds to 1.0f, gives 1 here as there
__device__ __forceinline__ uint32_t sample16(float v)
{
    const float c = v > 0.0f ? fminf(v, 65535.0f) : 0.0f;
    return (uint32_t)(c + 0.5f);
}

__device__ __forceinline__ float4 balance4f(uint32_t lo, uint32_t hi, const Black &bl, int32_t a_even, int32_t a_odd)
{
    return make_float4((float)balance(bl(lo & 0xFFFFu), a_even), (float)balance(bl(lo >> 16), a_odd),
                       (float)balance(bl(hi & 0xFFFFu), a_even), (float)balance(bl(hi >> 16), a_odd));
}

// the 8 pixels of one lane: planes at the lane's first pixel
template <bool K32, Tone TN>
__device__ __forceinline__ void tone8(const float *r, const float *g, const float *b, const RenderParams &p, const uint8_t *lut, const LookArg &lk,
                                      uint8_t *o)
{
    const float4 r0 = ((const float4 *)r)[0], r1 = ((const float4 *)r)[1];
    const float4 g0 = ((const float4 *)g)[0], g1 = ((const float4 *)g)[1];
    const float4 b0 = ((const float4 *)b)[0], b1 = ((const float4 *)b)[1];
    const float rr[8] = { r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w };
    const float gg[8] = { g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w };
    const float bb[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
    decltype(tone<K32, TN>(p, lut, lk, 0u, 0u, 0u)) px[8];
#pragma unroll
    for (int i = 0; i < 8; i++) px[i] = tone<K32, TN>(p, lut, lk, sample16(rr[i]), sample16(gg[i]), sample16(bb[i]));
    put_pixels8(o, px[0], px[1], px[2], px[3], px[4], px[5], px[6], px[7]);
}

template <bool K32, Tone TN>
__device__ __forceinline__ void tone_groups(const float *r, const float *g, const float *b, const RenderParams &p, const uint8_t *lut,
                                            const LookArg &lk, uint8_t *dst, uint32_t ngroups, uint32_t first, uint32_t step)
{
    for (uint32_t k = first; k < ngroups; k += step)
        tone8<K32, TN>(r + 8 * (size_t)k, g + 8 * (size_t)k, b + 8 * (size_t)k, p, lut, lk, dst + (size_t)k * (TN == DEEP ? 48 : 24));
}

// ngroups = W * H / 8 groups per frame
template <Tone TN>
__device__ __forceinline__ void amz_tone_x16(const float *__restrict__ red, const float *__restrict__ green, const float *__restrict__ blue,
                                             size_t plane_stride, const RenderParams *__restrict__ params, uint8_t *__restrict__ out,
                                             size_t out_stride, uint32_t ngroups, uint8_t *lut, const LookArg &lk, uint32_t first, uint32_t step)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const size_t at = (size_t)blockIdx.y * plane_stride;
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    if (fits32(p)) tone_groups<true, TN>(red + at, green + at, blue + at, p, lut, lk, dst, ngroups, first, step);
    else tone_groups<false, TN>(red + at, green + at, blue + at, p, lut, lk, dst, ngroups, first, step);
}

// npix = W * H pixels per frame
template <Tone TN>
__device__ __forceinline__ void amz_tone_generic(const float *__restrict__ red, const float *__restrict__ green, const float *__restrict__ blue,
                                                 size_t plane_stride, const RenderParams *__restrict__ params, uint8_t *__restrict__ out,
                                                 size_t out_stride, uint32_t npix, uint8_t *lut, const LookArg &lk, uint32_t first, uint32_t step)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const size_t at = (size_t)blockIdx.y * plane_stride;
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    for (uint32_t k = first; k < npix; k += step)
        put_pixel(dst + (size_t)k * (TN == DEEP ? 6 : 3),
                  tone<false, TN>(p, lut, lk, sample16(red[at + k]), sample16(green[at + k]), sample16(blue[at + k])));
}

}  // namespace

// ngroups = W * H / 8, gw = W / 8 groups per row
__global__ __launch_bounds__(256) void k_amz_balance_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                         float *__restrict__ planes, size_t plane_stride, uint32_t ngroups, uint32_t gw)
{
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const uint4 *src = (const uint4 *)(frames + (size_t)blockIdx.y * stride);
    float4 *dst = (float4 *)(planes + (size_t)blockIdx.y * plane_stride);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < ngroups; k += gridDim.x * blockDim.x) {
        const bool odd = (k / gw) & 1;
        const int32_t a_even = odd ? p.A[1] : p.A[0], a_odd = odd ? p.A[2] : p.A[1];
        const uint4 v = src[k];
        dst[2 * (size_t)k] = balance4f(v.x, v.y, bl, a_even, a_odd);
        dst[2 * (size_t)k + 1] = balance4f(v.z, v.w, bl, a_even, a_odd);
    }
}

// npix = W * H
__global__ __launch_bounds__(256) void k_amz_balance_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                             float *__restrict__ planes, size_t plane_stride, uint32_t npix, uint32_t w)
{
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    float *dst = planes + (size_t)blockIdx.y * plane_stride;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x) {
        const uint32_t y = k / w, x = k - y * w, j = (y & 1) + (x & 1);
        dst[k] = (float)balance(bl(src[k]), j == 0 ? p.A[0] : j == 1 ? p.A[1] : p.A[2]);
    }
}

__global__ __launch_bounds__(256) void k_amz_tone_x16(const float *__restrict__ red, const float *__restrict__ green, const float *__restrict__ blue,
                                                      size_t plane_stride, const RenderParams *__restrict__ params, uint8_t *__restrict__ out,
                                                      size_t out_stride, uint32_t ngroups)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    amz_tone_x16<PLAIN>(red, green, blue, plane_stride, params, out, out_stride, ngroups, lut, LookArg(), MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_amz_tone_look_x16(const float *__restrict__ red, const float *__restrict__ green,
                                                           const float *__restrict__ blue, size_t plane_stride, const RenderParams *__restrict__ params,
                                                           uint8_t *__restrict__ out, size_t out_stride, uint32_t ngroups, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    amz_tone_x16<LOOK>(red, green, blue, plane_stride, params, out, out_stride, ngroups, lut, lk, MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_amz_tone_deep_x16(const float *__restrict__ red, const float *__restrict__ green,
                                                           const float *__restrict__ blue, size_t plane_stride, const RenderParams *__restrict__ params,
                                                           uint8_t *__restrict__ out, size_t out_stride, uint32_t ngroups, const LookArg lk)
{
    amz_tone_x16<DEEP>(red, green, blue, plane_stride, params, out, out_stride, ngroups, nullptr, lk, MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_amz_tone_generic(const float *__restrict__ red, const float *__restrict__ green,
                                                          const float *__restrict__ blue, size_t plane_stride, const RenderParams *__restrict__ params,
                                                          uint8_t *__restrict__ out, size_t out_stride, uint32_t npix)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    amz_tone_generic<PLAIN>(red, green, blue, plane_stride, params, out, out_stride, npix, lut, LookArg(), MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_amz_tone_look_generic(const float *__restrict__ red, const float *__restrict__ green,
                                                               const float *__restrict__ blue, size_t plane_stride,
                                                               const RenderParams *__restrict__ params, uint8_t *__restrict__ out, size_t out_stride,
                                                               uint32_t npix, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    amz_tone_generic<LOOK>(red, green, blue, plane_stride, params, out, out_stride, npix, lut, lk, MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_amz_tone_deep_generic(const float *__restrict__ red, const float *__restrict__ green,
                                                               const float *__restrict__ blue, size_t plane_stride,
                                                               const RenderParams *__restrict__ params, uint8_t *__restrict__ out, size_t out_stride,
                                                               uint32_t npix, const LookArg lk)
{
    amz_tone_generic<DEEP>(red, green, blue, plane_stride, params, out, out_stride, npix, nullptr, lk, MLV_GRID_STRIDE);
}

// the workgroups of a launch share the machine: each of them stages its table once, and the lanes stride over the rest
static dim3 amz_grid(uint32_t items, int nframes)
{
    const uint32_t cap = 4 * std::max(2048u / (uint32_t)nframes, 64u);
    return dim3(std::min<uint32_t>((items + 255) / 256, cap), nframes);
}

// the callers check: rgb_amaze_geom(w, h), the planes apart from the frames and the parameters; d_params: 13 int32 per frame
int launch_amz_balance(const void *d_frames, size_t stride, const int32_t *d_params, float *d_planes, size_t plane_stride, int w, int h,
                       int nframes, hipStream_t stream)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (!rgb_amaze_geom(w, h)) return route_refuse("launch_amz", { RenderRoute::FULL, true }, w, h);
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    const bool fast = w % 16 == 0 && ((uintptr_t)d_frames % 16 == 0) && ((uintptr_t)d_planes % 16 == 0) &&
                      (nframes == 1 || (stride % 16 == 0 && plane_stride % 4 == 0));
    if (fast)
        hipLaunchKernelGGL(k_amz_balance_x16, amz_grid(npix / 8, nframes), dim3(256), 0, stream, (const uint8_t *)d_frames, stride,
                           (const RenderParams *)d_params, d_planes, plane_stride, npix / 8, (uint32_t)w / 8);
    else
        hipLaunchKernelGGL(k_amz_balance_generic, amz_grid(npix, nframes), dim3(256), 0, stream, (const uint8_t *)d_frames, stride,
                           (const RenderParams *)d_params, d_planes, plane_stride, npix, (uint32_t)w);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// lk: the look, or with deep the deep look; null: the sRGB table
int launch_amz_tone(const float *d_red, const float *d_green, const float *d_blue, size_t plane_stride, const int32_t *d_params, void *d_out,
                    size_t out_stride, int w, int h, int nframes, hipStream_t stream, const LookArg *lk, bool deep)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (!rgb_amaze_geom(w, h)) return route_refuse("launch_amz", { RenderRoute::FULL, true }, w, h);
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    const size_t oa = deep ? 16 : 8;                                                     // what the fast form's stores need
    const bool fast = w % 16 == 0 && (((uintptr_t)d_red | (uintptr_t)d_green | (uintptr_t)d_blue) % 16 == 0) && ((uintptr_t)d_out % oa == 0) &&
                      (nframes == 1 || (plane_stride % 4 == 0 && out_stride % oa == 0));
    const RenderParams *par = (const RenderParams *)d_params;
    uint8_t *out = (uint8_t *)d_out;
    if (fast) {
        launch_tone(k_amz_tone_deep_x16, k_amz_tone_look_x16, k_amz_tone_x16, amz_grid(npix / 8, nframes), stream, lk, deep, d_red, d_green, d_blue,
                    plane_stride, par, out, out_stride, npix / 8);
    } else {
        launch_tone(k_amz_tone_deep_generic, k_amz_tone_look_generic, k_amz_tone_generic, amz_grid(npix, nframes), stream, lk, deep, d_red, d_green,
                    d_blue, plane_stride, par, out, out_stride, npix);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

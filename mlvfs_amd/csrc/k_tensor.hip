// k_tensor.hip -- a clip's frames as device-resident tensors (include/mlvfs_amd.h, "a clip's frames as device-resident tensors";
// DESIGN.md 3.24): one element-wise pass behind whatever produced the rendering (interleaved R, G, B of 8 or 16 bits) or the final frame
// (16-bit RGGB mosaic).  Per element of channel c, with v the sample (RGB) or px - black (Bayer):
//     F32   y = fl32(fl32(fl32(v) unit) scale_c), out = fl32(y + bias_c)        -- three operations, each rounded on its own
//     F16, BF16   that value through the hardware's round-to-nearest-even conversions (v_cvt_f16_f32, v_cvt_pk_bf16_f32)
//     U8, U16     the sample itself (Bayer: the raw px), re-laid out
// The file is compiled with -ffp-contract=off and says so once more below: no multiplication here is ever fused with an addition.
//
// Never in place, frames in grid.y, the workgroups of a launch capped and the lanes striding over the rest (as k_render2_x16 does), no
// LDS, no scratch.  scale and bias are kernel arguments; a Bayer frame's black and unit come from a device array indexed by blockIdx.y
// (mlvfs_amd_tensor_bayer_params): both are scalar loads.
//   k_tensor_rgb_x8<SRC_BITS, DTYPE, LAYOUT> : pw % 8 == 0, both bases and strides 16-byte aligned.  One lane = 8 pixels = 24 or 48
//                       source bytes (three 64-bit or three 128-bit loads).  NCHW: three runs of 8 elements, one per plane -- a wave
//                       writes 512 B to 2 KiB contiguous per plane; NHWC: one run of 24 elements.
//   k_tensor_bayer_x8<DTYPE, LAYOUT> : W % 16 == 0, both bases and strides 16-byte aligned.  One lane = 16 pixels (two 128-bit loads)
//                       of each of the two rows of a superpixel row -- what k_render2_x16 reads -- = 8 elements to each of four planes,
//                       or 32 interleaved.
//   k_tensor_rgb_generic, k_tensor_bayer_generic : any shape, element alignment only, one output pixel per lane; dtype and layout
//                       are arguments, uniform in the launch.
// Bytes between frames and behind a frame's tensor are never touched; an odd last row or column of a Bayer frame is never read.
#include "tensor.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace mlv {

namespace {

constexpr int F32 = MLVFS_AMD_TENSOR_F32, F16 = MLVFS_AMD_TENSOR_F16, BF16 = MLVFS_AMD_TENSOR_BF16, U8 = MLVFS_AMD_TENSOR_U8, U16 = MLVFS_AMD_TENSOR_U16;
constexpr int NCHW = MLVFS_AMD_TENSOR_NCHW, NHWC = MLVFS_AMD_TENSOR_NHWC;

constexpr __host__ __device__ int elem_size(int dt) { return dt == F32 ? 4 : dt == U8 ? 1 : 2; }

// the definition's float value: each of the three operations is a statement of its own
__device__ __forceinline__ float affine(int v, float unit, float scale, float bias)
{
    const float x = (float)v * unit;
    const float y = x * scale;
    return y + bias;
}
__device__ __forceinline__ uint32_t half_bits(float o) { return __builtin_bit_cast(uint16_t, (_Float16)o); }
__device__ __forceinline__ uint32_t bfloat_bits(float o) { return __builtin_bit_cast(uint16_t, (__bf16)o); }

// one element as the bits that are stored, in the low bytes of a dword; raw: the sample an integer dtype keeps
template <int DT>
__device__ __forceinline__ uint32_t element(int v, uint32_t raw, float unit, float scale, float bias)
{
    if constexpr (DT == U8 || DT == U16) return raw;
    else if constexpr (DT == F32) return __float_as_uint(affine(v, unit, scale, bias));
    else if constexpr (DT == F16) return half_bits(affine(v, unit, scale, bias));
    else return bfloat_bits(affine(v, unit, scale, bias));
}
__device__ __forceinline__ uint32_t element_of(int dt, int v, uint32_t raw, float unit, float scale, float bias)
{
    if (dt == U8 || dt == U16) return raw;
    const float o = affine(v, unit, scale, bias);
    return dt == F32 ? __float_as_uint(o) : dt == F16 ? half_bits(o) : bfloat_bits(o);
}

// a run of 8 elements of ES bytes at a 16-byte (ES = 1: 8-byte) boundary
template <int ES>
__device__ __forceinline__ void put8(uint8_t *at, uint32_t e0, uint32_t e1, uint32_t e2, uint32_t e3, uint32_t e4, uint32_t e5, uint32_t e6, uint32_t e7)
{
    if constexpr (ES == 4) {
        ((uint4 *)at)[0] = make_uint4(e0, e1, e2, e3);
        ((uint4 *)at)[1] = make_uint4(e4, e5, e6, e7);
    } else if constexpr (ES == 2) {
        *(uint4 *)at = make_uint4(e0 | (e1 << 16), e2 | (e3 << 16), e4 | (e5 << 16), e6 | (e7 << 16));
    } else {
        *(uint2 *)at = make_uint2(e0 | (e1 << 8) | (e2 << 16) | (e3 << 24), e4 | (e5 << 8) | (e6 << 16) | (e7 << 24));
    }
}
// one element at index k of a tensor of es-byte elements
__device__ __forceinline__ void put1(uint8_t *base, size_t k, int es, uint32_t e)
{
    if (es == 4) ((uint32_t *)base)[k] = e;
    else if (es == 2) ((uint16_t *)base)[k] = (uint16_t)e;
    else base[k] = (uint8_t)e;
}

// groups = npix / 8 per frame: 8 pixels of the rendering in order (its rows have no padding)
template <int SRC_BITS, int DT, int LAYOUT>
__global__ __launch_bounds__(256) void k_tensor_rgb_x8(const uint8_t *__restrict__ src, size_t src_stride, uint8_t *__restrict__ out, size_t out_stride,
                                                       uint32_t groups, uint32_t npix, float unit, const TensorAffine a)
{
    constexpr int ES = elem_size(DT);
    const uint8_t *s = src + (size_t)blockIdx.y * src_stride;
    uint8_t *d = out + (size_t)blockIdx.y * out_stride;
    const uint32_t first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (uint32_t g = first; g < groups; g += step) {
        uint32_t v[24];                                                  // R, G, B of pixel 0, of pixel 1, ...
        if constexpr (SRC_BITS == 8) {
            const uint2 *q = (const uint2 *)(s + (size_t)g * 24);
            const uint2 q0 = q[0], q1 = q[1], q2 = q[2];
            const uint32_t w[6] = { q0.x, q0.y, q1.x, q1.y, q2.x, q2.y };
#pragma unroll
            for (int i = 0; i < 24; i++) v[i] = (w[i >> 2] >> (8 * (i & 3))) & 0xFFu;
        } else {
            const uint4 *q = (const uint4 *)(s + (size_t)g * 48);
            const uint4 q0 = q[0], q1 = q[1], q2 = q[2];
            const uint32_t w[12] = { q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w };
#pragma unroll
            for (int i = 0; i < 24; i++) v[i] = (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
        }
        uint32_t e[24];
#pragma unroll
        for (int i = 0; i < 24; i++) e[i] = element<DT>((int)v[i], v[i], unit, a.scale[i % 3], a.bias[i % 3]);
        if constexpr (LAYOUT == NHWC) {
#pragma unroll
            for (int r = 0; r < 3; r++)
                put8<ES>(d + ((size_t)g * 24 + 8 * r) * ES, e[8 * r], e[8 * r + 1], e[8 * r + 2], e[8 * r + 3], e[8 * r + 4], e[8 * r + 5], e[8 * r + 6], e[8 * r + 7]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++)
                put8<ES>(d + ((size_t)c * npix + (size_t)g * 8) * ES, e[c], e[3 + c], e[6 + c], e[9 + c], e[12 + c], e[15 + c], e[18 + c], e[21 + c]);
        }
    }
}

// npix = pw * ph pixels per frame
__global__ __launch_bounds__(256) void k_tensor_rgb_generic(const uint8_t *__restrict__ src, size_t src_stride, uint8_t *__restrict__ out, size_t out_stride,
                                                            uint32_t npix, int src_bits, int dt, int layout, float unit, const TensorAffine a)
{
    const int es = elem_size(dt);
    const uint8_t *s = src + (size_t)blockIdx.y * src_stride;
    uint8_t *d = out + (size_t)blockIdx.y * out_stride;
    const uint32_t first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (uint32_t k = first; k < npix; k += step) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const size_t at = (size_t)k * 3 + c;
            const uint32_t v = src_bits == 8 ? s[at] : ((const uint16_t *)s)[at];
            put1(d, layout == NHWC ? at : (size_t)c * npix + k, es, element_of(dt, (int)v, v, unit, a.scale[c], a.bias[c]));
        }
    }
}

// groups = W / 16 * (H / 2) per frame: superpixel rows in order, 16-pixel groups of a row in order.  row16 = W / 8: uint4s per source
// row.  npix = (W / 2) (H / 2): a group's 8 superpixels are the elements 8 g .. 8 g + 7 of a plane
template <int DT, int LAYOUT>
__global__ __launch_bounds__(256) void k_tensor_bayer_x8(const uint8_t *__restrict__ frames, size_t stride, const int32_t *__restrict__ levels,
                                                         uint8_t *__restrict__ out, size_t out_stride, uint32_t groups, uint32_t groups_per_row,
                                                         uint32_t row16, uint32_t npix, const TensorAffine a)
{
    constexpr int ES = elem_size(DT);
    const int black = levels[(size_t)blockIdx.y * TENSOR_LEVELS];
    const float unit = __int_as_float(levels[(size_t)blockIdx.y * TENSOR_LEVELS + 2]);
    const uint4 *src = (const uint4 *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *d = out + (size_t)blockIdx.y * out_stride;
    const uint32_t first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (uint32_t g = first; g < groups; g += step) {
        const uint32_t Y = g / groups_per_row, gx = g - Y * groups_per_row;
        const uint4 *q = src + (size_t)Y * 2 * row16 + (size_t)gx * 2;
        const uint4 tl = q[0], th = q[1], lo = q[row16], hi = q[row16 + 1];          // top and lower row, 8 pixels each
        const uint32_t top[8] = { tl.x, tl.y, tl.z, tl.w, th.x, th.y, th.z, th.w }, bot[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
        uint32_t e[32];                                                  // R, G1, G2, B of superpixel 0, of superpixel 1, ...
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t px[4] = { top[i] & 0xFFFFu, top[i] >> 16, bot[i] & 0xFFFFu, bot[i] >> 16 };
#pragma unroll
            for (int c = 0; c < 4; c++) e[4 * i + c] = element<DT>((int)px[c] - black, px[c], unit, a.scale[c], a.bias[c]);
        }
        if constexpr (LAYOUT == NHWC) {
#pragma unroll
            for (int r = 0; r < 4; r++)
                put8<ES>(d + ((size_t)g * 32 + 8 * r) * ES, e[8 * r], e[8 * r + 1], e[8 * r + 2], e[8 * r + 3], e[8 * r + 4], e[8 * r + 5], e[8 * r + 6], e[8 * r + 7]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++)
                put8<ES>(d + ((size_t)c * npix + (size_t)g * 8) * ES, e[c], e[4 + c], e[8 + c], e[12 + c], e[16 + c], e[20 + c], e[24 + c], e[28 + c]);
        }
    }
}

// npix = pw * ph superpixels per frame, pw = w / 2
__global__ __launch_bounds__(256) void k_tensor_bayer_generic(const uint8_t *__restrict__ frames, size_t stride, const int32_t *__restrict__ levels,
                                                              uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw,
                                                              int dt, int layout, const TensorAffine a)
{
    const int es = elem_size(dt);
    const int black = levels[(size_t)blockIdx.y * TENSOR_LEVELS];
    const float unit = __int_as_float(levels[(size_t)blockIdx.y * TENSOR_LEVELS + 2]);
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *d = out + (size_t)blockIdx.y * out_stride;
    const uint32_t first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (uint32_t k = first; k < npix; k += step) {
        const uint32_t Y = k / pw, X = k - Y * pw;
        const uint16_t *q = src + (size_t)Y * 2 * w + (size_t)X * 2;
        const uint32_t px[4] = { q[0], q[1], q[w], q[(size_t)w + 1] };
#pragma unroll
        for (int c = 0; c < 4; c++)
            put1(d, layout == NHWC ? (size_t)k * 4 + c : (size_t)c * npix + k, es, element_of(dt, (int)px[c] - black, px[c], unit, a.scale[c], a.bias[c]));
    }
}

bool aligned16(const void *a, const void *b, size_t sa, size_t sb, int nframes)
{
    return (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0 && (nframes == 1 || (sa % 16 == 0 && sb % 16 == 0));
}

// the workgroups of a launch share the machine: some two thousand of them in all, the lanes stride over the rest
uint32_t group_cap(int nframes) { return std::max(2048u / (uint32_t)nframes, 64u); }

template <int SRC_BITS, int LAYOUT, class... Args>
void rgb_x8(int dtype, dim3 grid, hipStream_t stream, Args... args)
{
    switch (dtype) {
    case F32: hipLaunchKernelGGL((k_tensor_rgb_x8<SRC_BITS, F32, LAYOUT>), grid, dim3(256), 0, stream, args...); break;
    case F16: hipLaunchKernelGGL((k_tensor_rgb_x8<SRC_BITS, F16, LAYOUT>), grid, dim3(256), 0, stream, args...); break;
    case BF16: hipLaunchKernelGGL((k_tensor_rgb_x8<SRC_BITS, BF16, LAYOUT>), grid, dim3(256), 0, stream, args...); break;
    default: hipLaunchKernelGGL((k_tensor_rgb_x8<SRC_BITS, SRC_BITS == 8 ? U8 : U16, LAYOUT>), grid, dim3(256), 0, stream, args...); break;
    }
}

template <int LAYOUT, class... Args>
void bayer_x8(int dtype, dim3 grid, hipStream_t stream, Args... args)
{
    switch (dtype) {
    case F32: hipLaunchKernelGGL((k_tensor_bayer_x8<F32, LAYOUT>), grid, dim3(256), 0, stream, args...); break;
    case F16: hipLaunchKernelGGL((k_tensor_bayer_x8<F16, LAYOUT>), grid, dim3(256), 0, stream, args...); break;
    case BF16: hipLaunchKernelGGL((k_tensor_bayer_x8<BF16, LAYOUT>), grid, dim3(256), 0, stream, args...); break;
    default: hipLaunchKernelGGL((k_tensor_bayer_x8<U16, LAYOUT>), grid, dim3(256), 0, stream, args...); break;
    }
}

}  // namespace

// d_out apart from d_src, the dtype legal for src_bits, the strides and the element alignment as the definition asks (the callers check)
int launch_tensor_rgb(const void *d_src, size_t src_stride, int pw, int ph, int src_bits, int dtype, int layout, const TensorAffine &a, void *d_out,
                      size_t out_stride, int nframes, hipStream_t stream)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (pw < 1 || ph < 1 || (uint64_t)pw * (uint64_t)ph >= (1u << 28) || (src_bits != 8 && src_bits != 16) || !tensor_dtype_legal(dtype, src_bits) ||
        !tensor_layout_ok(layout)) {
        set_error("launch_tensor_rgb: %dx%d at %d bits to dtype %d, layout %d not supported", pw, ph, src_bits, dtype, layout);
        return MLVFS_AMD_ERR_ARG;
    }
    const uint32_t npix = (uint32_t)pw * (uint32_t)ph, cap = group_cap(nframes);
    // the double quotient rounded once
    const float unit = src_bits == 8 ? (float)(1.0 / 255.0) : (float)(1.0 / 65535.0);
    const uint8_t *s = (const uint8_t *)d_src;
    uint8_t *d = (uint8_t *)d_out;
    if (pw % 8 == 0 && aligned16(d_src, d_out, src_stride, out_stride, nframes)) {
        const uint32_t groups = npix / 8;
        const dim3 grid(std::min<uint32_t>((groups + 255) / 256, cap), nframes);
        if (src_bits == 8) {
            if (layout == NCHW) rgb_x8<8, NCHW>(dtype, grid, stream, s, src_stride, d, out_stride, groups, npix, unit, a);
            else rgb_x8<8, NHWC>(dtype, grid, stream, s, src_stride, d, out_stride, groups, npix, unit, a);
        } else {
            if (layout == NCHW) rgb_x8<16, NCHW>(dtype, grid, stream, s, src_stride, d, out_stride, groups, npix, unit, a);
            else rgb_x8<16, NHWC>(dtype, grid, stream, s, src_stride, d, out_stride, groups, npix, unit, a);
        }
    } else {
        const dim3 grid(std::min<uint32_t>((npix + 255) / 256, 4 * cap), nframes);
        hipLaunchKernelGGL(k_tensor_rgb_generic, grid, dim3(256), 0, stream, s, src_stride, d, out_stride, npix, src_bits, dtype, layout, unit, a);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// d_levels: TENSOR_LEVELS int32 per frame, 4-byte aligned; the rest as above
int launch_tensor_bayer(const void *d_frames, size_t stride, int w, int h, const int32_t *d_levels, int dtype, int layout, const TensorAffine &a,
                        void *d_out, size_t out_stride, int nframes, hipStream_t stream)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (w < 2 || h < 2 || (uint64_t)w * (uint64_t)h >= (1u << 28) || !tensor_dtype_legal(dtype, 16) || !tensor_layout_ok(layout)) {
        set_error("launch_tensor_bayer: %dx%d to dtype %d, layout %d not supported", w, h, dtype, layout);
        return MLVFS_AMD_ERR_ARG;
    }
    const uint32_t pw = (uint32_t)w / 2, ph = (uint32_t)h / 2, npix = pw * ph, cap = group_cap(nframes);
    const uint8_t *s = (const uint8_t *)d_frames;
    uint8_t *d = (uint8_t *)d_out;
    if (w % 16 == 0 && aligned16(d_frames, d_out, stride, out_stride, nframes)) {
        const uint32_t gpr = (uint32_t)w / 16, groups = gpr * ph;
        const dim3 grid(std::min<uint32_t>((groups + 255) / 256, cap), nframes);
        if (layout == NCHW) bayer_x8<NCHW>(dtype, grid, stream, s, stride, d_levels, d, out_stride, groups, gpr, (uint32_t)w / 8, npix, a);
        else bayer_x8<NHWC>(dtype, grid, stream, s, stride, d_levels, d, out_stride, groups, gpr, (uint32_t)w / 8, npix, a);
    } else {
        const dim3 grid(std::min<uint32_t>((npix + 255) / 256, 4 * cap), nframes);
        hipLaunchKernelGGL(k_tensor_bayer_generic, grid, dim3(256), 0, stream, s, stride, d_levels, d, out_stride, npix, (uint32_t)w, pw, dtype, layout, a);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

// k_tone_dev.h -- what the render kernels share (k_render.hip, k_demosaic.hip, k_scale.hip): the per-frame parameters, the black
// level, the balance (step 2), the matrix (step 3) in its 64-bit and its 32-bit form, and step 4 once, as a template on LOOK:
//     plain   out_i = LUT[t_i]                       the 4 KiB sRGB table in LDS, three byte reads
//     look    4a .. 4d of include/mlvfs_amd.h, "a look for the rendered frames": the shaper S (8 KiB) in LDS INSTEAD of the sRGB table,
//             the cube T in global memory as padded 8-byte entries (R | G << 16, B), one 64-bit gather per vertex, four per pixel.
//             The tetrahedron is found without a branch: maximum, minimum and median of the three fractions by compares and selects;
//             the step from V0 to V1 is the stride of the axis that holds the maximum (priorities r, g, b), the step from V3 back to V2
//             that of the axis that holds the minimum (priorities b, g, r), so the two axes differ even where fractions are equal.
//             i_c <= N - 2 for every 16-bit shaper value, so every gather lies inside the N^3 entries whatever S and t hold.
//     deep    the 16-bit routes (include/mlvfs_amd.h, "rendered frames at 16 bits"): step 3d's 16-bit index, 4a from the deep look's
//             S16 -- 128 KiB, which stays in global memory and is read through the cache as 2-byte gathers: a deep kernel stages
//             nothing in LDS and has no barrier at entry --, then 4b and 4c as above, or nothing where N = 0 (uniform in a launch);
//             no 4d: three 16-bit samples per pixel.  t <= 65535 and u <= 65535, so every gather is in bounds whatever S16 holds.
// A kernel body is a template on the form (Tone); its plain __global__ form passes an empty LookArg that no instruction reads.
// The host side picks among a kernel's three __global__ forms in one place, launch_tone.
#pragma once
#include "clip.h"
#include "render_route.h"

#define MLV_SRGB_LUT12_ATTR __device__ __attribute__((aligned(16)))          // stage_lut reads it in 16-byte pieces
#include "srgb_lut12.h"

// a grid-stride loop's first index and step, for the bodies that take them as arguments.  A kernel reads blockDim itself: read inside
// a device function that is inlined into it, the compiler takes the general form of the work-group size (a load and a select) where
// the kernel's own read folds to the launch's uniform size
#define MLV_GRID_STRIDE blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x

namespace mlv {

enum Tone { PLAIN, LOOK, DEEP };           // the three forms of steps 3 and 4

struct RenderParams {          // mlvfs_amd_rgb_params' out[RGB_PARAMS]
    int32_t black, A[3], K[9];
};
static_assert(sizeof(RenderParams) == RGB_PARAMS * sizeof(int32_t), "mlvfs_amd_rgb_params' layout");

namespace {                    // every including file's own copy

// host side: one of a kernel's three forms launched with 256 lanes a workgroup -- the deep form with *lk, the look form with *lk, or
// the plain form, which takes no look -- and otherwise the same arguments
template <class KDeep, class KLook, class KPlain, class... Args>
void launch_tone(KDeep k_deep, KLook k_look, KPlain k_plain, const dim3 &grid, hipStream_t stream, const LookArg *lk, bool deep, Args... args)
{
    if (deep) hipLaunchKernelGGL(k_deep, grid, dim3(256), 0, stream, args..., *lk);
    else if (lk) hipLaunchKernelGGL(k_look, grid, dim3(256), 0, stream, args..., *lk);
    else hipLaunchKernelGGL(k_plain, grid, dim3(256), 0, stream, args...);
}

// bytes of the table a workgroup stages: the sRGB bytes, or the look's shaper (a deep kernel stages none and declares none)
template <Tone TN> constexpr int TONE_LDS = TN == LOOK ? LOOK_SHAPER_BYTES : 4096;

// 256 lanes x 16 bytes, or x 32; deep: nothing, and no barrier
template <Tone TN>
__device__ __forceinline__ void stage_lut(uint8_t *lut, const LookArg &lk)
{
    if constexpr (TN == DEEP) {
        return;
    } else if constexpr (TN == LOOK) {
        ((uint4 *)lut)[threadIdx.x] = ((const uint4 *)lk.image)[threadIdx.x];
        ((uint4 *)lut)[threadIdx.x + 256] = ((const uint4 *)lk.image)[threadIdx.x + 256];
    } else {
        ((uint4 *)lut)[threadIdx.x] = ((const uint4 *)kSrgbLut12)[threadIdx.x];
    }
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

// step 3 in 64 bits, and in 32 where the frame's K allows it (fits32: every |K| < 2^15, every sum below 2^31)
template <bool K32>
__device__ __forceinline__ uint32_t tone_index(const int32_t *K, uint32_t n0, uint32_t n1, uint32_t n2)
{
    if constexpr (K32) {
        const int acc = __mul24(K[0], (int)n0) + __mul24(K[1], (int)n1) + __mul24(K[2], (int)n2) + 32768;
        const int t = acc >> 16;
        return t < 0 ? 0u : t > 4095 ? 4095u : (uint32_t)t;
    }
    const int64_t acc = (int64_t)K[0] * (int32_t)n0 + (int64_t)K[1] * (int32_t)n1 + (int64_t)K[2] * (int32_t)n2 + 32768;
    const int64_t t = acc >> 16;
    return t < 0 ? 0u : t > 4095 ? 4095u : (uint32_t)t;
}

// step 3d: the same sum read four bits further down; the 32-bit form stays valid, its rounding term is the smaller one
template <bool K32>
__device__ __forceinline__ uint32_t tone_index16(const int32_t *K, uint32_t n0, uint32_t n1, uint32_t n2)
{
    if constexpr (K32) {
        const int acc = __mul24(K[0], (int)n0) + __mul24(K[1], (int)n1) + __mul24(K[2], (int)n2) + 2048;
        const int t = acc >> 12;
        return t < 0 ? 0u : t > 65535 ? 65535u : (uint32_t)t;
    }
    const int64_t acc = (int64_t)K[0] * (int32_t)n0 + (int64_t)K[1] * (int32_t)n1 + (int64_t)K[2] * (int32_t)n2 + 2048;
    const int64_t t = acc >> 12;
    return t < 0 ? 0u : t > 65535 ? 65535u : (uint32_t)t;
}

__device__ __forceinline__ bool fits32(const RenderParams &p)
{
    bool ok = true;
    for (int i = 0; i < 3; i++) {
        uint64_t sum = 0;
        for (int j = 0; j < 3; j++) { const int64_t k = p.K[3 * i + j]; sum += (uint64_t)(k < 0 ? -k : k); }
        ok = ok && sum * 65535u + 32768u < (1ull << 31);
    }
    return ok;
}

// 4c for one output channel: the four vertices' values of it, the weights; every factor is below 2^24 and the sum below 2^32
__device__ __forceinline__ uint32_t look_vertex_sum(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
    return (__umul24(w0, v0) + __umul24(w1, v1) + __umul24(w2, v2) + __umul24(w3, v3) + 32768u) >> 16;
}

// 4c and 4d for one output channel
__device__ __forceinline__ uint32_t look_channel(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
    const uint32_t v = look_vertex_sum(v0, v1, v2, v3, w0, w1, w2, w3);
    return (v + 128u) / 257u;
}

// step 4 with a look: the three bytes of one output pixel in bits 0 .. 23, R, G, B from the low byte up, from its three 12-bit indices
__device__ __forceinline__ uint32_t look_out(const uint8_t *lut, const LookArg &lk, uint32_t tr, uint32_t tg, uint32_t tb)
{
    const uint16_t *S = (const uint16_t *)lut;
    const uint32_t N = lk.n, NN = N * N, n1 = N - 1u;
    const uint32_t pr = S[tr] * n1, pg = S[tg] * n1, pb = S[tb] * n1;                    // 4a, 4b: below 2^16 * 64
    const uint32_t ir = pr >> 16, ig = pg >> 16, ib = pb >> 16, fr = pr & 65535u, fg = pg & 65535u, fb = pb & 65535u;
    const uint32_t fmax = max(fr, max(fg, fb)), fmin = min(fr, min(fg, fb)), fmed = max(min(fr, fg), min(max(fr, fg), fb));
    const uint32_t up = fr == fmax ? 1u : fg == fmax ? N : NN;                            // V0 -> V1
    const uint32_t down = fb == fmin ? NN : fg == fmin ? N : 1u;                          // V3 -> V2
    const uint2 *T = (const uint2 *)(lk.image + LOOK_SHAPER_BYTES) + ((ib * N + ig) * N + ir);
    const uint32_t far = NN + N + 1u;
    const uint2 v0 = T[0], v1 = T[up], v2 = T[far - down], v3 = T[far];
    const uint32_t w0 = 65536u - fmax, w1 = fmax - fmed, w2 = fmed - fmin, w3 = fmin;
    const uint32_t r = look_channel(v0.x & 0xFFFFu, v1.x & 0xFFFFu, v2.x & 0xFFFFu, v3.x & 0xFFFFu, w0, w1, w2, w3);
    const uint32_t g = look_channel(v0.x >> 16, v1.x >> 16, v2.x >> 16, v3.x >> 16, w0, w1, w2, w3);
    const uint32_t b = look_channel(v0.y & 0xFFFFu, v1.y & 0xFFFFu, v2.y & 0xFFFFu, v3.y & 0xFFFFu, w0, w1, w2, w3);
    return r | (g << 8) | (b << 16);
}

// step 4 with a deep look: the three 16-bit samples of one output pixel, R | G << 16 and B, from its three 16-bit indices.  S16 is read
// where it lies: 2-byte gathers through the cache.  lk.n == 0: no table (uniform in a launch).  4b and 4c are look_out's, stated once more
// and not shared with it: look_out routed through a common function -- by reference, by value, with the loads inside or outside -- cost
// k_render1_look_x16 18 VGPRs and an occupancy step
__device__ __forceinline__ uint2 deep_out(const LookArg &lk, uint32_t tr, uint32_t tg, uint32_t tb)
{
    const uint16_t *S = (const uint16_t *)lk.image;
    const uint32_t N = lk.n, NN = N * N, n1 = N - 1u;
    const uint32_t ur = S[tr], ug = S[tg], ub = S[tb];                                    // 4a
    if (!N) return make_uint2(ur | (ug << 16), ub);
    const uint32_t pr = ur * n1, pg = ug * n1, pb = ub * n1;                              // 4b
    const uint32_t ir = pr >> 16, ig = pg >> 16, ib = pb >> 16, fr = pr & 65535u, fg = pg & 65535u, fb = pb & 65535u;
    const uint32_t fmax = max(fr, max(fg, fb)), fmin = min(fr, min(fg, fb)), fmed = max(min(fr, fg), min(max(fr, fg), fb));
    const uint32_t up = fr == fmax ? 1u : fg == fmax ? N : NN;
    const uint32_t down = fb == fmin ? NN : fg == fmin ? N : 1u;
    const uint2 *T = (const uint2 *)(lk.image + LOOK16_SHAPER_BYTES) + ((ib * N + ig) * N + ir);
    const uint32_t far = NN + N + 1u;
    const uint2 v0 = T[0], v1 = T[up], v2 = T[far - down], v3 = T[far];
    const uint32_t w0 = 65536u - fmax, w1 = fmax - fmed, w2 = fmed - fmin, w3 = fmin;
    const uint32_t r = look_vertex_sum(v0.x & 0xFFFFu, v1.x & 0xFFFFu, v2.x & 0xFFFFu, v3.x & 0xFFFFu, w0, w1, w2, w3);
    const uint32_t g = look_vertex_sum(v0.x >> 16, v1.x >> 16, v2.x >> 16, v3.x >> 16, w0, w1, w2, w3);
    const uint32_t b = look_vertex_sum(v0.y & 0xFFFFu, v1.y & 0xFFFFu, v2.y & 0xFFFFu, v3.y & 0xFFFFu, w0, w1, w2, w3);
    return make_uint2(r | (g << 16), b);
}

// steps 3 and 4 of one output pixel from its three 16-bit channels.  Plain and look: bits 0 .. 23, R, G, B from the low byte up -- plain
// three byte reads from the sRGB table, each behind its index (the order the plain kernels always had); look the three indices, then
// look_out.  Deep: deep_out's uint2
template <bool K32, Tone TN>
__device__ __forceinline__ auto tone(const RenderParams &p, const uint8_t *lut, const LookArg &lk, uint32_t m0, uint32_t m1, uint32_t m2)
{
    if constexpr (TN == PLAIN) {
        const uint32_t r = lut[tone_index<K32>(p.K, m0, m1, m2)], g = lut[tone_index<K32>(p.K + 3, m0, m1, m2)], b = lut[tone_index<K32>(p.K + 6, m0, m1, m2)];
        return r | (g << 8) | (b << 16);
    } else if constexpr (TN == LOOK) {
        return look_out(lut, lk, tone_index<K32>(p.K, m0, m1, m2), tone_index<K32>(p.K + 3, m0, m1, m2), tone_index<K32>(p.K + 6, m0, m1, m2));
    } else {
        return deep_out(lk, tone_index16<K32>(p.K, m0, m1, m2), tone_index16<K32>(p.K + 3, m0, m1, m2), tone_index16<K32>(p.K + 6, m0, m1, m2));
    }
}

// ---- how a pixel is written.  8 bits: three bytes; 16 bits: six, little-endian
__device__ __forceinline__ void put_pixel(uint8_t *o, uint32_t v)
{
    o[0] = (uint8_t)v;
    o[1] = (uint8_t)(v >> 8);
    o[2] = (uint8_t)(v >> 16);
}
// any alignment: the generic kernels
__device__ __forceinline__ void put_pixel(uint8_t *o, uint2 v)
{
    o[0] = (uint8_t)v.x; o[1] = (uint8_t)(v.x >> 8); o[2] = (uint8_t)(v.x >> 16); o[3] = (uint8_t)(v.x >> 24);
    o[4] = (uint8_t)v.y; o[5] = (uint8_t)(v.y >> 8);
}
// 8 pixels of a lane of an x16 kernel.  8 bits: 24 bytes as three 64-bit stores (four pixels of 24 bits are three dwords); 16 bits: 48
// bytes as three aligned 128-bit stores (two pixels of 48 bits are three dwords), contiguous across the wave
__device__ __forceinline__ void put_pixels8(void *at, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t p4, uint32_t p5, uint32_t p6, uint32_t p7)
{
    uint2 *o = (uint2 *)at;
    o[0] = make_uint2(p0 | (p1 << 24), (p1 >> 8) | (p2 << 16));
    o[1] = make_uint2((p2 >> 16) | (p3 << 8), p4 | (p5 << 24));
    o[2] = make_uint2((p5 >> 8) | (p6 << 16), (p6 >> 16) | (p7 << 8));
}
__device__ __forceinline__ void put_pixels8(void *at, uint2 p0, uint2 p1, uint2 p2, uint2 p3, uint2 p4, uint2 p5, uint2 p6, uint2 p7)
{
    uint4 *o = (uint4 *)at;
    o[0] = make_uint4(p0.x, p0.y | (p1.x << 16), (p1.x >> 16) | (p1.y << 16), p2.x);
    o[1] = make_uint4(p2.y | (p3.x << 16), (p3.x >> 16) | (p3.y << 16), p4.x, p4.y | (p5.x << 16));
    o[2] = make_uint4((p5.x >> 16) | (p5.y << 16), p6.x, p6.y | (p7.x << 16), (p7.x >> 16) | (p7.y << 16));
}

}  // namespace
}  // namespace mlv

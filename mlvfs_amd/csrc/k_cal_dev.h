// k_cal_dev.h -- the calibration stage's per-pixel definition, shared by the kernels that apply it while a frame
// is loaded: k_cal.hip and the subtracting kernels of k_mlvpack.hip.
#pragma once
#include "common.h"

namespace mlv {

// DARK (stage 0):   clamp(px - dk + black_d, 0, top)                                  black_d: the dark plane's pedestal
// FLAT (stage 0b):  clamp(black + floor(((px - black) * gain + 8192) / 16384), 0, top) on the result; gain is Q14
// WIDE = int: px <= top <= 32767, 0 <= black <= 32767 and gain <= 65535, so the product and the rounding term fit 32 signed bits
// (32767 * 65535 + 8192 < 2^31); WIDE = long long: any depth and black level.  >> of a negative value is arithmetic.
// Without DARK nothing here clamps the input: a caller whose pixels may exceed top (decoded frames may hold anything; the unpack's
// are masked) clamps them first -- clamp_px8.
template <bool DARK, bool FLAT, typename WIDE = int>
__device__ __forceinline__ uint32_t cal_px(uint32_t px, uint32_t dk, uint32_t gain, int black_d, int black, int top)
{
    int v = (int)px;
    if (DARK) v = min(max(v - (int)dk + black_d, 0), top);
    if (FLAT) v = (int)min(max(black + ((((WIDE)v - black) * (WIDE)gain + 8192) >> 14), (WIDE)0), (WIDE)top);
    return (uint32_t)v;
}

// two pixels in a dword
template <bool DARK, bool FLAT>
__device__ __forceinline__ uint32_t cal_px2(uint32_t p, uint32_t d, uint32_t g, int black_d, int black, int top)
{
    return cal_px<DARK, FLAT>(p & 0xFFFFu, d & 0xFFFFu, g & 0xFFFFu, black_d, black, top) |
           (cal_px<DARK, FLAT>(p >> 16, d >> 16, g >> 16, black_d, black, top) << 16);
}

template <bool DARK, bool FLAT>
__device__ __forceinline__ uint4 cal_px8(uint4 p, uint4 d, uint4 g, int black_d, int black, int top)
{
    uint4 r;
    r.x = cal_px2<DARK, FLAT>(p.x, d.x, g.x, black_d, black, top); r.y = cal_px2<DARK, FLAT>(p.y, d.y, g.y, black_d, black, top);
    r.z = cal_px2<DARK, FLAT>(p.z, d.z, g.z, black_d, black, top); r.w = cal_px2<DARK, FLAT>(p.w, d.w, g.w, black_d, black, top);
    return r;
}

__device__ __forceinline__ uint32_t clamp_px2(uint32_t p, uint32_t top) { return min(p & 0xFFFFu, top) | (min(p >> 16, top) << 16); }

__device__ __forceinline__ uint4 clamp_px8(uint4 p, uint32_t top)
{
    uint4 r;
    r.x = clamp_px2(p.x, top); r.y = clamp_px2(p.y, top); r.z = clamp_px2(p.z, top); r.w = clamp_px2(p.w, top);
    return r;
}

}  // namespace mlv

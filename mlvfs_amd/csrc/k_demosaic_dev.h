// k_demosaic_dev.h -- what the kernels that demosaic a strip share (k_demosaic.hip, k_resample.hip): the ring of balanced rows in LDS
// -- a strip of R1_STRIP columns with a 2-pixel halo at both sides, a row loaded by one wave, balanced once and kept as 16 bits -- and
// the Malvar-He-Cutler sums of the 8 pixels of one lane (include/mlvfs_amd.h, "rendered full-size sRGB frames", steps 1 and 2).
#pragma once
#include "k_tone_dev.h"

namespace mlv {
namespace {                    // every including file's own copy

constexpr int R1_STRIP = 512;                         // columns of a workgroup's strip: 64 lanes x 8 pixels
constexpr int R1_RING = 16;                           // rows of the ring: the 12 a step has live (8 read, 4 written), as a power of two
constexpr int R1_PITCH = 8 + R1_STRIP + 8;            // uint16 per ring row: the strip from [8] on, the halos at [6], [7] and behind it

// the index inside 0 .. n - 1 that stands for i in -2 .. n + 1 (n >= 3)
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }

__device__ __forceinline__ uint32_t sixteenths(int s)
{
    const int m = (s + 8) >> 4;
    return (uint32_t)(m < 0 ? 0 : m > 65535 ? 65535 : m);
}

// one source row of the strip as a wave loads it: 8 pixels per lane, and in lanes 0 .. 3 one halo pixel each
struct RowLoad {
    uint4 main;
    uint32_t halo;
};

// row r of the frame (-2 .. h + 1 are reflected); rows behind rmax -- the frame's last row + 2, the run's last row + 2 -- are not needed
// and not read; x0: the strip's first column, sw its width
__device__ __forceinline__ void load_row(RowLoad &v, const uint16_t *src, int w, int h, int r, int rmax, int x0, int sw, int lane)
{
    if (r > rmax) return;
    const uint16_t *row = src + (size_t)reflect(r, h) * w;
    if (8 * lane < sw) v.main = *(const uint4 *)(row + x0 + 8 * lane);
    if (lane < 4) v.halo = row[reflect(lane < 2 ? x0 - 2 + lane : x0 + sw + lane - 2, w)];
}

__device__ __forceinline__ uint32_t balance2(uint32_t d, const Black &bl, int32_t a_even, int32_t a_odd)
{
    return balance(bl(d & 0xFFFFu), a_even) | (balance(bl(d >> 16), a_odd) << 16);
}

// balanced once, into slot `slot` of the ring
__device__ __forceinline__ void store_row(const RowLoad &v, uint16_t *ring, int slot, int r, int rmax, int sw, int lane, const Black &bl, const RenderParams &p)
{
    if (r > rmax) return;
    const bool odd = r & 1;                                   // the reflection keeps the parity
    const int32_t a_even = odd ? p.A[1] : p.A[0], a_odd = odd ? p.A[2] : p.A[1];
    uint16_t *row = ring + slot * R1_PITCH;
    if (8 * lane < sw)
        *(uint4 *)(row + 8 + 8 * lane) = make_uint4(balance2(v.main.x, bl, a_even, a_odd), balance2(v.main.y, bl, a_even, a_odd),
                                                    balance2(v.main.z, bl, a_even, a_odd), balance2(v.main.w, bl, a_even, a_odd));
    if (lane < 4) row[lane < 2 ? 6 + lane : 8 + sw + lane - 2] = (uint16_t)balance(bl(v.halo), (lane & 1) ? a_odd : a_even);
}

__device__ __forceinline__ void unpack8(int *o, const uint4 &v)
{
    o[0] = v.x & 0xFFFFu; o[1] = v.x >> 16; o[2] = v.y & 0xFFFFu; o[3] = v.y >> 16;
    o[4] = v.z & 0xFFFFu; o[5] = v.z >> 16; o[6] = v.w & 0xFFFFu; o[7] = v.w >> 16;
}

// the three 16-bit channels of the 8 pixels of one lane: rows y - 2 .. y + 2 of the ring at m2, m1, c0, p1, p2 (each at the lane's first
// pixel), ODD the row's parity; each(i, m_R, m_G, m_B) takes pixel i
template <bool ODD, class Each>
__device__ __forceinline__ void demosaic8(const uint16_t *m2, const uint16_t *m1, const uint16_t *c0, const uint16_t *p1, const uint16_t *p2, Each &&each)
{
    int a[8], b[10], c[12], d[10], e[8];                      // a, e: columns 0 .. 7; b, d: -1 .. 8; c: -2 .. 9
    unpack8(a, *(const uint4 *)m2);
    unpack8(e, *(const uint4 *)p2);
    unpack8(b + 1, *(const uint4 *)m1);
    unpack8(d + 1, *(const uint4 *)p1);
    unpack8(c + 2, *(const uint4 *)c0);
    b[0] = m1[-1]; b[9] = m1[8];
    d[0] = p1[-1]; d[9] = p1[8];
    const uint32_t cl = *(const uint32_t *)(c0 - 2), cr = *(const uint32_t *)(c0 + 8);
    c[0] = cl & 0xFFFFu; c[1] = cl >> 16; c[10] = cr & 0xFFFFu; c[11] = cr >> 16;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int cc = c[i + 2], h1 = c[i + 1] + c[i + 3], h2 = c[i] + c[i + 4], v1 = b[i + 1] + d[i + 1], v2 = a[i] + e[i];
        const int d1 = b[i] + b[i + 2] + d[i] + d[i + 2];
        uint32_t m0, mg, mb;
        if ((i & 1) == (ODD ? 1 : 0)) {                       // an R site (even row) or a B site (odd row): green and the other colour
            const uint32_t g = sixteenths(8 * cc + 4 * (h1 + v1) - 2 * (h2 + v2)), x = sixteenths(12 * cc + 4 * d1 - 3 * (h2 + v2));
            m0 = ODD ? x : (uint32_t)cc; mg = g; mb = ODD ? (uint32_t)cc : x;
        } else {                                              // a green site: the colour of its row and the colour of its column
            const uint32_t sh = sixteenths(10 * cc + 8 * h1 - 2 * d1 - 2 * h2 + v2), sv = sixteenths(10 * cc + 8 * v1 - 2 * d1 - 2 * v2 + h2);
            m0 = ODD ? sv : sh; mg = (uint32_t)cc; mb = ODD ? sh : sv;
        }
        each(i, m0, mg, mb);
    }
}

}  // namespace
}  // namespace mlv

// k_demosaic.hip -- rendered full-size sRGB frames: the frames the mount serves, developed to 8-bit RGB at the size they were shot
// (include/mlvfs_amd.h, "rendered full-size sRGB frames").  A W x H RGGB frame becomes W x H pixels of 3 bytes:
//     b(y, x) = min((max(in(y, x) - black, 0) * A_j + 2048) >> 12, 65535)     j = (y & 1) + (x & 1)      (the product in 64 bits)
//     b outside the frame: reflected about the edge pixel (-1 -> 1, n -> n - 2)
//     the Malvar-He-Cutler 5x5 filter in sixteenths, c = b(y, x), h1 / v1 / d1 the neighbours at distance 1, h2 / v2 at distance 2:
//         sG = 8c + 4(h1 + v1) - 2(h2 + v2)     sH = 10c + 8 h1 - 2 d1 - 2 h2 + v2     sV = 10c + 8 v1 - 2 d1 - 2 v2 + h2
//         sD = 12c + 4 d1 - 3(h2 + v2)          m = clamp((s + 8) >> 4, 0, 65535), or c for the site's own channel
//     t_i = clamp((sum_j K[i][j] * m_j + 32768) >> 16, 0, 4095)     out_i = LUT[t_i]
// black, A[3], K[9]: the half-size rendering's 13 int32 per frame (mlvfs_amd_rgb_params), uniform in a workgroup.
//
// The first stencil of the rendered routes.  Frames are batched in grid.y, never in place, no scratch, the 4 KiB LUT in LDS.
//   k_render1_x16     : W % 16 == 0, source base and stride 16-byte, destination base and stride 8-byte aligned.  A workgroup of four
//                       waves owns a strip of R1_STRIP columns and walks down R1_RUN rows of it, four rows a step, one row per wave.
//                       Every source pixel it loads is balanced once (the 64-bit multiply) and kept as 16 bits in a ring of R1_RING
//                       rows in LDS with a 2-pixel halo at both sides; a step's loads are issued before its arithmetic and stored
//                       behind it, one barrier a step.  A lane produces an even-aligned group of 8 pixels of its wave's row -- the
//                       CFA site of each is a compile-time fact, the row's parity is uniform in the wave -- = 24 bytes: three 64-bit
//                       stores; a wave reads 1 KiB contiguous of a source row and writes 1.5 KiB contiguous.  Source bytes read:
//                       (R1_RUN + 4) / R1_RUN rows of (R1_STRIP + 4) / R1_STRIP columns = 1.13 frames.
//                       Where sum_j |K[i][j]| * 65535 + 32768 < 2^31 for every i (uniform: taken per frame from the parameters) step 3
//                       runs in 24-bit multiplies and 32-bit sums, otherwise in 64 bits; the results are the same.
//   k_render1_generic : any W, H >= 4, 2-byte source alignment, 1-byte destination alignment; one lane = one output pixel, the 13
//                       taps straight from global memory with the reflection applied to the indices.
// Bytes between frames and behind 3 * W * H are never touched.
// k_render1_look_x16, k_render1_look_generic: the same bodies with a look as step 4 (k_tone_dev.h).
// k_render1_deep_x16, k_render1_deep_generic: the same bodies with the 16-bit form of steps 3 and 4 and 6 bytes per pixel -- a lane of
// the x16 form writes 48 bytes as three 128-bit stores, so its destination base and stride are 16-byte aligned (one that is only 8-byte
// aligned takes the generic kernel); no table in LDS.
#include "k_demosaic_dev.h"

namespace mlv {

namespace {                    // this file's device helpers

constexpr int R1_RUN = 32;                            // rows a workgroup walks down

// ---- k_render1_x16 (the ring and the filter: k_demosaic_dev.h)
// the 8 pixels of one lane: rows y - 2 .. y + 2 of the ring at m2, m1, c0, p1, p2 (each at the lane's first pixel).  ODD: the row's parity.
// (demosaic8 of k_demosaic_dev.h is the same filter handing its channels on; routed through it this kernel's registers change)
template <bool ODD, bool K32, Tone TN>
__device__ __forceinline__ void develop8(const uint16_t *m2, const uint16_t *m1, const uint16_t *c0, const uint16_t *p1, const uint16_t *p2,
                                         const RenderParams &p, const uint8_t *lut, const LookArg &lk, uint8_t *o)
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
    decltype(tone<K32, TN>(p, lut, lk, 0u, 0u, 0u)) px[8];
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
        px[i] = tone<K32, TN>(p, lut, lk, m0, mg, mb);
    }
    put_pixels8(o, px[0], px[1], px[2], px[3], px[4], px[5], px[6], px[7]);
}

// rows y0 .. y0 + R1_RUN - 1 of columns x0 .. x0 + sw - 1.  The ring's slot of row r: (r - y0 + 2) & (R1_RING - 1).
template <bool K32, Tone TN>
__device__ __forceinline__ void walk_strip(const uint16_t *src, uint8_t *dst, int w, int h, int x0, int sw, int y0, const RenderParams &p,
                                           const Black &bl, uint16_t *ring, const uint8_t *lut, const LookArg &lk)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rmax = min(h, y0 + R1_RUN) + 1;
    RowLoad v = {};
    // rows y0 - 2 .. y0 + 5: what the first step reads
    for (int k = 0; k < 2; k++) {
        const int r = y0 - 2 + 4 * k + wave;
        load_row(v, src, w, h, r, rmax, x0, sw, lane);
        store_row(v, ring, 4 * k + wave, r, rmax, sw, lane, bl, p);
    }
    __syncthreads();
    for (int y = y0 + wave; y < y0 + R1_RUN; y += 4) {        // y - wave is uniform in the workgroup: every wave meets every barrier
        const int rn = y + 6;                                 // the row this wave fetches for the next step
        load_row(v, src, w, h, rn, rmax, x0, sw, lane);
        if (y < h && 8 * lane < sw) {
            const int s = y - y0 + 2;
            const uint16_t *at = ring + 8 + 8 * lane;
            const uint16_t *m2 = at + ((s - 2) & (R1_RING - 1)) * R1_PITCH, *m1 = at + ((s - 1) & (R1_RING - 1)) * R1_PITCH;
            const uint16_t *c0 = at + (s & (R1_RING - 1)) * R1_PITCH;
            const uint16_t *p1 = at + ((s + 1) & (R1_RING - 1)) * R1_PITCH, *p2 = at + ((s + 2) & (R1_RING - 1)) * R1_PITCH;
            uint8_t *o = dst + ((size_t)y * w + x0 + 8 * lane) * (TN == DEEP ? 6 : 3);
            if (y & 1) develop8<true, K32, TN>(m2, m1, c0, p1, p2, p, lut, lk, o);
            else develop8<false, K32, TN>(m2, m1, c0, p1, p2, p, lut, lk, o);
        }
        store_row(v, ring, (rn - y0 + 2) & (R1_RING - 1), rn, rmax, sw, lane, bl, p);
        __syncthreads();
    }
}

// grid.x = strips * runs, strips side by side first
template <Tone TN>
__device__ __forceinline__ void render1_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                            uint8_t *__restrict__ out, size_t out_stride, int w, int h, uint32_t strips, uint8_t *lut, uint16_t *ring,
                                            const LookArg &lk)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    const int run = blockIdx.x / strips, x0 = (int)(blockIdx.x - run * strips) * R1_STRIP, sw = min(w - x0, R1_STRIP);
    if (fits32(p)) walk_strip<true, TN>(src, dst, w, h, x0, sw, run * R1_RUN, p, bl, ring, lut, lk);
    else walk_strip<false, TN>(src, dst, w, h, x0, sw, run * R1_RUN, p, bl, ring, lut, lk);
}

// ---- k_render1_generic
// npix = W * H output pixels per frame
template <Tone TN>
__device__ __forceinline__ void render1_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, int w, int h, uint8_t *lut,
                                                const LookArg &lk, uint32_t first, uint32_t step, int32_t *site_a)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    if constexpr (TN != PLAIN) {
        if (threadIdx.x == 0) { site_a[0] = p.A[0]; site_a[1] = site_a[2] = p.A[1]; site_a[3] = p.A[2]; }
        __syncthreads();
    }
    for (uint32_t k = first; k < npix; k += step) {
        const int y = (int)(k / (uint32_t)w), x = (int)(k - (uint32_t)y * (uint32_t)w);
        // the balanced sample at (y + dy, x + dx): its site's colour is that of the reflected position too.  (The compiler turns the
        // three-way choice among p.A into a table per lane: in LDS in the plain kernel, as ever, but in scratch in the look kernel, which
        // therefore reads A by site from a table of its own in LDS, as the deep kernel does)
        auto tap = [&](int dy, int dx) __attribute__((always_inline)) -> int {
            const int yy = reflect(y + dy, h), xx = reflect(x + dx, w);
            const int j = (yy & 1) + (xx & 1);
            if constexpr (TN != PLAIN) return (int)balance(bl(src[(size_t)yy * w + xx]), site_a[2 * (yy & 1) + (xx & 1)]);
            return (int)balance(bl(src[(size_t)yy * w + xx]), j == 0 ? p.A[0] : j == 1 ? p.A[1] : p.A[2]);
        };
        const int c = tap(0, 0), h1 = tap(0, -1) + tap(0, 1), v1 = tap(-1, 0) + tap(1, 0), h2 = tap(0, -2) + tap(0, 2), v2 = tap(-2, 0) + tap(2, 0);
        const int d1 = tap(-1, -1) + tap(-1, 1) + tap(1, -1) + tap(1, 1);
        const uint32_t sg = sixteenths(8 * c + 4 * (h1 + v1) - 2 * (h2 + v2)), sd = sixteenths(12 * c + 4 * d1 - 3 * (h2 + v2));
        const uint32_t sh = sixteenths(10 * c + 8 * h1 - 2 * d1 - 2 * h2 + v2), sv = sixteenths(10 * c + 8 * v1 - 2 * d1 - 2 * v2 + h2);
        const bool yo = y & 1, xo = x & 1;
        const uint32_t m0 = yo ? (xo ? sd : sv) : (xo ? sh : (uint32_t)c);
        const uint32_t m1 = yo == xo ? sg : (uint32_t)c;
        const uint32_t m2 = yo ? (xo ? (uint32_t)c : sh) : (xo ? sv : sd);
        put_pixel(dst + (size_t)k * (TN == DEEP ? 6 : 3), tone<false, TN>(p, lut, lk, m0, m1, m2));
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_render1_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                     uint8_t *__restrict__ out, size_t out_stride, int w, int h, uint32_t strips)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    __shared__ __attribute__((aligned(16))) uint16_t ring[R1_RING * R1_PITCH];
    render1_x16<PLAIN>(frames, stride, params, out, out_stride, w, h, strips, lut, ring, LookArg());
}

__global__ __launch_bounds__(256) void k_render1_look_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                          uint8_t *__restrict__ out, size_t out_stride, int w, int h, uint32_t strips, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    __shared__ __attribute__((aligned(16))) uint16_t ring[R1_RING * R1_PITCH];
    render1_x16<LOOK>(frames, stride, params, out, out_stride, w, h, strips, lut, ring, lk);
}

// the 16-bit form: the ring alone in LDS; the destination base and stride 16-byte aligned
__global__ __launch_bounds__(256) void k_render1_deep_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                          uint8_t *__restrict__ out, size_t out_stride, int w, int h, uint32_t strips, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint16_t ring[R1_RING * R1_PITCH];
    render1_x16<DEEP>(frames, stride, params, out, out_stride, w, h, strips, nullptr, ring, lk);
}

__global__ __launch_bounds__(256) void k_render1_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                         uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, int w, int h)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    render1_generic<PLAIN>(frames, stride, params, out, out_stride, npix, w, h, lut, LookArg(), MLV_GRID_STRIDE, nullptr);
}

__global__ __launch_bounds__(256) void k_render1_look_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                              uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, int w, int h, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    __shared__ int32_t site_a[4];                             // A of the four CFA sites, [2 * (y & 1) + (x & 1)]
    render1_generic<LOOK>(frames, stride, params, out, out_stride, npix, w, h, lut, lk, MLV_GRID_STRIDE, site_a);
}

__global__ __launch_bounds__(256) void k_render1_deep_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                              uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, int w, int h, const LookArg lk)
{
    __shared__ int32_t site_a[4];                             // A of the four CFA sites, [2 * (y & 1) + (x & 1)]
    render1_generic<DEEP>(frames, stride, params, out, out_stride, npix, w, h, nullptr, lk, MLV_GRID_STRIDE, site_a);
}

// d_out apart from d_frames (the callers check); w, h >= 4, w * h < 2^25; d_params: 13 int32 per frame, 4-byte aligned
int launch_render1(const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h, int nframes,
                   hipStream_t stream, const LookArg *lk, bool deep)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (!rgb_full_geom(w, h)) return route_refuse("launch_render1", { RenderRoute::FULL }, w, h);
    const size_t oa = deep ? 16 : 8;                                                     // what the fast form's stores need
    const bool fast = w % 16 == 0 && ((uintptr_t)d_frames % 16 == 0) && ((uintptr_t)d_out % oa == 0) &&
                      (nframes == 1 || (stride % 16 == 0 && out_stride % oa == 0));
    if (fast) {
        const uint32_t strips = ((uint32_t)w + R1_STRIP - 1) / R1_STRIP, runs = ((uint32_t)h + R1_RUN - 1) / R1_RUN;
        launch_tone(k_render1_deep_x16, k_render1_look_x16, k_render1_x16, dim3(strips * runs, nframes), stream, lk, deep, (const uint8_t *)d_frames,
                    stride, (const RenderParams *)d_params, (uint8_t *)d_out, out_stride, w, h, strips);
    } else {
        // the workgroups of a launch share the machine: each of them stages the table once, and the lanes stride over the rest
        const uint32_t npix = (uint32_t)w * (uint32_t)h, cap = 4 * std::max(2048u / (uint32_t)nframes, 64u);
        const dim3 grid(std::min<uint32_t>((npix + 255) / 256, cap), nframes);
        launch_tone(k_render1_deep_generic, k_render1_look_generic, k_render1_generic, grid, stream, lk, deep, (const uint8_t *)d_frames, stride,
                    (const RenderParams *)d_params, (uint8_t *)d_out, out_stride, npix, w, h);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

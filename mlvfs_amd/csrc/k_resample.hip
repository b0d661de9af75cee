// k_resample.hip -- rendered frames resampled from the full-size rendering: the three demosaiced 16-bit channels of the full-size
// definition, area-averaged in linear light to ow x oh pixels, any size from 1x1 up to the frame's own, between the demosaic and the
// matrix (include/mlvfs_amd.h, "rendered frames resampled from the full-size rendering").
//     d_c(y, x)  = the full-size definition's steps 1 and 2 on the W x H grid (balanced at the site, reflected border, MHC in sixteenths)
//     wx(u, x)   = max(0, min((x + 1) ow, (u + 1) W) - max(x ow, u W))             wy(v, y) likewise with H, oh
//     hd_c(y, u) = floor((sum_x wx(u, x) d_c(y, x) + (W >> 1)) / W)                32 bits unsigned hold every sum
//     m_c(v, u)  = floor((sum_y wy(v, y) hd_c(y, u) + (H >> 1)) / H)
//     t_i = clamp((sum_j K[i][j] * m_j + 32768) >> 16, 0, 4095)     out_i = LUT[t_i]
// black, A[3], K[9]: the half-size rendering's 13 int32 per frame (mlvfs_amd_rgb_params), uniform in a workgroup.
//
// One pass, no plane in between.  Frames are batched in grid.y, never in place, no scratch.
//   k_resample_x16     : W % 16 == 0, source base and stride 16-byte aligned, 2 ow >= W -- so that an output column's span is at most
//                        three source pixels and the horizontal pass has no loop.  A workgroup of four waves owns a strip of `uo`
//                        output columns (at most RS_NOUT per lane, lane l the columns us0 + l + 256 i) and a band of `bo` output rows,
//                        and walks down the source rows the band covers, RS_ROWS a step, one per wave.  The strip's source columns,
//                        from a multiple of 8 to a multiple of 8, are at most RS_STRIP; every source pixel is balanced once and kept
//                        in k_render1_x16's ring (k_demosaic_dev.h).  A wave demosaics its row -- a lane 8 pixels -- into three 16-bit
//                        planes in LDS, one set of them (two would cost the fourth workgroup of a CU), so a step has two barriers.
//                        Between them a lane takes the step's rows top down: per column and channel three products, one division by W, wy hd added to the column's sum;
//                        with the last source row of an output row it divides by H, develops and stores, and the part of that source
//                        row which belongs to the next output row starts the next sum (oh <= H: a source row meets at most two).
//                        A source row that straddles two bands is demosaiced by both.  Both divisions are sc_div's (k_scale_dev.h).
//                        The matrix runs in 32 bits where the frame's K allows it (fits32), as in k_render1_x16.
//   k_resample_generic : any W, H >= 4, any size, 2-byte source alignment; one lane = one output pixel, every pixel of its footprint
//                        demosaiced from global memory with the reflection applied to the indices, both divisions with the plain
//                        operator.
// Bytes between renderings and behind 3 * ow * oh are never touched.
// k_resample_look_x16, k_resample_look_generic: the same bodies with a look as step 4 (k_tone_dev.h).
// k_resample_deep_x16, k_resample_deep_generic: the same bodies with the 16-bit form of steps 3 and 4 and 6 bytes per pixel -- a lane of
// the x16 form writes three 16-bit values where it wrote three bytes, so its destination base and stride are 2-byte aligned (an odd one
// takes the generic kernel); no table in LDS.
#include "k_demosaic_dev.h"
#include "k_scale_dev.h"

namespace mlv {

struct ResampleArgs {          // uniform in a launch
    uint32_t w, h, ow, oh;
    uint32_t uo, nstrips, bo;                         // output columns of a strip, strips of a row, output rows of a band
    ScDiv dw, dh;                                     // / W, / H
};

namespace {                    // this file's device helpers

static_assert(RS_STRIP == R1_STRIP && RS_ROWS == 4, "the strip is the ring's, a step is one row per wave");
constexpr int RS_NOUT = 2;                            // output columns of a lane: uo <= RS_STRIP - 16
constexpr int RS_PITCH = RS_STRIP + 8;                // uint16 per plane: a span may name two columns behind its first

// one row of the strip demosaiced into its three planes; pl: the R plane at the lane's first pixel
template <bool ODD>
__device__ __forceinline__ void demosaic_row(const uint16_t *m2, const uint16_t *m1, const uint16_t *c0, const uint16_t *p1, const uint16_t *p2,
                                             uint16_t *pl)
{
    uint32_t ch[3][8];
    demosaic8<ODD>(m2, m1, c0, p1, p2, [&](int i, uint32_t m0, uint32_t mg, uint32_t mb) __attribute__((always_inline)) {
        ch[0][i] = m0; ch[1][i] = mg; ch[2][i] = mb;
    });
#pragma unroll
    for (int j = 0; j < 3; j++)
        *(uint4 *)(pl + j * RS_PITCH) = make_uint4(ch[j][0] | (ch[j][1] << 16), ch[j][2] | (ch[j][3] << 16), ch[j][4] | (ch[j][5] << 16),
                                                   ch[j][6] | (ch[j][7] << 16));
}

// grid.x = strips * bands, strips side by side first
template <Tone TN>
__device__ __forceinline__ void resample_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                             uint8_t *__restrict__ out, size_t out_stride, const ResampleArgs &a, uint8_t *lut, uint16_t *ring,
                                             uint16_t (*planes)[3][RS_PITCH], const LookArg &lk)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const bool k32 = fits32(p);                                                              // uniform: the matrix in 24-bit multiplies
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    const int w = (int)a.w, h = (int)a.h;
    const uint32_t band = blockIdx.x / a.nstrips, strip = blockIdx.x - band * a.nstrips;
    const uint32_t us0 = strip * a.uo, us1 = min(us0 + a.uo, a.ow);                          // the strip's output columns
    const uint32_t v0 = band * a.bo, v1 = min(v0 + a.bo, a.oh);                              // the band's output rows
    // the source columns the strip covers, from a multiple of 8 to a multiple of 8 (W % 8 == 0: inside the frame), and the source rows
    // the band covers.  Every product here is at most ow W or oh H, below 2^32
    const uint32_t xs1 = (us1 * a.w - 1u) / a.ow + 1u;
    const int x0 = (int)((us0 * a.w / a.ow) & ~7u), sw = min((int)((xs1 + 7u) & ~7u) - x0, RS_STRIP);
    const int y0 = (int)(v0 * a.h / a.oh), y1 = (int)((v1 * a.h - 1u) / a.oh) + 1;
    // this lane's columns: where the span begins in the planes, and its three weights (they sum to W); a column outside the strip has none
    uint32_t xi[RS_NOUT], wa[RS_NOUT], wb[RS_NOUT], wc[RS_NOUT];
#pragma unroll
    for (int i = 0; i < RS_NOUT; i++) {
        const uint32_t u = us0 + threadIdx.x + 256u * i;
        const bool mine = u < us1;
        const uint32_t lo = mine ? u * a.w : 0u, hi = lo + a.w, xl = lo / a.ow, e1 = min((xl + 1u) * a.ow, hi), e2 = min((xl + 2u) * a.ow, hi);
        xi[i] = mine ? min(xl - (uint32_t)x0, (uint32_t)RS_STRIP - 1u) : 0u;                     // the plan keeps it below sw: a bound for the read
        wa[i] = mine ? e1 - lo : 0u;
        wb[i] = mine ? e2 - e1 : 0u;
        wc[i] = mine ? hi - e2 : 0u;
    }
    uint32_t vacc[RS_NOUT][3] = {};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rmax = min(h, y1) + 1;
    RowLoad ld = {};
    // rows y0 - 2 .. y0 + 5: what the first step reads.  The ring's slot of row r: (r - y0 + 2) & (R1_RING - 1)
    for (int k = 0; k < 2; k++) {
        const int r = y0 - 2 + 4 * k + wave;
        load_row(ld, src, w, h, r, rmax, x0, sw, lane);
        store_row(ld, ring, 4 * k + wave, r, rmax, sw, lane, bl, p);
    }
    __syncthreads();
    uint32_t v = v0;
    for (int yb = y0; yb < y1; yb += RS_ROWS) {                                              // uniform: every wave meets every barrier
        const int y = yb + wave, rn = y + 6;                                                 // this wave's row, and the one it fetches
        load_row(ld, src, w, h, rn, rmax, x0, sw, lane);
        if (y < y1 && 8 * lane < sw) {
            const int s = y - y0 + 2;
            const uint16_t *at = ring + 8 + 8 * lane;
            const uint16_t *m2 = at + ((s - 2) & (R1_RING - 1)) * R1_PITCH, *m1 = at + ((s - 1) & (R1_RING - 1)) * R1_PITCH;
            const uint16_t *c0 = at + (s & (R1_RING - 1)) * R1_PITCH;
            const uint16_t *p1 = at + ((s + 1) & (R1_RING - 1)) * R1_PITCH, *p2 = at + ((s + 2) & (R1_RING - 1)) * R1_PITCH;
            uint16_t *pl = &planes[wave][0][8 * lane];
            if (y & 1) demosaic_row<true>(m2, m1, c0, p1, p2, pl);
            else demosaic_row<false>(m2, m1, c0, p1, p2, pl);
        }
        store_row(ld, ring, (rn - y0 + 2) & (R1_RING - 1), rn, rmax, sw, lane, bl, p);
        __syncthreads();
        // the step's rows top down
        for (int r = 0; r < RS_ROWS && yb + r < y1 && v < v1; r++) {                         // v < v1 holds by construction: a bound for the stores
            const uint32_t e = (uint32_t)(yb + r) * a.oh, vlo = v * a.h, vhi = vlo + a.h;
            const uint32_t wy = min(e + a.oh, vhi) - max(e, vlo);
            const bool last = e + a.oh >= vhi;                                               // of output row v
            const uint32_t wnext = e + a.oh - min(e + a.oh, vhi);                            // what of the row belongs to v + 1
#pragma unroll
            for (int i = 0; i < RS_NOUT; i++) {
                const uint32_t u = us0 + threadIdx.x + 256u * i;
                if (u < us1) {
                    uint32_t hd[3];
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const uint16_t *q = &planes[r][j][xi[i]];
                        const uint32_t sum = __umul24(wa[i], q[0]) + __umul24(wb[i], q[1]) + __umul24(wc[i], q[2]);   // factors below 2^16
                        hd[j] = sc_div(sum + (a.w >> 1), a.dw);
                        vacc[i][j] += __umul24(wy, hd[j]);
                    }
                    if (last) {
                        const uint32_t m0 = sc_div(vacc[i][0] + (a.h >> 1), a.dh), m1 = sc_div(vacc[i][1] + (a.h >> 1), a.dh);
                        const uint32_t m2 = sc_div(vacc[i][2] + (a.h >> 1), a.dh);
                        const auto px = k32 ? tone<true, TN>(p, lut, lk, m0, m1, m2) : tone<false, TN>(p, lut, lk, m0, m1, m2);
                        if constexpr (TN == DEEP) {                                          // the same columns, stores twice as wide
                            uint16_t *o = (uint16_t *)(dst + ((size_t)v * a.ow + u) * 6);
                            o[0] = (uint16_t)px.x;
                            o[1] = (uint16_t)(px.x >> 16);
                            o[2] = (uint16_t)px.y;
                        } else {
                            put_pixel(dst + ((size_t)v * a.ow + u) * 3, px);
                        }
#pragma unroll
                        for (int j = 0; j < 3; j++) vacc[i][j] = __umul24(wnext, hd[j]);
                    }
                }
            }
            if (last) v++;
        }
        __syncthreads();                                                                     // the next step writes the planes
    }
}

// ---- k_resample_generic
// npix = ow * oh output pixels per frame; site_a: A of the four CFA sites in LDS, [2 * (y & 1) + (x & 1)]
template <Tone TN>
__device__ __forceinline__ void resample_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                 uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, int w, int h, uint32_t ow,
                                                 uint32_t oh, uint8_t *lut, const LookArg &lk, uint32_t first, uint32_t step, int32_t *site_a)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    if (threadIdx.x == 0) { site_a[0] = p.A[0]; site_a[1] = site_a[2] = p.A[1]; site_a[3] = p.A[2]; }
    __syncthreads();
    const uint32_t uw = (uint32_t)w, uh = (uint32_t)h;
    for (uint32_t k = first; k < npix; k += step) {
        const uint32_t v = k / ow, u = k - v * ow;
        const uint32_t ulo = u * uw, uhi = ulo + uw, vlo = v * uh, vhi = vlo + uh;
        const uint32_t xlo = ulo / ow, xhi = (uhi - 1u) / ow, ylo = vlo / oh, yhi = (vhi - 1u) / oh;
        uint32_t m[3] = { 0, 0, 0 };
        for (uint32_t yy = ylo; yy <= yhi; yy++) {
            const uint32_t wy = min((yy + 1u) * oh, vhi) - max(yy * oh, vlo);
            uint32_t s[3] = { 0, 0, 0 };
            for (uint32_t xx = xlo; xx <= xhi; xx++) {
                const uint32_t wx = min((xx + 1u) * ow, uhi) - max(xx * ow, ulo);
                const int y = (int)yy, x = (int)xx;
                // the balanced sample at (y + dy, x + dx): its site's colour is that of the reflected position too
                auto tap = [&](int dy, int dx) __attribute__((always_inline)) -> int {
                    const int ty = reflect(y + dy, h), tx = reflect(x + dx, w);
                    return (int)balance(bl(src[(size_t)ty * w + tx]), site_a[2 * (ty & 1) + (tx & 1)]);
                };
                const int c = tap(0, 0), h1 = tap(0, -1) + tap(0, 1), v1 = tap(-1, 0) + tap(1, 0), h2 = tap(0, -2) + tap(0, 2), v2 = tap(-2, 0) + tap(2, 0);
                const int d1 = tap(-1, -1) + tap(-1, 1) + tap(1, -1) + tap(1, 1);
                const uint32_t sg = sixteenths(8 * c + 4 * (h1 + v1) - 2 * (h2 + v2)), sd = sixteenths(12 * c + 4 * d1 - 3 * (h2 + v2));
                const uint32_t sh = sixteenths(10 * c + 8 * h1 - 2 * d1 - 2 * h2 + v2), sv = sixteenths(10 * c + 8 * v1 - 2 * d1 - 2 * v2 + h2);
                const bool yo = y & 1, xo = x & 1;
                s[0] += wx * (yo ? (xo ? sd : sv) : (xo ? sh : (uint32_t)c));
                s[1] += wx * (yo == xo ? sg : (uint32_t)c);
                s[2] += wx * (yo ? (xo ? (uint32_t)c : sh) : (xo ? sv : sd));
            }
            for (int j = 0; j < 3; j++) m[j] += wy * ((s[j] + (uw >> 1)) / uw);
        }
        put_pixel(dst + (size_t)k * (TN == DEEP ? 6 : 3),
                  tone<false, TN>(p, lut, lk, (m[0] + (uh >> 1)) / uh, (m[1] + (uh >> 1)) / uh, (m[2] + (uh >> 1)) / uh));
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_resample_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                      uint8_t *__restrict__ out, size_t out_stride, const ResampleArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    __shared__ __attribute__((aligned(16))) uint16_t ring[R1_RING * R1_PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t planes[RS_ROWS][3][RS_PITCH];
    resample_x16<PLAIN>(frames, stride, params, out, out_stride, a, lut, ring, planes, LookArg());
}

__global__ __launch_bounds__(256) void k_resample_look_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                           uint8_t *__restrict__ out, size_t out_stride, const ResampleArgs a, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    __shared__ __attribute__((aligned(16))) uint16_t ring[R1_RING * R1_PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t planes[RS_ROWS][3][RS_PITCH];
    resample_x16<LOOK>(frames, stride, params, out, out_stride, a, lut, ring, planes, lk);
}

// the 16-bit form: the ring and the planes alone in LDS; the destination base and stride 2-byte aligned
__global__ __launch_bounds__(256) void k_resample_deep_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                           uint8_t *__restrict__ out, size_t out_stride, const ResampleArgs a, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint16_t ring[R1_RING * R1_PITCH];
    __shared__ __attribute__((aligned(16))) uint16_t planes[RS_ROWS][3][RS_PITCH];
    resample_x16<DEEP>(frames, stride, params, out, out_stride, a, nullptr, ring, planes, lk);
}

__global__ __launch_bounds__(256) void k_resample_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                          uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, int w, int h, uint32_t ow,
                                                          uint32_t oh)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    __shared__ int32_t site_a[4];
    resample_generic<PLAIN>(frames, stride, params, out, out_stride, npix, w, h, ow, oh, lut, LookArg(), MLV_GRID_STRIDE, site_a);
}

__global__ __launch_bounds__(256) void k_resample_look_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                               uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, int w, int h, uint32_t ow,
                                                               uint32_t oh, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    __shared__ int32_t site_a[4];
    resample_generic<LOOK>(frames, stride, params, out, out_stride, npix, w, h, ow, oh, lut, lk, MLV_GRID_STRIDE, site_a);
}

__global__ __launch_bounds__(256) void k_resample_deep_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                               uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, int w, int h, uint32_t ow,
                                                               uint32_t oh, const LookArg lk)
{
    __shared__ int32_t site_a[4];
    resample_generic<DEEP>(frames, stride, params, out, out_stride, npix, w, h, ow, oh, nullptr, lk, MLV_GRID_STRIDE, site_a);
}

// d_out apart from d_frames (the callers check); d_params: 13 int32 per frame, 4-byte aligned
int launch_render_resampled(const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h, int ow,
                            int oh, int nframes, hipStream_t stream, const LookArg *lk, bool deep)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (!resample_geom(w, h, ow, oh)) return route_refuse("launch_render_resampled", { RenderRoute::RESAMPLED, false, ow, oh }, w, h);
    const bool fast = resample_fast_geom(w, ow) && ((uintptr_t)d_frames % 16 == 0) && (nframes == 1 || stride % 16 == 0) &&
                      (!deep || ((uintptr_t)d_out % 2 == 0 && (nframes == 1 || out_stride % 2 == 0)));      // 16-bit stores
    if (fast) {
        const ResamplePlan pl = resample_plan(w, h, ow, oh, nframes);
        const ResampleArgs a{ (uint32_t)w, (uint32_t)h, (uint32_t)ow, (uint32_t)oh, pl.uo, pl.nstrips, pl.bo, scdiv_make((uint32_t)w), scdiv_make((uint32_t)h) };
        const dim3 grid(pl.nstrips * pl.nbands, nframes);
        launch_tone(k_resample_deep_x16, k_resample_look_x16, k_resample_x16, grid, stream, lk, deep, (const uint8_t *)d_frames, stride,
                    (const RenderParams *)d_params, (uint8_t *)d_out, out_stride, a);
    } else {
        const uint32_t npix = (uint32_t)ow * (uint32_t)oh, cap = std::max(2048u / (uint32_t)nframes, 64u);
        const dim3 grid(std::min<uint32_t>((npix + 255) / 256, 4 * cap), nframes);
        launch_tone(k_resample_deep_generic, k_resample_look_generic, k_resample_generic, grid, stream, lk, deep, (const uint8_t *)d_frames, stride,
                    (const RenderParams *)d_params, (uint8_t *)d_out, out_stride, npix, w, h, (uint32_t)ow, (uint32_t)oh);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

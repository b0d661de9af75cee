// k_scale.hip -- rendered frames at any smaller size: the half-size rendering's balanced superpixels, area-averaged in linear light to
// ow x oh pixels between the balance and the matrix (include/mlvfs_amd.h, "rendered frames at any smaller size").
//     n_j(Y, X)  = the half-size definition's steps 1 and 2 on the W' x H' grid
//     wx(u, X)   = max(0, min((X + 1) ow, (u + 1) W') - max(X ow, u W'))           wy(v, Y) likewise with H', oh
//     hm_j(Y, u) = floor((sum_X wx(u, X) n_j(Y, X) + (W' >> 1)) / W')              32 bits unsigned hold every sum
//     m_j(v, u)  = floor((sum_Y wy(v, Y) hm_j(Y, u) + (H' >> 1)) / H')
//     t_i = clamp((sum_j K[i][j] * m_j + 32768) >> 16, 0, 4095)     out_i = LUT[t_i]
// black, A[3], K[9]: the half-size rendering's 13 int32 per frame (mlvfs_amd_rgb_params), uniform in a workgroup.
//
// One pass, no plane in between.  Frames are batched in grid.y, never in place, no scratch, the 4 KiB LUT in LDS.
//   k_scale_x16     : W % 16 == 0, source base and stride 16-byte aligned.  A workgroup owns a strip of `uo` output columns (at most
//                     SC_STRIP, SC_NOUT per lane, lane l the columns us0 + l + 256 i) and a band of `bo` output rows, and walks down
//                     the source superpixel rows the band covers.  A step stages SC_CHUNK superpixels of one row: a lane loads 8
//                     pixels of each of the row's two raw rows (one 128-bit load each; a wave reads 1 KiB contiguous of both),
//                     balances its 4 superpixels and puts them as 16 bits into three planes in LDS.  Two buffers alternate, so a
//                     step has one barrier, and the next step's loads are issued in front of it.  Behind it a lane adds the part
//                     of each of its columns' spans that lies in the chunk; the launch sizes the strips so that a row is one chunk
//                     wherever one column's span fits one, and any number of chunks is walked where it does not.  With
//                     a row's last chunk the lane divides once per column and channel and adds wy hm to the column's sum; with the
//                     last source row of an output row it divides again, develops and stores 3 bytes, and the part of that source
//                     row which belongs to the next output row starts the next sum (oh <= H': a source row meets at most two).
//                     A source row that straddles two bands is read by both.  Both divisions are by a launch-wide constant and
//                     run as a multiplication that is exact for every 32-bit numerator (sc_div).  Where sum_j |K[i][j]| * 65535 +
//                     32768 < 2^31 for every i (uniform: taken per frame from the parameters) step 3 runs in 24-bit multiplies and
//                     32-bit sums, otherwise in 64 bits, as in k_render1_x16; the results are the same.
//   k_scale_generic : any W, H >= 2, 2-byte source alignment; one lane = one output pixel, its footprint straight from global memory,
//                     both divisions with the plain operator.
// Bytes between renderings and behind 3 * ow * oh are never touched.
// k_scale_look_x16, k_scale_look_generic: the same bodies with a look as step 4 (k_tone_dev.h).
// k_scale_deep_x16, k_scale_deep_generic: the same bodies with the 16-bit form of steps 3 and 4 and 6 bytes per pixel -- a lane of the
// x16 form keeps its output columns and writes three 16-bit values where it wrote three bytes, so its destination base and stride are
// 2-byte aligned (an odd one takes the generic kernel); no table in LDS.
#include "k_tone_dev.h"
#include "k_scale_dev.h"

namespace mlv {

struct ScaleArgs {             // uniform in a launch
    uint32_t pw, ph, ow, oh;                          // W', H' and the output size
    uint32_t uo, nstrips, bo;                         // output columns of a strip, strips of a row, output rows of a band
    uint32_t row16;                                   // uint4s of a source row
    ScDiv dw, dh;                                     // / W', / H'
};

namespace {                    // this file's device helpers

constexpr int SC_NOUT = SC_STRIP / 256;               // output columns of a lane

// the three balanced channels of the superpixel in a dword of row 2Y (R low, G high) and the one below it (G low, B high)
__device__ __forceinline__ void balance3(uint32_t top, uint32_t bot, const Black &bl, const RenderParams &p, uint32_t n[3])
{
    n[0] = balance(bl(top & 0xFFFFu), p.A[0]);
    n[1] = balance(bl(((top >> 16) + (bot & 0xFFFFu) + 1u) >> 1), p.A[1]);
    n[2] = balance(bl(bot >> 16), p.A[2]);
}

template <Tone TN>
__device__ __forceinline__ void scale_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                          uint8_t *__restrict__ out, size_t out_stride, const ScaleArgs &a, uint8_t *lut,
                                          uint16_t (*planes)[3][SC_CHUNK], const LookArg &lk)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const bool k32 = fits32(p);                                                              // uniform: the matrix in 24-bit multiplies
    const uint4 *src = (const uint4 *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    const uint32_t band = blockIdx.x / a.nstrips, strip = blockIdx.x - band * a.nstrips;
    const uint32_t us0 = strip * a.uo, us1 = min(us0 + a.uo, a.ow);                          // the strip's output columns
    const uint32_t v0 = band * a.bo, v1 = min(v0 + a.bo, a.oh);                              // the band's output rows
    // the source columns the strip covers, from a multiple of 4 on, in chunks; the source rows the band covers.  Every product here is
    // at most ow W' or oh H', below 2^32
    const uint32_t xs0 = (us0 * a.pw / a.ow) & ~3u, xs1 = (us1 * a.pw - 1u) / a.ow + 1u;
    const uint32_t nchunks = (xs1 - xs0 + SC_CHUNK - 1) / SC_CHUNK;
    const uint32_t Y0 = v0 * a.ph / a.oh, Y1 = (v1 * a.ph - 1u) / a.oh + 1u;
    const uint32_t steps = (Y1 - Y0) * nchunks;
    // this lane's columns: u W' and the first and the last source column of each; a column outside the strip gets an empty span
    uint32_t lo[SC_NOUT], xlo[SC_NOUT], xhi[SC_NOUT];
#pragma unroll
    for (int i = 0; i < SC_NOUT; i++) {
        const uint32_t u = us0 + threadIdx.x + 256u * i;
        const bool mine = u < us1;
        lo[i] = mine ? u * a.pw : 0u;
        xlo[i] = mine ? lo[i] / a.ow : 1u;
        xhi[i] = mine ? (lo[i] + a.pw - 1u) / a.ow : 0u;
    }
    uint32_t hacc[SC_NOUT][3] = {}, vacc[SC_NOUT][3] = {};
    const uint32_t lane4 = threadIdx.x * 4u;
    uint4 top = make_uint4(0, 0, 0, 0), bot = top;
    if (xs0 + lane4 < xs1) {
        const uint4 *q = src + (size_t)Y0 * 2 * a.row16 + (xs0 + lane4) / 4;
        top = q[0];
        bot = q[a.row16];
    }
    uint32_t Y = Y0, k = 0, v = v0;
    for (uint32_t t = 0; t < steps; t++) {
        uint16_t (*pl)[SC_CHUNK] = planes[t & 1];
        const uint32_t cx0 = xs0 + k * SC_CHUNK, cx1 = min(cx0 + SC_CHUNK, xs1);
        if (cx0 + lane4 < xs1) {                                                          // W' % 4 == 0: all four or none
            uint32_t n0[3], n1[3], n2[3], n3[3];
            balance3(top.x, bot.x, bl, p, n0);
            balance3(top.y, bot.y, bl, p, n1);
            balance3(top.z, bot.z, bl, p, n2);
            balance3(top.w, bot.w, bl, p, n3);
#pragma unroll
            for (int j = 0; j < 3; j++) *(uint2 *)&pl[j][lane4] = make_uint2(n0[j] | (n1[j] << 16), n2[j] | (n3[j] << 16));
        }
        // the next step's loads
        uint32_t kn = k + 1, Yn = Y;
        if (kn == nchunks) { kn = 0; Yn++; }
        if (t + 1 < steps) {
            const uint32_t X = xs0 + kn * SC_CHUNK + lane4;
            if (X < xs1) {
                const uint4 *q = src + (size_t)Yn * 2 * a.row16 + X / 4;
                top = q[0];
                bot = q[a.row16];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SC_NOUT; i++) {
            const uint32_t xa = max(xlo[i], cx0), xb = min(xhi[i] + 1u, cx1), hi = lo[i] + a.pw;
            uint32_t e = xa * a.ow;                                                       // the source column's left edge
            for (uint32_t X = xa; X < xb; X++, e += a.ow) {
                const uint32_t w = min(e + a.ow, hi) - max(e, lo[i]);
                hacc[i][0] += __umul24(w, pl[0][X - cx0]);                                // both factors below 2^16: the full-rate multiply
                hacc[i][1] += __umul24(w, pl[1][X - cx0]);
                hacc[i][2] += __umul24(w, pl[2][X - cx0]);
            }
        }
        if (kn == 0) {                                                                    // the row is complete
            const uint32_t e = Y * a.oh, vlo = v * a.ph, vhi = vlo + a.ph;
            const uint32_t wy = min(e + a.oh, vhi) - max(e, vlo);
            const bool last = e + a.oh >= vhi;                                            // of output row v
            const uint32_t wnext = e + a.oh - min(e + a.oh, vhi);                         // what of the row belongs to v + 1
#pragma unroll
            for (int i = 0; i < SC_NOUT; i++) {
                const uint32_t u = us0 + threadIdx.x + 256u * i;
                if (u < us1) {
                    uint32_t hm[3];
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        hm[j] = sc_div(hacc[i][j] + (a.pw >> 1), a.dw);
                        hacc[i][j] = 0;
                        vacc[i][j] += __umul24(wy, hm[j]);
                    }
                    if (last) {
                        const uint32_t m0 = sc_div(vacc[i][0] + (a.ph >> 1), a.dh), m1 = sc_div(vacc[i][1] + (a.ph >> 1), a.dh);
                        const uint32_t m2 = sc_div(vacc[i][2] + (a.ph >> 1), a.dh);
                        const auto px = k32 ? tone<true, TN>(p, lut, lk, m0, m1, m2) : tone<false, TN>(p, lut, lk, m0, m1, m2);
                        if constexpr (TN == DEEP) {                                       // the same columns, stores twice as wide
                            uint16_t *o = (uint16_t *)(dst + ((size_t)v * a.ow + u) * 6);
                            o[0] = (uint16_t)px.x;
                            o[1] = (uint16_t)(px.x >> 16);
                            o[2] = (uint16_t)px.y;
                        } else {
                            put_pixel(dst + ((size_t)v * a.ow + u) * 3, px);
                        }
#pragma unroll
                        for (int j = 0; j < 3; j++) vacc[i][j] = __umul24(wnext, hm[j]);
                    }
                }
            }
            if (last) v++;
        }
        k = kn;
        Y = Yn;
    }
}

// npix = ow * oh output pixels per frame
template <Tone TN>
__device__ __forceinline__ void scale_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                              uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw, uint32_t ph,
                                              uint32_t ow, uint32_t oh, uint8_t *lut, const LookArg &lk, uint32_t first, uint32_t step)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const Black bl(p.black);
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    for (uint32_t k = first; k < npix; k += step) {
        const uint32_t v = k / ow, u = k - v * ow;
        const uint32_t ulo = u * pw, uhi = ulo + pw, vlo = v * ph, vhi = vlo + ph;
        const uint32_t xlo = ulo / ow, xhi = (uhi - 1u) / ow, ylo = vlo / oh, yhi = (vhi - 1u) / oh;
        uint32_t m[3] = { 0, 0, 0 };
        for (uint32_t Y = ylo; Y <= yhi; Y++) {
            const uint32_t wy = min((Y + 1u) * oh, vhi) - max(Y * oh, vlo);
            uint32_t s[3] = { 0, 0, 0 };
            for (uint32_t X = xlo; X <= xhi; X++) {
                const uint32_t wx = min((X + 1u) * ow, uhi) - max(X * ow, ulo);
                const uint16_t *q = src + (size_t)Y * 2 * w + (size_t)X * 2;
                s[0] += wx * balance(bl(q[0]), p.A[0]);
                s[1] += wx * balance(bl(((uint32_t)q[1] + q[w] + 1u) >> 1), p.A[1]);
                s[2] += wx * balance(bl(q[(size_t)w + 1]), p.A[2]);
            }
            for (int j = 0; j < 3; j++) m[j] += wy * ((s[j] + (pw >> 1)) / pw);
        }
        put_pixel(dst + (size_t)k * (TN == DEEP ? 6 : 3),
                  tone<false, TN>(p, lut, lk, (m[0] + (ph >> 1)) / ph, (m[1] + (ph >> 1)) / ph, (m[2] + (ph >> 1)) / ph));
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_scale_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                   uint8_t *__restrict__ out, size_t out_stride, const ScaleArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    __shared__ __attribute__((aligned(16))) uint16_t planes[2][3][SC_CHUNK];
    scale_x16<PLAIN>(frames, stride, params, out, out_stride, a, lut, planes, LookArg());
}

__global__ __launch_bounds__(256) void k_scale_look_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                        uint8_t *__restrict__ out, size_t out_stride, const ScaleArgs a, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    __shared__ __attribute__((aligned(16))) uint16_t planes[2][3][SC_CHUNK];
    scale_x16<LOOK>(frames, stride, params, out, out_stride, a, lut, planes, lk);
}

// the 16-bit form: the planes alone in LDS; the destination base and stride 2-byte aligned
__global__ __launch_bounds__(256) void k_scale_deep_x16(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                        uint8_t *__restrict__ out, size_t out_stride, const ScaleArgs a, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint16_t planes[2][3][SC_CHUNK];
    scale_x16<DEEP>(frames, stride, params, out, out_stride, a, nullptr, planes, lk);
}

__global__ __launch_bounds__(256) void k_scale_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                       uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw,
                                                       uint32_t ph, uint32_t ow, uint32_t oh)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    scale_generic<PLAIN>(frames, stride, params, out, out_stride, npix, w, pw, ph, ow, oh, lut, LookArg(), MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_scale_look_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                            uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw,
                                                            uint32_t ph, uint32_t ow, uint32_t oh, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    scale_generic<LOOK>(frames, stride, params, out, out_stride, npix, w, pw, ph, ow, oh, lut, lk, MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_scale_deep_generic(const uint8_t *__restrict__ frames, size_t stride, const RenderParams *__restrict__ params,
                                                            uint8_t *__restrict__ out, size_t out_stride, uint32_t npix, uint32_t w, uint32_t pw,
                                                            uint32_t ph, uint32_t ow, uint32_t oh, const LookArg lk)
{
    scale_generic<DEEP>(frames, stride, params, out, out_stride, npix, w, pw, ph, ow, oh, nullptr, lk, MLV_GRID_STRIDE);
}

// d_out apart from d_frames (the callers check); d_params: 13 int32 per frame, 4-byte aligned
int launch_render_scaled(const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h, int ow,
                         int oh, int nframes, hipStream_t stream, const LookArg *lk, bool deep)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    int pw, ph;
    if (!scale_geom(w, h, ow, oh, &pw, &ph)) return route_refuse("launch_render_scaled", { RenderRoute::SCALED, false, ow, oh }, w, h);
    const bool fast = w % 16 == 0 && ((uintptr_t)d_frames % 16 == 0) && (nframes == 1 || stride % 16 == 0) &&
                      (!deep || ((uintptr_t)d_out % 2 == 0 && (nframes == 1 || out_stride % 2 == 0)));      // 16-bit stores
    if (fast) {
        const ScalePlan pl = scale_plan(pw, ph, ow, oh, nframes);
        const ScaleArgs a{ (uint32_t)pw, (uint32_t)ph, (uint32_t)ow, (uint32_t)oh, pl.uo, pl.nstrips, pl.bo, (uint32_t)w / 8,
                           scdiv_make((uint32_t)pw), scdiv_make((uint32_t)ph) };
        launch_tone(k_scale_deep_x16, k_scale_look_x16, k_scale_x16, dim3(pl.nstrips * pl.nbands, nframes), stream, lk, deep, (const uint8_t *)d_frames,
                    stride, (const RenderParams *)d_params, (uint8_t *)d_out, out_stride, a);
    } else {
        const uint32_t npix = (uint32_t)ow * (uint32_t)oh, cap = std::max(2048u / (uint32_t)nframes, 64u);
        const dim3 grid(std::min<uint32_t>((npix + 255) / 256, 4 * cap), nframes);
        launch_tone(k_scale_deep_generic, k_scale_look_generic, k_scale_generic, grid, stream, lk, deep, (const uint8_t *)d_frames, stride,
                    (const RenderParams *)d_params, (uint8_t *)d_out, out_stride, npix, (uint32_t)w, (uint32_t)pw, (uint32_t)ph, (uint32_t)ow, (uint32_t)oh);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

// k_amaze_resample.hip -- resampled rendered frames with AMaZE as the demosaic (include/mlvfs_amd.h, "resampled rendered frames demosaiced
// by AMaZE"): the one pass behind amaze_launch that turns a batch's three float planes into the ow x oh renderings.
//     n_c(y, x)  = (int)(clampf(v_c) + 0.5f), clampf(v) = 0 for NaN and v <= 0, 65535 for v >= 65535, else v      (3.19's step 3)
//     wx(u, x)   = max(0, min((x + 1) ow, (u + 1) W) - max(x ow, u W))             wy(v, y) likewise with H, oh
//     hd_c(y, u) = floor((sum_x wx(u, x) n_c(y, x) + (W >> 1)) / W)                32 bits unsigned hold every sum (W, H <= 65535)
//     m_c(v, u)  = floor((sum_y wy(v, y) hd_c(y, u) + (H >> 1)) / H)
//     then steps 3 and 4 of the rendered routes from k_tone_dev.h on m: the sRGB table in LDS, a look, or a deep look
// black, A[3], K[9]: the renderings' 13 int32 per frame (mlvfs_amd_rgb_params), uniform in a workgroup; this pass reads K alone.
// Frames are batched in grid.y; frame k's plane lies k * plane_stride floats behind the batch's plane pointer.  Never in place, no scratch.
//   k_amz_resample_x16<FORM>     : W % 8 == 0, 2 ow >= W, plane bases and stride 16-byte aligned (a row starts on a 16-byte boundary then,
//                        W being a multiple of 4), in the deep form a 2-byte aligned destination base and stride.  k_resample_x16 with its
//                        first half taken out: a workgroup of four waves owns a strip of `uo` output columns (at most AZ_NOUT per lane)
//                        and a band of `bo` output rows (resample_plan, clip.h) and walks the band's source rows AZ_ROWS a step, one per
//                        wave.  A lane loads 8 pixels of each plane as two 128-bit loads -- the row of the next step while this one is
//                        averaged --, runs step 3 once per sample and stores the three channels as 16-bit words into the step's planes
//                        in LDS, one 128-bit store per plane.  Behind a barrier a lane takes the step's rows top down: three products
//                        per column and channel, sc_div by W, wy hd added to the column's sum; with the last source row of an output
//                        row sc_div by H, matrix, tone and stores.  No ring, no halo: a source row that straddles two bands is read by
//                        both.  The averaging lines are k_resample_x16's, stated here once more and not shared with it, so that its
//                        kernels compile to what they were.
//   k_amz_resample_generic<FORM> : any geometry the route takes, 4-byte plane alignment, any destination; one lane = one output pixel, its
//                        footprint read straight from the planes with step 3 on every sample, both divisions with the plain operator,
//                        the 64-bit matrix.
// Bytes between renderings and behind 3 (6) ow oh are never touched.
#include "k_tone_dev.h"
#include "k_scale_dev.h"

namespace mlv {

struct AmzResampleArgs {       // uniform in a launch
    uint32_t w, h, ow, oh;
    uint32_t uo, nstrips, bo;                         // output columns of a strip, strips of a row, output rows of a band
    ScDiv dw, dh;                                     // / W, / H
};

namespace {                    // this file's device helpers

constexpr int AZ_STRIP = RS_STRIP;                    // source columns of a strip at most: 64 lanes x 8 pixels
constexpr int AZ_ROWS = RS_ROWS;                      // source rows of a step: one per wave
constexpr int AZ_NOUT = 2;                            // output columns of a lane: uo <= AZ_STRIP - 16
constexpr int AZ_PITCH = AZ_STRIP + 8;                // uint16 per plane: a span may name two columns behind its first
static_assert(AZ_ROWS == 4 && AZ_STRIP == 512, "a step is one row per wave, a row 8 pixels per lane");

// 3.19's step 3 (k_amaze_render.hip's sample16): NaN fails the compare and gives 0; the sum is the definition's binary32 sum
__device__ __forceinline__ uint32_t sample16(float v)
{
    const float c = v > 0.0f ? fminf(v, 65535.0f) : 0.0f;
    return (uint32_t)(c + 0.5f);
}

struct PlaneRow {              // a lane's 8 pixels of the three planes
    float4 v[3][2];
};

// row y of the strip, where the band has it (y < y1) and the lane lies in the strip; at: the planes at the frame, x0: the strip's first column
__device__ __forceinline__ void load_planes(PlaneRow &ld, const float *r, const float *g, const float *b, int w, int y, int y1, int x0, int sw, int lane)
{
    if (y < y1 && 8 * lane < sw) {
        const size_t at = (size_t)y * w + x0 + 8 * lane;
        ld.v[0][0] = ((const float4 *)(r + at))[0]; ld.v[0][1] = ((const float4 *)(r + at))[1];
        ld.v[1][0] = ((const float4 *)(g + at))[0]; ld.v[1][1] = ((const float4 *)(g + at))[1];
        ld.v[2][0] = ((const float4 *)(b + at))[0]; ld.v[2][1] = ((const float4 *)(b + at))[1];
    }
}

// step 3 on the lane's samples; pl: the R plane of the wave's row at the lane's first pixel
__device__ __forceinline__ void store_planes(const PlaneRow &ld, uint16_t *pl)
{
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const float4 a = ld.v[j][0], c = ld.v[j][1];
        *(uint4 *)(pl + j * AZ_PITCH) = make_uint4(sample16(a.x) | (sample16(a.y) << 16), sample16(a.z) | (sample16(a.w) << 16),
                                                   sample16(c.x) | (sample16(c.y) << 16), sample16(c.z) | (sample16(c.w) << 16));
    }
}

// grid.x = strips * bands, strips side by side first
template <Tone TN>
__device__ __forceinline__ void amz_resample_x16(const float *__restrict__ red, const float *__restrict__ green, const float *__restrict__ blue,
                                                 size_t plane_stride, const RenderParams *__restrict__ params, uint8_t *__restrict__ out,
                                                 size_t out_stride, const AmzResampleArgs &a, uint8_t *lut, uint16_t (*planes)[3][AZ_PITCH],
                                                 const LookArg &lk)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const bool k32 = fits32(p);                                                              // uniform: the matrix in 24-bit multiplies
    const size_t at = (size_t)blockIdx.y * plane_stride;
    const float *r = red + at, *g = green + at, *b = blue + at;
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    const int w = (int)a.w;
    const uint32_t band = blockIdx.x / a.nstrips, strip = blockIdx.x - band * a.nstrips;
    const uint32_t us0 = strip * a.uo, us1 = min(us0 + a.uo, a.ow);                          // the strip's output columns
    const uint32_t v0 = band * a.bo, v1 = min(v0 + a.bo, a.oh);                              // the band's output rows
    // the source columns the strip covers, from a multiple of 8 to a multiple of 8 (W % 8 == 0: inside the frame), and the source rows
    // the band covers (y1 <= H).  Every product here is at most ow W or oh H, below 2^32
    const uint32_t xs1 = (us1 * a.w - 1u) / a.ow + 1u;
    const int x0 = (int)((us0 * a.w / a.ow) & ~7u), sw = min((int)((xs1 + 7u) & ~7u) - x0, AZ_STRIP);
    const int y0 = (int)(v0 * a.h / a.oh), y1 = min((int)((v1 * a.h - 1u) / a.oh) + 1, (int)a.h);
    // this lane's columns: where the span begins in the planes, and its three weights (they sum to W); a column outside the strip has none
    uint32_t xi[AZ_NOUT], wa[AZ_NOUT], wb[AZ_NOUT], wc[AZ_NOUT];
#pragma unroll
    for (int i = 0; i < AZ_NOUT; i++) {
        const uint32_t u = us0 + threadIdx.x + 256u * i;
        const bool mine = u < us1;
        const uint32_t lo = mine ? u * a.w : 0u, hi = lo + a.w, xl = lo / a.ow, e1 = min((xl + 1u) * a.ow, hi), e2 = min((xl + 2u) * a.ow, hi);
        xi[i] = mine ? min(xl - (uint32_t)x0, (uint32_t)AZ_STRIP - 1u) : 0u;                     // the plan keeps it below sw: a bound for the read
        wa[i] = mine ? e1 - lo : 0u;
        wb[i] = mine ? e2 - e1 : 0u;
        wc[i] = mine ? hi - e2 : 0u;
    }
    uint32_t vacc[AZ_NOUT][3] = {};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    PlaneRow ld = {};
    load_planes(ld, r, g, b, w, y0 + wave, y1, x0, sw, lane);
    uint32_t v = v0;
    for (int yb = y0; yb < y1; yb += AZ_ROWS) {                                              // uniform: every wave meets every barrier
        const int y = yb + wave;
        if (y < y1 && 8 * lane < sw) store_planes(ld, &planes[wave][0][8 * lane]);
        load_planes(ld, r, g, b, w, y + AZ_ROWS, y1, x0, sw, lane);                          // in flight while this step is averaged
        __syncthreads();
        // the step's rows top down
        for (int rr = 0; rr < AZ_ROWS && yb + rr < y1 && v < v1; rr++) {                     // v < v1 holds by construction: a bound for the stores
            const uint32_t e = (uint32_t)(yb + rr) * a.oh, vlo = v * a.h, vhi = vlo + a.h;
            const uint32_t wy = min(e + a.oh, vhi) - max(e, vlo);
            const bool last = e + a.oh >= vhi;                                               // of output row v
            const uint32_t wnext = e + a.oh - min(e + a.oh, vhi);                            // what of the row belongs to v + 1
#pragma unroll
            for (int i = 0; i < AZ_NOUT; i++) {
                const uint32_t u = us0 + threadIdx.x + 256u * i;
                if (u < us1) {
                    uint32_t hd[3];
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const uint16_t *q = &planes[rr][j][xi[i]];
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

// npix = ow * oh output pixels per frame
template <Tone TN>
__device__ __forceinline__ void amz_resample_generic(const float *__restrict__ red, const float *__restrict__ green, const float *__restrict__ blue,
                                                     size_t plane_stride, const RenderParams *__restrict__ params, uint8_t *__restrict__ out,
                                                     size_t out_stride, uint32_t npix, uint32_t uw, uint32_t uh, uint32_t ow, uint32_t oh,
                                                     uint8_t *lut, const LookArg &lk, uint32_t first, uint32_t step)
{
    stage_lut<TN>(lut, lk);
    const RenderParams p = params[blockIdx.y];
    const size_t at = (size_t)blockIdx.y * plane_stride;
    const float *pl[3] = { red + at, green + at, blue + at };
    uint8_t *dst = out + (size_t)blockIdx.y * out_stride;
    for (uint32_t k = first; k < npix; k += step) {
        const uint32_t v = k / ow, u = k - v * ow;
        const uint32_t ulo = u * uw, uhi = ulo + uw, vlo = v * uh, vhi = vlo + uh;
        const uint32_t xlo = ulo / ow, xhi = (uhi - 1u) / ow, ylo = vlo / oh, yhi = (vhi - 1u) / oh;       // xhi < W, yhi < H
        uint32_t m[3] = { 0, 0, 0 };
        for (uint32_t yy = ylo; yy <= yhi; yy++) {
            const uint32_t wy = min((yy + 1u) * oh, vhi) - max(yy * oh, vlo);
            uint32_t s[3] = { 0, 0, 0 };
            for (uint32_t xx = xlo; xx <= xhi; xx++) {
                const uint32_t wx = min((xx + 1u) * ow, uhi) - max(xx * ow, ulo);
                const size_t q = (size_t)yy * uw + xx;
#pragma unroll
                for (int j = 0; j < 3; j++) s[j] += wx * sample16(pl[j][q]);
            }
#pragma unroll
            for (int j = 0; j < 3; j++) m[j] += wy * ((s[j] + (uw >> 1)) / uw);
        }
        put_pixel(dst + (size_t)k * (TN == DEEP ? 6 : 3),
                  tone<false, TN>(p, lut, lk, (m[0] + (uh >> 1)) / uh, (m[1] + (uh >> 1)) / uh, (m[2] + (uh >> 1)) / uh));
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_amz_resample_x16(const float *__restrict__ red, const float *__restrict__ green, const float *__restrict__ blue,
                                                          size_t plane_stride, const RenderParams *__restrict__ params, uint8_t *__restrict__ out,
                                                          size_t out_stride, const AmzResampleArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    __shared__ __attribute__((aligned(16))) uint16_t planes[AZ_ROWS][3][AZ_PITCH];
    amz_resample_x16<PLAIN>(red, green, blue, plane_stride, params, out, out_stride, a, lut, planes, LookArg());
}

__global__ __launch_bounds__(256) void k_amz_resample_look_x16(const float *__restrict__ red, const float *__restrict__ green,
                                                               const float *__restrict__ blue, size_t plane_stride,
                                                               const RenderParams *__restrict__ params, uint8_t *__restrict__ out, size_t out_stride,
                                                               const AmzResampleArgs a, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    __shared__ __attribute__((aligned(16))) uint16_t planes[AZ_ROWS][3][AZ_PITCH];
    amz_resample_x16<LOOK>(red, green, blue, plane_stride, params, out, out_stride, a, lut, planes, lk);
}

// the 16-bit form: the planes alone in LDS; the destination base and stride 2-byte aligned
__global__ __launch_bounds__(256) void k_amz_resample_deep_x16(const float *__restrict__ red, const float *__restrict__ green,
                                                               const float *__restrict__ blue, size_t plane_stride,
                                                               const RenderParams *__restrict__ params, uint8_t *__restrict__ out, size_t out_stride,
                                                               const AmzResampleArgs a, const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint16_t planes[AZ_ROWS][3][AZ_PITCH];
    amz_resample_x16<DEEP>(red, green, blue, plane_stride, params, out, out_stride, a, nullptr, planes, lk);
}

__global__ __launch_bounds__(256) void k_amz_resample_generic(const float *__restrict__ red, const float *__restrict__ green,
                                                              const float *__restrict__ blue, size_t plane_stride,
                                                              const RenderParams *__restrict__ params, uint8_t *__restrict__ out, size_t out_stride,
                                                              uint32_t npix, uint32_t w, uint32_t h, uint32_t ow, uint32_t oh)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<PLAIN>];
    amz_resample_generic<PLAIN>(red, green, blue, plane_stride, params, out, out_stride, npix, w, h, ow, oh, lut, LookArg(), MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_amz_resample_look_generic(const float *__restrict__ red, const float *__restrict__ green,
                                                                   const float *__restrict__ blue, size_t plane_stride,
                                                                   const RenderParams *__restrict__ params, uint8_t *__restrict__ out,
                                                                   size_t out_stride, uint32_t npix, uint32_t w, uint32_t h, uint32_t ow, uint32_t oh,
                                                                   const LookArg lk)
{
    __shared__ __attribute__((aligned(16))) uint8_t lut[TONE_LDS<LOOK>];
    amz_resample_generic<LOOK>(red, green, blue, plane_stride, params, out, out_stride, npix, w, h, ow, oh, lut, lk, MLV_GRID_STRIDE);
}

__global__ __launch_bounds__(256) void k_amz_resample_deep_generic(const float *__restrict__ red, const float *__restrict__ green,
                                                                   const float *__restrict__ blue, size_t plane_stride,
                                                                   const RenderParams *__restrict__ params, uint8_t *__restrict__ out,
                                                                   size_t out_stride, uint32_t npix, uint32_t w, uint32_t h, uint32_t ow, uint32_t oh,
                                                                   const LookArg lk)
{
    amz_resample_generic<DEEP>(red, green, blue, plane_stride, params, out, out_stride, npix, w, h, ow, oh, nullptr, lk, MLV_GRID_STRIDE);
}

// the callers check: amz_resample_geom(w, h, ow, oh), the destination apart from the planes and the parameters; d_params: 13 int32 per
// frame.  lk: the look, or with deep the deep look; null: the sRGB table
int launch_amz_resample(const float *d_red, const float *d_green, const float *d_blue, size_t plane_stride, const int32_t *d_params, void *d_out,
                        size_t out_stride, int w, int h, int ow, int oh, int nframes, hipStream_t stream, const LookArg *lk, bool deep)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (!amz_resample_geom(w, h, ow, oh)) return route_refuse("launch_amz_resample", { RenderRoute::RESAMPLED, true, ow, oh }, w, h);
    const bool fast = amz_resample_fast_geom(w, ow) && (((uintptr_t)d_red | (uintptr_t)d_green | (uintptr_t)d_blue) % 16 == 0) &&
                      (nframes == 1 || plane_stride % 4 == 0) &&
                      (!deep || ((uintptr_t)d_out % 2 == 0 && (nframes == 1 || out_stride % 2 == 0)));      // 16-bit stores
    const RenderParams *par = (const RenderParams *)d_params;
    uint8_t *out = (uint8_t *)d_out;
    if (fast) {
        const ResamplePlan pl = resample_plan(w, h, ow, oh, nframes);
        const AmzResampleArgs a{ (uint32_t)w, (uint32_t)h, (uint32_t)ow, (uint32_t)oh, pl.uo, pl.nstrips, pl.bo, scdiv_make((uint32_t)w), scdiv_make((uint32_t)h) };
        const dim3 grid(pl.nstrips * pl.nbands, nframes);
        launch_tone(k_amz_resample_deep_x16, k_amz_resample_look_x16, k_amz_resample_x16, grid, stream, lk, deep, d_red, d_green, d_blue, plane_stride,
                    par, out, out_stride, a);
    } else {
        const uint32_t npix = (uint32_t)ow * (uint32_t)oh, cap = std::max(2048u / (uint32_t)nframes, 64u);
        const dim3 grid(std::min<uint32_t>((npix + 255) / 256, 4 * cap), nframes);
        const uint32_t uw = (uint32_t)w, uh = (uint32_t)h, uow = (uint32_t)ow, uoh = (uint32_t)oh;
        launch_tone(k_amz_resample_deep_generic, k_amz_resample_look_generic, k_amz_resample_generic, grid, stream, lk, deep, d_red, d_green, d_blue,
                    plane_stride, par, out, out_stride, npix, uw, uh, uow, uoh);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

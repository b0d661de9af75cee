// render_route.h -- the rendering routes, each described once: which frames a route takes and what size comes out (route_geom), the
// words of its limits (route_refuse), and its launcher (route_launch, the only caller of the six launch_render* functions).  The
// leaves are here too: the geometry predicates, the plans of the scaled and the resampled kernels, the look argument and the
// launcher prototypes that the host files and the kernel files share.  render_route.cpp holds the device entry points
// (mlvfs_amd_render*_dev) with their one checked body, the exported geometry and fit calls and the plan test hooks.
#pragma once

#include "common.h"

#include <algorithm>

namespace mlv {

struct ThreadCtx;

// mlvfs_amd_rgb_params' int32 per frame: black, A[3], K[9] (k_tone_dev.h's RenderParams)
constexpr int RGB_PARAMS = 13;

// rendered half-size sRGB frames (k_render.hip): W' x H' of a w x h frame, false below 2x2 and from 2^27 pixels on; the developing pass
// (d_params: mlvfs_amd_rgb_params' RGB_PARAMS int32 per frame)
inline bool rgb_geom(int w, int h, int *pw, int *ph)
{
    if (w < 2 || h < 2 || (uint64_t)w * (uint64_t)h >= (1u << 27)) return false;
    *pw = w / 2;
    *ph = h / 2;
    return true;
}
// a look for the rendered frames (look.cpp; k_tone_dev.h): the device image mlvfs_amd_look_pack writes -- the shaper's 4096 uint16, then
// n^3 entries of 8 bytes (R, G, B, 0 as uint16), red fastest -- as the look kernels take it; lk == nullptr below: the plain kernels
constexpr size_t LOOK_SHAPER_BYTES = 4096 * sizeof(uint16_t);
// a deep look for the 16-bit routes (look.cpp; k_tone_dev.h): S16's 65536 uint16, then the same entries; n == 0: no table.  The deep
// kernels take it as a LookArg too (deep == true below, with lk set)
constexpr size_t LOOK16_SHAPER_BYTES = 65536 * sizeof(uint16_t);
struct LookArg {
    const uint8_t *image = nullptr;
    uint32_t n = 0;
};
// the handle's image on c's device (MLVFS_AMD_ERR_ARG, with the error set: the handle was created on another device)
int look_on_device(const mlvfs_amd_look_t *look, ThreadCtx *c, LookArg *out);
// n triples of 12-bit indices (masked) -> n triples of bytes through step 4 with the look (k_render.hip)
int launch_look_apply(const LookArg &lk, const uint16_t *d_t, size_t n, uint8_t *d_out, hipStream_t stream);
int look16_on_device(const mlvfs_amd_look16_t *look, ThreadCtx *c, LookArg *out);
// n triples of 16-bit indices -> n triples of 16-bit samples through step 4 of the 16-bit routes (k_render.hip)
int launch_look16_apply(const LookArg &lk, const uint16_t *d_t, size_t n, uint16_t *d_out, hipStream_t stream);
int launch_render2(const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h, int nframes,
                   hipStream_t stream, const LookArg *lk = nullptr, bool deep = false);
// rendered full-size sRGB frames (k_demosaic.hip): W x H pixels of a w x h frame, false below 4x4 and from 2^25 pixels on (what
// mlvfs_amd_rgb_header writes); the demosaicing pass, with the same parameters
inline bool rgb_full_geom(int w, int h) { return w >= 4 && h >= 4 && (uint64_t)w * (uint64_t)h < (1u << 25); }
int launch_render1(const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h, int nframes,
                   hipStream_t stream, const LookArg *lk = nullptr, bool deep = false);
// rendered full-size frames demosaiced by AMaZE (k_amaze_render.hip, amaze_render.cpp): the frames AMaZE takes -- a width that is a
// multiple of 4, 36 x 36 and more -- below 2^25 pixels; the two element-wise passes around amaze_launch; the three passes for a batch,
// in sub-batches that fit the calling thread's work memory (lk, deep: launch_render1's)
inline bool rgb_amaze_geom(int w, int h) { return (w & 3) == 0 && w >= 36 && h >= 36 && (uint64_t)w * (uint64_t)h < (1u << 25); }
int launch_amz_balance(const void *d_frames, size_t stride, const int32_t *d_params, float *d_planes, size_t plane_stride, int w, int h,
                       int nframes, hipStream_t stream);
int launch_amz_tone(const float *d_red, const float *d_green, const float *d_blue, size_t plane_stride, const int32_t *d_params, void *d_out,
                    size_t out_stride, int w, int h, int nframes, hipStream_t stream, const LookArg *lk = nullptr, bool deep = false);
int launch_render1_amaze(ThreadCtx *c, const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h,
                         int nframes, hipStream_t stream, const LookArg *lk = nullptr, bool deep = false);
// rendered frames at any smaller size (k_scale.hip): W' x H' of a w x h frame as rgb_geom gives them, false where a side of that grid
// exceeds 65535 or ow x oh is not 1x1 up to W' x H'; the scaling pass, with the same parameters
inline bool scale_geom(int w, int h, int ow, int oh, int *pw, int *ph)
{
    return rgb_geom(w, h, pw, ph) && *pw <= 65535 && *ph <= 65535 && ow >= 1 && ow <= *pw && oh >= 1 && oh <= *ph;
}
// floor(n / d) = (t + ((n - t) >> s1)) >> s2 with t = the high 32 bits of n m, for every n below 2^32 and any d >= 1: division by an
// invariant with a 33-bit multiplier, rounded up (Granlund and Montgomery, PLDI 1994, figure 4.1), l = ceil(log2 d)
struct ScDiv {
    uint32_t m, s1, s2;
};
inline ScDiv scdiv_make(uint32_t d)
{
    uint32_t l = 0;
    while ((1ull << l) < d) l++;
    return { (uint32_t)((((1ull << l) - d) << 32) / d + 1), l ? 1u : 0u, l ? l - 1 : 0u };
}
inline uint32_t scdiv_host(uint32_t n, const ScDiv &d)
{
    const uint32_t t = (uint32_t)(((uint64_t)n * d.m) >> 32);
    return (t + ((n - t) >> d.s1)) >> d.s2;
}
// how k_scale_x16 divides a frame among workgroups: strips of uo output columns, bands of bo output rows
constexpr int SC_CHUNK = 1024;                        // superpixels of a source row a step stages: 256 lanes x 4
constexpr int SC_STRIP = 1024;                        // most output columns of a strip: 256 lanes x 4
constexpr int SC_BAND_ROWS = 8;                       // source rows a band covers at least: a seam costs one row read twice
struct ScalePlan {
    uint32_t uo, nstrips, bo, nbands;
};
inline ScalePlan scale_plan(int pw, int ph, int ow, int oh, int nframes)
{
    ScalePlan p;
    // a strip's source columns, floor(us0 W' / ow) rounded down to 4 up to ceil(us1 W' / ow), fit one chunk where one column's do
    p.uo = (uint32_t)((uint64_t)(SC_CHUNK - 8) * ow / pw);
    p.uo = std::min(std::min(std::max(p.uo, 1u), (uint32_t)SC_STRIP), (uint32_t)ow);
    p.nstrips = ((uint32_t)ow + p.uo - 1) / p.uo;
    // as many workgroups in a launch as the machine holds at once (256 CUs x 4 of them at 4 waves per SIMD): a launch of a few more
    // would run the last of them alone; and bands that are not all seam
    const uint32_t budget = std::max(1024u / (uint32_t)std::max(nframes, 1), 32u);
    const uint32_t nb = std::min(std::max(budget / p.nstrips, 1u), (uint32_t)oh);
    const uint32_t least = (uint32_t)(((uint64_t)SC_BAND_ROWS * oh + ph - 1) / ph);
    p.bo = std::min(std::max(((uint32_t)oh + nb - 1) / nb, least), (uint32_t)oh);
    p.nbands = ((uint32_t)oh + p.bo - 1) / p.bo;
    return p;
}
int launch_render_scaled(const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h, int ow,
                         int oh, int nframes, hipStream_t stream, const LookArg *lk = nullptr, bool deep = false);
// rendered frames resampled from the full-size rendering (k_resample.hip): the full-size rendering's frames with both sides up to
// 65535, and ow x oh from 1x1 up to the frame's own size; the resampling pass, with the same parameters
inline bool resample_geom(int w, int h, int ow, int oh)
{
    return rgb_full_geom(w, h) && w <= 65535 && h <= 65535 && ow >= 1 && ow <= w && oh >= 1 && oh <= h;
}
// what k_resample_x16 asks of the sizes: whole 16-pixel groups, and output columns that span at most three source pixels
inline bool resample_fast_geom(int w, int ow) { return w % 16 == 0 && 2 * (int64_t)ow >= w; }
// how k_resample_x16 divides a frame among workgroups: strips of uo output columns whose source columns, from a multiple of 8 to a
// multiple of 8, fit the RS_STRIP columns of the ring (k_demosaic_dev.h), and bands of bo output rows
constexpr int RS_STRIP = 512;                         // source columns a workgroup demosaics at most
constexpr int RS_ROWS = 4;                            // source rows a step demosaics: one per wave
constexpr int RS_BAND_ROWS = 32;                      // source rows a band covers at least: a seam costs five rows balanced twice
struct ResamplePlan {
    uint32_t uo, nstrips, bo, nbands;
};
inline ResamplePlan resample_plan(int w, int h, int ow, int oh, int nframes)
{
    ResamplePlan p;
    // uo output columns cover at most ceil(uo w / ow) + 1 source columns, and the rounding to 8 adds at most 7 at each side
    p.uo = (uint32_t)((uint64_t)(RS_STRIP - 16) * ow / w);
    // a lane takes the columns l and l + 256 of its strip: a strip of a few more than 256 would make one wave walk twice for them
    // while the others wait, so a strip is 256 columns unless it fills at least half of the second round
    if (p.uo > 256 && p.uo < 384) p.uo = 256;
    p.uo = std::min(std::max(p.uo, 1u), (uint32_t)ow);
    p.nstrips = ((uint32_t)ow + p.uo - 1) / p.uo;
    // as many workgroups in a launch as the machine holds at once (256 CUs x 4 of them by their LDS), and bands that are not all seam
    const uint32_t budget = std::max(1024u / (uint32_t)std::max(nframes, 1), 32u);
    const uint32_t nb = std::min(std::max(budget / p.nstrips, 1u), (uint32_t)oh);
    const uint32_t least = (uint32_t)(((uint64_t)RS_BAND_ROWS * oh + h - 1) / h);
    p.bo = std::min(std::max(((uint32_t)oh + nb - 1) / nb, least), (uint32_t)oh);
    p.nbands = ((uint32_t)oh + p.bo - 1) / p.bo;
    return p;
}
int launch_render_resampled(const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h, int ow,
                            int oh, int nframes, hipStream_t stream, const LookArg *lk = nullptr, bool deep = false);
// resampled rendered frames demosaiced by AMaZE (k_amaze_resample.hip, amaze_render.cpp): the frames the AMaZE rendering takes with
// both sides up to 65535, and ow x oh from 1x1 up to the frame's own size; the pass behind amaze_launch; balance, AMaZE and that pass
// for a batch, in launch_render1_amaze's work memory and sub-batches
inline bool amz_resample_geom(int w, int h, int ow, int oh)
{
    return rgb_amaze_geom(w, h) && w <= 65535 && h <= 65535 && ow >= 1 && ow <= w && oh >= 1 && oh <= h;
}
// what k_amz_resample_x16 asks of the sizes: whole 8-pixel groups, and output columns that span at most three source pixels.  It
// divides a frame among workgroups as k_resample_x16 does (resample_plan), which asks no more of the width than that
inline bool amz_resample_fast_geom(int w, int ow) { return w % 8 == 0 && 2 * (int64_t)ow >= w; }
int launch_amz_resample(const float *d_red, const float *d_green, const float *d_blue, size_t plane_stride, const int32_t *d_params, void *d_out,
                        size_t out_stride, int w, int h, int ow, int oh, int nframes, hipStream_t stream, const LookArg *lk = nullptr,
                        bool deep = false);
int launch_render_resampled_amaze(ThreadCtx *c, const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w,
                                  int h, int ow, int oh, int nframes, hipStream_t stream, const LookArg *lk = nullptr, bool deep = false);

// ---- a route: the size of the rendering -- half the frame's, the frame's own, ow x oh area-averaged from the half-size grid, or ow x oh
// area-averaged from the full-size rendering -- and, for the two that demosaic, whether AMaZE does it
struct RenderRoute {
    enum Size { HALF, FULL, SCALED, RESAMPLED } size = HALF;
    bool amaze = false;
    int ow = 0, oh = 0;                               // SCALED, RESAMPLED
    bool sized() const { return size == SCALED || size == RESAMPLED; }
};
// whether the route takes w x h (to ow x oh); if so *pw x *ph is what comes out, otherwise neither is written
bool route_geom(const RenderRoute &r, int w, int h, int *pw, int *ph);
// the refusal of a shape route_geom does not take: the error set to the route's limits in the name of `who` ("render2", "mount"),
// MLVFS_AMD_ERR_ARG returned
int route_refuse(const char *who, const RenderRoute &r, int w, int h);
// the route's launcher; c: the calling thread's context (AMaZE's work memory is per thread); lk == nullptr: the plain kernels
int route_launch(const RenderRoute &r, ThreadCtx *c, const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride,
                 int w, int h, int nframes, hipStream_t stream, const LookArg *lk, bool deep);

}  // namespace mlv

// amaze_render.cpp -- rendered full-size frames with AMaZE as the demosaic (include/mlvfs_amd.h, "rendered full-size frames demosaiced
// by AMaZE"): the geometry, the work memory and its sub-batches, the three passes of a batch (k_amaze_render.hip's balance,
// amaze_launch of k_amaze.hip / k_amaze_rows.hip as it is, k_amaze_render.hip's tone) and the entry points of the passes alone: the
// balance, and the last pass from three float planes.  The resampled form ("resampled rendered frames demosaiced by AMaZE")
// is the same loop with k_amaze_resample.hip's pass in the place of the tone pass.  The two routes' own entry points, with every other
// route's, are in render_route.cpp.
//
// Work memory, per (host thread, device), grown on demand: four float planes per frame of a sub-batch (raw, red, green, blue, each kind
// as one batch of planes plane_stride floats apart) and AMaZE's tile planes, amaze_scratch_bytes per frame.  The tile planes are this
// route's own buffer -- no dual-ISO conversion, mlvfs_amd_amaze_demosaic_dev call or debug call ever reads or writes it, and this route
// never touches theirs -- and they are zeroed whenever the buffer is (re)allocated or the geometry it last served changes: AMaZE relies
// on planes that read as zero where a tile never writes, and for one geometry every tile rewrites exactly what it wrote before.
#include "clip.h"
#include "dualiso.h"
#include "render_route.h"

#include <algorithm>
#include <map>

namespace mlv {

namespace {

constexpr size_t AMZ_WORK_CAP = (size_t)6 << 30;          // most work memory a call reserves by itself: 8 frames of 3584 x 1320

struct AmzPlan {
    size_t plane_stride;       // floats from one frame's plane to the next, a multiple of 64
    size_t tile_stride;        // floats of one frame's tile planes
    size_t frame_bytes;        // four planes and the tile planes
    int sub;                   // frames of a sub-batch
};

AmzPlan amz_plan(int w, int h, int nframes, size_t cap)
{
    AmzPlan p;
    p.plane_stride = ((size_t)w * h + 63) / 64 * 64;
    p.tile_stride = amaze_tiles(w, h) * AMAZE_TILE_FLOATS;
    p.frame_bytes = (4 * p.plane_stride + p.tile_stride) * sizeof(float);
    p.sub = (int)std::min<size_t>(std::max<size_t>(cap / p.frame_bytes, 1), (size_t)std::max(nframes, 1));
    return p;
}

struct AmzWork {
    DevBuf planes, tiles;
    const void *zeroed = nullptr;      // the block of `tiles` that was zeroed, its size and the geometry it has served since
    size_t zeroed_bytes = 0;
    int w = 0, h = 0;
};
thread_local std::map<int, AmzWork> t_amz;

// room for `sub` frames; the tile planes zeroed where they have to be
int amz_reserve(AmzWork &wk, const AmzPlan &p, int sub, int w, int h, hipStream_t s)
{
    if (const int rc = wk.planes.reserve(4 * p.plane_stride * sizeof(float) * sub)) return rc;
    if (const int rc = wk.tiles.reserve(p.tile_stride * sizeof(float) * sub)) return rc;
    if (wk.zeroed != wk.tiles.p || wk.zeroed_bytes != wk.tiles.bytes || wk.w != w || wk.h != h) {
        MLV_HIP(hipMemsetAsync(wk.tiles, 0, wk.tiles.bytes, s));
        wk.zeroed = wk.tiles.p; wk.zeroed_bytes = wk.tiles.bytes; wk.w = w; wk.h = h;
    }
    return MLVFS_AMD_OK;
}

}  // namespace

void amaze_render_trim()
{
    for (auto &kv : t_amz) {
        if (kv.second.planes.p || kv.second.tiles.p) (void)hipDeviceSynchronize();
        kv.second.planes.release(); kv.second.tiles.release();
        kv.second.zeroed = nullptr; kv.second.zeroed_bytes = 0; kv.second.w = kv.second.h = 0;
    }
}

namespace {

// balance -> AMaZE -> the last pass for nframes frames, `sub` at a time: the tone pass (ow == 0, the full-size rendering) or the
// resampling pass to ow x oh.  A sub-batch that cannot be reserved is halved until one frame is left: a batch fails only where a single
// frame's work memory cannot be had.  The callers check the geometry
int amaze_batches(ThreadCtx *c, const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h, int ow,
                  int oh, int nframes, hipStream_t stream, const LookArg *lk, bool deep)
{
    const AmzPlan p = amz_plan(w, h, nframes, AMZ_WORK_CAP);
    if (p.tile_stride * sizeof(float) != amaze_scratch_bytes(w, h)) { set_error("amaze_render: the tile planes of %dx%d are sized wrongly", w, h); return MLVFS_AMD_ERR_ARG; }
    AmzWork &wk = t_amz[c->dev->id];
    int sub = p.sub;
    for (;;) {
        const int rc = amz_reserve(wk, p, sub, w, h, stream);
        if (rc == MLVFS_AMD_OK) break;
        if (sub == 1) return rc;
        sub = (sub + 1) / 2;
    }
    float *raw = wk.planes, *red = raw + (size_t)sub * p.plane_stride, *green = red + (size_t)sub * p.plane_stride, *blue = green + (size_t)sub * p.plane_stride;
    for (int f0 = 0; f0 < nframes; f0 += sub) {
        const int n = std::min(sub, nframes - f0);
        const int32_t *par = d_params + (size_t)f0 * RGB_PARAMS;
        int rc = launch_amz_balance((const uint8_t *)d_frames + (size_t)f0 * stride, stride, par, raw, p.plane_stride, w, h, n, stream);
        if (!rc) rc = amaze_launch(raw, w, h, red, green, blue, wk.tiles, stream, n, p.plane_stride, p.tile_stride);
        uint8_t *dst = (uint8_t *)d_out + (size_t)f0 * out_stride;
        if (!rc) rc = ow ? launch_amz_resample(red, green, blue, p.plane_stride, par, dst, out_stride, w, h, ow, oh, n, stream, lk, deep)
                         : launch_amz_tone(red, green, blue, p.plane_stride, par, dst, out_stride, w, h, n, stream, lk, deep);
        if (rc) return rc;
    }
    return MLVFS_AMD_OK;
}

}  // namespace

int launch_render1_amaze(ThreadCtx *c, const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w, int h,
                         int nframes, hipStream_t stream, const LookArg *lk, bool deep)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (!rgb_amaze_geom(w, h)) return route_refuse("launch_render1_amaze", { RenderRoute::FULL, true }, w, h);
    return amaze_batches(c, d_frames, stride, d_params, d_out, out_stride, w, h, 0, 0, nframes, stream, lk, deep);
}

// the same loop with the resampling pass behind AMaZE (k_amaze_resample.hip) in the place of the tone pass
int launch_render_resampled_amaze(ThreadCtx *c, const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride, int w,
                                  int h, int ow, int oh, int nframes, hipStream_t stream, const LookArg *lk, bool deep)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (!amz_resample_geom(w, h, ow, oh)) return route_refuse("launch_render_resampled_amaze", { RenderRoute::RESAMPLED, true, ow, oh }, w, h);
    return amaze_batches(c, d_frames, stride, d_params, d_out, out_stride, w, h, ow, oh, nframes, stream, lk, deep);
}

}  // namespace mlv

using namespace mlv;

namespace {

bool overlap(uintptr_t a0, size_t an, uintptr_t b0, size_t bn) { return a0 < b0 + bn && b0 < a0 + an; }

// mlvfs_amd_amaze_tone_dev (r: the full-size AMaZE route) and mlvfs_amd_amaze_resample_dev (r: the resampled one): the last pass alone,
// from three float planes; every check before any device work
int amaze_plane_dev(const char *who, const RenderRoute &r, const float *d_red, const float *d_green, const float *d_blue, size_t plane_stride,
                    int width, int height, const int32_t *d_params, void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look_t *look,
                    const mlvfs_amd_look16_t *look16, void *stream)
{
    if (!d_red || !d_green || !d_blue || !d_params || !d_out) { set_error("%s: null argument", who); return MLVFS_AMD_ERR_ARG; }
    if (look && look16) { set_error("%s: a look and a deep look in one call", who); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("%s: negative frame count", who); return MLVFS_AMD_ERR_ARG; }
    int pw, ph;
    if (!route_geom(r, width, height, &pw, &ph)) return route_refuse(who, r, width, height);
    const size_t npix = (size_t)width * height, pimg = (size_t)(look16 ? 6 : 3) * pw * ph;
    if ((((uintptr_t)d_red | (uintptr_t)d_green | (uintptr_t)d_blue | (uintptr_t)d_params) & 3)) { set_error("%s: planes or parameters off a 4-byte boundary", who); return MLVFS_AMD_ERR_ARG; }
    if (nframes > 1 && (plane_stride < npix || out_stride < pimg)) {
        set_error("%s: strides %zu / %zu too small", who, plane_stride, out_stride);
        return MLVFS_AMD_ERR_ARG;
    }
    if (nframes == 0) return MLVFS_AMD_OK;
    const uintptr_t b0 = (uintptr_t)d_out;
    const size_t bn = (size_t)(nframes - 1) * out_stride + pimg, an = ((size_t)(nframes - 1) * plane_stride + npix) * sizeof(float);
    if (overlap((uintptr_t)d_red, an, b0, bn) || overlap((uintptr_t)d_green, an, b0, bn) || overlap((uintptr_t)d_blue, an, b0, bn) ||
        overlap((uintptr_t)d_params, (size_t)nframes * RGB_PARAMS * sizeof(int32_t), b0, bn)) {
        set_error("%s: the destination overlaps a plane or the parameters", who);
        return MLVFS_AMD_ERR_ARG;
    }
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    LookArg lk;
    if (look) if (const int rc = look_on_device(look, c, &lk)) return rc;
    if (look16) if (const int rc = look16_on_device(look16, c, &lk)) return rc;
    const LookArg *lkp = look || look16 ? &lk : nullptr;
    hipStream_t s = pick_stream(stream, c);
    return r.sized() ? launch_amz_resample(d_red, d_green, d_blue, plane_stride, d_params, d_out, out_stride, width, height, pw, ph, nframes, s, lkp, look16 != nullptr)
                     : launch_amz_tone(d_red, d_green, d_blue, plane_stride, d_params, d_out, out_stride, width, height, nframes, s, lkp, look16 != nullptr);
}

}  // namespace

extern "C" {

int mlvfs_amd_amaze_balance_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, float *d_planes,
                                size_t plane_stride, int nframes, void *stream)
{
    if (!d_frames || !d_planes || !d_params) { set_error("amaze_balance: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("amaze_balance: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    if (!rgb_amaze_geom(width, height)) return route_refuse("amaze_balance", { RenderRoute::FULL, true }, width, height);
    const size_t npix = (size_t)width * height, img = npix * 2;
    if (((uintptr_t)d_frames & 1) || ((uintptr_t)d_params & 3) || ((uintptr_t)d_planes & 3)) { set_error("amaze_balance: an odd source address, or parameters or planes off a 4-byte boundary"); return MLVFS_AMD_ERR_ARG; }
    if (nframes > 1 && (stride < img || plane_stride < npix || (stride & 1))) {
        set_error("amaze_balance: strides %zu / %zu too small, or an odd source stride", stride, plane_stride);
        return MLVFS_AMD_ERR_ARG;
    }
    if (nframes == 0) return MLVFS_AMD_OK;
    const uintptr_t b0 = (uintptr_t)d_planes;
    const size_t bn = ((size_t)(nframes - 1) * plane_stride + npix) * sizeof(float);
    if (overlap((uintptr_t)d_frames, (size_t)(nframes - 1) * stride + img, b0, bn) || overlap((uintptr_t)d_params, (size_t)nframes * RGB_PARAMS * sizeof(int32_t), b0, bn)) {
        set_error("amaze_balance: the planes overlap the source or the parameters");
        return MLVFS_AMD_ERR_ARG;
    }
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    return launch_amz_balance(d_frames, stride, d_params, d_planes, plane_stride, width, height, nframes, pick_stream(stream, c));
}

int mlvfs_amd_amaze_tone_dev(const float *d_red, const float *d_green, const float *d_blue, size_t plane_stride, int width, int height,
                             const int32_t *d_params, void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look_t *look,
                             const mlvfs_amd_look16_t *look16, void *stream)
{
    return amaze_plane_dev("amaze_tone", { RenderRoute::FULL, true }, d_red, d_green, d_blue, plane_stride, width, height, d_params, d_out, out_stride,
                           nframes, look, look16, stream);
}

int mlvfs_amd_amaze_resample_dev(const float *d_red, const float *d_green, const float *d_blue, size_t plane_stride, int width, int height,
                                 const int32_t *d_params, int ow, int oh, void *d_out, size_t out_stride, int nframes,
                                 const mlvfs_amd_look_t *look, const mlvfs_amd_look16_t *look16, void *stream)
{
    return amaze_plane_dev("amaze_resample", { RenderRoute::RESAMPLED, true, ow, oh }, d_red, d_green, d_blue, plane_stride, width, height, d_params, d_out,
                           out_stride, nframes, look, look16, stream);
}

/* test hook, host only: how launch_amz_resample would divide a launch among workgroups.  out[0]: 1 the x16 form (for aligned planes), 0
   the generic one; [1] the most source columns of a strip; [2] uo, the output columns of a strip: strip k begins at column k uo; [3] the
   strips; [4] bo, the output rows of a band: band k begins at row k bo; [5] the bands; [6] the source rows a band covers at least;
   [7] the source rows of a step */
int mlvfs_amd_test_amz_resample_plan(int width, int height, int ow, int oh, int nframes, int32_t out[8])
{
    if (!out || nframes < 1 || !amz_resample_geom(width, height, ow, oh)) { set_error("test_amz_resample_plan: bad argument"); return MLVFS_AMD_ERR_ARG; }
    int32_t v[8] = { 0, RS_STRIP, 0, 0, 0, 0, RS_BAND_ROWS, RS_ROWS };
    if (amz_resample_fast_geom(width, ow)) {
        const ResamplePlan p = resample_plan(width, height, ow, oh, nframes);
        v[0] = 1; v[2] = (int32_t)p.uo; v[3] = (int32_t)p.nstrips; v[4] = (int32_t)p.bo; v[5] = (int32_t)p.nbands;
    }
    std::copy(v, v + 8, out);
    return MLVFS_AMD_OK;
}

/* test hook, host only: how a batch of nframes frames is cut into sub-batches that fit cap_bytes of work memory (0: the library's own cap) */
int mlvfs_amd_test_amaze_render_plan(int width, int height, int nframes, size_t cap_bytes, int64_t out[4])
{
    if (!out || nframes < 1 || !rgb_amaze_geom(width, height)) { set_error("test_amaze_render_plan: bad argument"); return MLVFS_AMD_ERR_ARG; }
    const AmzPlan p = amz_plan(width, height, nframes, cap_bytes ? cap_bytes : AMZ_WORK_CAP);
    out[0] = (int64_t)p.plane_stride; out[1] = (int64_t)p.tile_stride; out[2] = (int64_t)p.frame_bytes; out[3] = p.sub;
    return MLVFS_AMD_OK;
}

}  // extern "C"

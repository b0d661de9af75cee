// render_route.cpp -- the rendering routes on the host (render_route.h): each route's geometry rule, the words of its limits and its
// launcher, once; the one checked body of the eighteen device entry points mlvfs_amd_render*_dev (six routes x plain, look, deep); the
// exported geometry and fit calls; the plan test hooks of the scaled and the resampled kernels.  Nothing here knows a mount.
#include "clip.h"
#include "render_route.h"

using namespace mlv;

namespace mlv {

bool route_geom(const RenderRoute &r, int w, int h, int *pw, int *ph)
{
    int gw = w, gh = h;
    bool ok = false;
    switch (r.size) {
    case RenderRoute::HALF: ok = rgb_geom(w, h, &gw, &gh); break;
    case RenderRoute::FULL: ok = r.amaze ? rgb_amaze_geom(w, h) : rgb_full_geom(w, h); break;
    case RenderRoute::SCALED: ok = scale_geom(w, h, r.ow, r.oh, &gw, &gh); break;
    case RenderRoute::RESAMPLED: ok = r.amaze ? amz_resample_geom(w, h, r.ow, r.oh) : resample_geom(w, h, r.ow, r.oh); break;
    }
    if (!ok) return false;
    *pw = r.sized() ? r.ow : gw;
    *ph = r.sized() ? r.oh : gh;
    return true;
}

int route_refuse(const char *who, const RenderRoute &r, int w, int h)
{
    const char *limits = "a half-size rendering takes frames of 2x2 up to 2^27 pixels";
    switch (r.size) {
    case RenderRoute::HALF: break;
    case RenderRoute::FULL:
        limits = r.amaze ? "an AMaZE rendering takes frames of 36x36 up to 2^25 pixels, the width a multiple of 4"
                         : "a full-size rendering takes frames of 4x4 up to 2^25 pixels";
        break;
    case RenderRoute::SCALED:
        limits = "a scaled rendering takes frames of 2x2 up to 2^27 pixels, 65535 a side at half size, and gives 1x1 up to the half size";
        break;
    case RenderRoute::RESAMPLED:
        limits = r.amaze ? "a resampled AMaZE rendering takes frames of 36x36 up to 2^25 pixels, 65535 a side, the width a multiple of 4, and gives 1x1 up to the frame's size"
                         : "a resampled rendering takes frames of 4x4 up to 2^25 pixels, 65535 a side, and gives 1x1 up to the frame's size";
        break;
    }
    if (r.sized()) set_error("%s: %dx%d to %dx%d not supported: %s", who, w, h, r.ow, r.oh, limits);
    else set_error("%s: %dx%d not supported: %s", who, w, h, limits);
    return MLVFS_AMD_ERR_ARG;
}

int route_launch(const RenderRoute &r, ThreadCtx *c, const void *d_frames, size_t stride, const int32_t *d_params, void *d_out, size_t out_stride,
                 int w, int h, int nframes, hipStream_t stream, const LookArg *lk, bool deep)
{
    switch (r.size) {
    case RenderRoute::HALF: return launch_render2(d_frames, stride, d_params, d_out, out_stride, w, h, nframes, stream, lk, deep);
    case RenderRoute::FULL:
        return r.amaze ? launch_render1_amaze(c, d_frames, stride, d_params, d_out, out_stride, w, h, nframes, stream, lk, deep)
                       : launch_render1(d_frames, stride, d_params, d_out, out_stride, w, h, nframes, stream, lk, deep);
    case RenderRoute::SCALED: return launch_render_scaled(d_frames, stride, d_params, d_out, out_stride, w, h, r.ow, r.oh, nframes, stream, lk, deep);
    case RenderRoute::RESAMPLED:
        return r.amaze ? launch_render_resampled_amaze(c, d_frames, stride, d_params, d_out, out_stride, w, h, r.ow, r.oh, nframes, stream, lk, deep)
                       : launch_render_resampled(d_frames, stride, d_params, d_out, out_stride, w, h, r.ow, r.oh, nframes, stream, lk, deep);
    }
    set_error("route_launch: no such route");
    return MLVFS_AMD_ERR_ARG;
}

}  // namespace mlv

namespace {

// what a device entry point is called with, apart from its route and its look
struct DevCall {
    const void *d_frames;
    size_t stride;
    int width, height;
    const int32_t *d_params;
    void *d_out;
    size_t out_stride;
    int nframes;
    void *stream;
};

// which of a route's three forms an entry point is: the plain one, or the one that takes a look or a deep look, which is then required
struct Tone {
    const mlvfs_amd_look_t *look = nullptr;
    const mlvfs_amd_look16_t *deep = nullptr;
    bool with_look = false, with_deep = false;
};
Tone with_look(const mlvfs_amd_look_t *look) { return { look, nullptr, true, false }; }
Tone with_deep(const mlvfs_amd_look16_t *deep) { return { nullptr, deep, false, true }; }

// every mlvfs_amd_render*_dev call: all checks before any device work, then the route's launcher
int render_dev(const char *who, const RenderRoute &r, const DevCall &a, const Tone &t = Tone())
{
    if (!a.d_frames || !a.d_out || !a.d_params || (t.with_look && !t.look) || (t.with_deep && !t.deep)) { set_error("%s: null argument", who); return MLVFS_AMD_ERR_ARG; }
    if (a.nframes < 0) { set_error("%s: negative frame count", who); return MLVFS_AMD_ERR_ARG; }
    int pw, ph;
    if (!route_geom(r, a.width, a.height, &pw, &ph)) return route_refuse(who, r, a.width, a.height);
    const size_t img = (size_t)a.width * a.height * 2, pimg = (size_t)(t.with_deep ? 6 : 3) * pw * ph;
    if (((uintptr_t)a.d_frames & 1) || ((uintptr_t)a.d_params & 3)) { set_error("%s: an odd source address, or parameters off a 4-byte boundary", who); return MLVFS_AMD_ERR_ARG; }
    if (a.nframes > 1 && (a.stride < img || a.out_stride < pimg || (a.stride & 1))) {
        set_error("%s: strides %zu / %zu too small, or an odd source stride", who, a.stride, a.out_stride);
        return MLVFS_AMD_ERR_ARG;
    }
    if (a.nframes == 0) return MLVFS_AMD_OK;
    const uintptr_t a0 = (uintptr_t)a.d_frames, a1 = a0 + (size_t)(a.nframes - 1) * a.stride + img;
    const uintptr_t b0 = (uintptr_t)a.d_out, b1 = b0 + (size_t)(a.nframes - 1) * a.out_stride + pimg;
    const uintptr_t p0 = (uintptr_t)a.d_params, p1 = p0 + (size_t)a.nframes * RGB_PARAMS * sizeof(int32_t);
    if ((a0 < b1 && b0 < a1) || (p0 < b1 && b0 < p1)) { set_error("%s: the destination overlaps the source or the parameters (the rendering does not work in place)", who); return MLVFS_AMD_ERR_ARG; }
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    LookArg lk;
    if (t.with_look) if (const int rc = look_on_device(t.look, c, &lk)) return rc;
    if (t.with_deep) if (const int rc = look16_on_device(t.deep, c, &lk)) return rc;
    return route_launch(r, c, a.d_frames, a.stride, a.d_params, a.d_out, a.out_stride, a.width, a.height, a.nframes, pick_stream(a.stream, c),
                        t.with_look || t.with_deep ? &lk : nullptr, t.with_deep);
}

// mlvfs_amd_rgb_geom and its kin: W' x H' of a frame the route takes
int geom_export(const char *who, const RenderRoute &r, int width, int height, int *pw, int *ph)
{
    if (!pw || !ph) { set_error("%s: null argument", who); return MLVFS_AMD_ERR_ARG; }
    return route_geom(r, width, height, pw, ph) ? MLVFS_AMD_OK : route_refuse(who, r, width, height);
}

// the largest size inside a box at the aspect of the gw x gh grid, neither side above the grid's
int fit(const char *who, const RenderRoute &r, int width, int height, int box_w, int box_h, int *ow, int *oh)
{
    if (!ow || !oh) { set_error("%s: null argument", who); return MLVFS_AMD_ERR_ARG; }
    int one_w, one_h;
    if (box_w < 1 || box_h < 1 || !route_geom(r, width, height, &one_w, &one_h)) {
        set_error("%s: a box of %dx%d, or a %dx%d frame that the %s rendering does not take", who, box_w, box_h, width, height, r.size == RenderRoute::SCALED ? "scaled" : "resampled");
        return MLVFS_AMD_ERR_ARG;
    }
    const int gw = r.size == RenderRoute::SCALED ? width / 2 : width, gh = r.size == RenderRoute::SCALED ? height / 2 : height;
    int64_t fw = gw, fh = gh;
    if (box_w < gw || box_h < gh) {
        if ((int64_t)box_w * gh <= (int64_t)box_h * gw) {                // the width limits
            fw = std::min(box_w, gw);
            fh = std::max<int64_t>(1, (2 * fw * gh + gw) / (2 * (int64_t)gw));
        } else {
            fh = std::min(box_h, gh);
            fw = std::max<int64_t>(1, (2 * fh * gw + gh) / (2 * (int64_t)gh));
        }
    }
    *ow = (int)fw;
    *oh = (int)fh;
    return MLVFS_AMD_OK;
}

constexpr RenderRoute kHalf{ RenderRoute::HALF }, kFull{ RenderRoute::FULL }, kFullAmaze{ RenderRoute::FULL, true };
RenderRoute scaled(int ow, int oh) { return { RenderRoute::SCALED, false, ow, oh }; }
RenderRoute resampled(int ow, int oh, bool amaze = false) { return { RenderRoute::RESAMPLED, amaze, ow, oh }; }

}  // namespace

extern "C" {

int mlvfs_amd_rgb_geom(int width, int height, int *pw, int *ph) { return geom_export("rgb_geom", kHalf, width, height, pw, ph); }
int mlvfs_amd_rgb_full_geom(int width, int height, int *pw, int *ph) { return geom_export("rgb_full_geom", kFull, width, height, pw, ph); }
int mlvfs_amd_rgb_amaze_geom(int width, int height, int *pw, int *ph) { return geom_export("rgb_amaze_geom", kFullAmaze, width, height, pw, ph); }
int mlvfs_amd_rgb_amaze_resample_geom(int width, int height, int ow, int oh)
{
    int pw, ph;
    return geom_export("rgb_amaze_resample_geom", resampled(ow, oh, true), width, height, &pw, &ph);
}

int mlvfs_amd_rgb_fit(int width, int height, int box_w, int box_h, int *ow, int *oh) { return fit("rgb_fit", scaled(1, 1), width, height, box_w, box_h, ow, oh); }
int mlvfs_amd_rgb_fit_full(int width, int height, int box_w, int box_h, int *ow, int *oh)
{
    return fit("rgb_fit_full", resampled(1, 1), width, height, box_w, box_h, ow, oh);
}

int mlvfs_amd_render2_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out, size_t out_stride,
                          int nframes, void *stream)
{
    return render_dev("render2", kHalf, { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream });
}
int mlvfs_amd_render2_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                               size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream)
{
    return render_dev("render2", kHalf, { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_look(look));
}
int mlvfs_amd_render2_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                               size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream)
{
    return render_dev("render2", kHalf, { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_deep(look));
}

int mlvfs_amd_render1_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out, size_t out_stride,
                          int nframes, void *stream)
{
    return render_dev("render1", kFull, { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream });
}
int mlvfs_amd_render1_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                               size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream)
{
    return render_dev("render1", kFull, { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_look(look));
}
int mlvfs_amd_render1_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                               size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream)
{
    return render_dev("render1", kFull, { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_deep(look));
}

int mlvfs_amd_render1_amaze_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                                size_t out_stride, int nframes, void *stream)
{
    return render_dev("render1_amaze", kFullAmaze, { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream });
}
int mlvfs_amd_render1_amaze_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                                     size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream)
{
    return render_dev("render1_amaze", kFullAmaze, { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_look(look));
}
int mlvfs_amd_render1_amaze_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                                     size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream)
{
    return render_dev("render1_amaze", kFullAmaze, { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_deep(look));
}

int mlvfs_amd_render_scaled_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh, void *d_out,
                                size_t out_stride, int nframes, void *stream)
{
    return render_dev("render_scaled", scaled(ow, oh), { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream });
}
int mlvfs_amd_render_scaled_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                     void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream)
{
    return render_dev("render_scaled", scaled(ow, oh), { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_look(look));
}
int mlvfs_amd_render_scaled_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                     void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream)
{
    return render_dev("render_scaled", scaled(ow, oh), { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_deep(look));
}

int mlvfs_amd_render_resampled_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                   void *d_out, size_t out_stride, int nframes, void *stream)
{
    return render_dev("render_resampled", resampled(ow, oh), { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream });
}
int mlvfs_amd_render_resampled_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                        void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream)
{
    return render_dev("render_resampled", resampled(ow, oh), { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_look(look));
}
int mlvfs_amd_render_resampled_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                        void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream)
{
    return render_dev("render_resampled", resampled(ow, oh), { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_deep(look));
}

int mlvfs_amd_render_resampled_amaze_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                         void *d_out, size_t out_stride, int nframes, void *stream)
{
    return render_dev("render_resampled_amaze", resampled(ow, oh, true), { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream });
}
int mlvfs_amd_render_resampled_amaze_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                              void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream)
{
    return render_dev("render_resampled_amaze", resampled(ow, oh, true), { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_look(look));
}
int mlvfs_amd_render_resampled_amaze_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                              void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream)
{
    return render_dev("render_resampled_amaze", resampled(ow, oh, true), { d_frames, stride, width, height, d_params, d_out, out_stride, nframes, stream }, with_deep(look));
}

/* test hooks, host only: floor(in[k] / d) as k_scale_x16 computes it; how launch_render_scaled and launch_render_resampled would divide
   a launch among workgroups */
int mlvfs_amd_test_scale_div(uint32_t d, int n, const uint32_t *in, uint32_t *out)
{
    if (!d || n < 0 || !in || !out) { set_error("test_scale_div: bad argument"); return MLVFS_AMD_ERR_ARG; }
    const ScDiv dv = scdiv_make(d);
    for (int k = 0; k < n; k++) out[k] = scdiv_host(in[k], dv);
    return MLVFS_AMD_OK;
}

int mlvfs_amd_test_scale_plan(int width, int height, int ow, int oh, int nframes, int32_t out[8])
{
    int pw, ph;
    if (!out || nframes < 1 || !scale_geom(width, height, ow, oh, &pw, &ph)) { set_error("test_scale_plan: bad argument"); return MLVFS_AMD_ERR_ARG; }
    const ScalePlan p = scale_plan(pw, ph, ow, oh, nframes);
    const int32_t v[8] = { width % 16 == 0, SC_CHUNK, SC_STRIP, (int32_t)p.uo, (int32_t)p.nstrips, (int32_t)p.bo, (int32_t)p.nbands, SC_BAND_ROWS };
    std::copy(v, v + 8, out);
    return MLVFS_AMD_OK;
}

int mlvfs_amd_test_resample_plan(int width, int height, int ow, int oh, int nframes, int32_t out[8])
{
    if (!out || nframes < 1 || !resample_geom(width, height, ow, oh)) { set_error("test_resample_plan: bad argument"); return MLVFS_AMD_ERR_ARG; }
    int32_t v[8] = { 0, RS_STRIP, 0, 0, 0, 0, RS_BAND_ROWS, RS_ROWS };
    if (resample_fast_geom(width, ow)) {
        const ResamplePlan p = resample_plan(width, height, ow, oh, nframes);
        v[0] = 1; v[2] = (int32_t)p.uo; v[3] = (int32_t)p.nstrips; v[4] = (int32_t)p.bo; v[5] = (int32_t)p.nbands;
    }
    std::copy(v, v + 8, out);
    return MLVFS_AMD_OK;
}

}  // extern "C"

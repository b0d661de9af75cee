// cal.cpp -- the calibration stage's host side: dark frames and flat fields (k_cal.hip).  Both are a handle with a
// host plane that is uploaded once per device -- the dark plane itself, or the flat field's Q14 gain plane --, made from a plane given
// on the host or from the mean of a clip's frames summed on the GPU in batches, and applied in place to device frames.
//
//     out     = clamp(px - dark + black_d, 0, 2^bpp - 1)          black_d: the black level of the clip the plane was averaged from
//     dark[p] = (sum over n frames of px_f[p] + n / 2) / n        1 <= n <= 65536
//     s[p]    = max(F[p] - black_f, 1)          black_f: the black level of the clip the flat plane F was averaged from
//     M_c     = (sum of s[p] over channel c + n_c / 2) / n_c          c = (y & 1) * 2 + (x & 1); 64-bit sums
//     gain[p] = min((M_c * 16384 + s[p] / 2) / s[p], 65535)           Q14: gains stop just under 4.0
//     out     = clamp(black + floor(((px - black) * gain[p] + 8192) / 16384), 0, 2^bpp - 1)       the frame's own black and bpp
// The planes are applied by position in the stored frame (xRes x yRes): panPosX/Y and cropPosX/Y are ignored.  The reference has no
// such stage.  The mount (mount.cpp) and the transcoder (mlvwriter.cpp) hand the handles' device planes (calib_on_device) to the
// reader's load (mlvreader.cpp: reader_load_list), which subtracts as stage 0 and corrects as stage 0b, in one pass.
//
// mlvfs_amd_{dark,flat}_create / _info / _plane / _gain / _destroy and every argument check are host code: no HIP device is needed.
#include "clip.h"

#include <cstring>
#include <map>

using namespace mlv;

// what both handles are.  They are const to their users: the per-device copies appear behind the mutex, on a device's first use.
struct CalPlane {
    int w = 0, h = 0, bpp = 0, black = 0;               // of the plane given or averaged (a gain plane itself has no depth)
    int averaged = 0;                                   // frames the plane is the mean of; 0: given to _create
    std::vector<uint16_t> plane;                        // the dark plane; the flat field's gain plane
    mutable std::mutex mu;
    mutable std::map<int, void *> on_dev;

    ~CalPlane() { for (auto &kv : on_dev) if (kv.second) (void)hipFree(kv.second); }

    // the plane on c's device; what: "dark: uploading the plane"
    int on_device(const char *what, ThreadCtx *c, const uint16_t **d_plane) const
    {
        std::lock_guard<std::mutex> lk(mu);
        void *&p = on_dev[c->dev->id];
        if (!p) {
            void *fresh = nullptr;
            MLV_HIP(hipMalloc(&fresh, plane.size() * 2));
            const hipError_t e = hipMemcpy(fresh, plane.data(), plane.size() * 2, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(fresh);
                set_error("%s -> %s", what, hipGetErrorString(e));
                return MLVFS_AMD_ERR_HIP;
            }
            p = fresh;
        }
        *d_plane = (const uint16_t *)p;
        return MLVFS_AMD_OK;
    }
};
struct mlvfs_amd_dark : CalPlane {};
struct mlvfs_amd_flat : CalPlane {
    uint32_t mean[4] = { 0, 0, 0, 0 };                  // M_c; 0 for a channel without pixels
};

namespace {

// false with the error set: a non-positive size or 2^27 pixels and more, bpp outside 1..16, a pedestal outside 0..65535
bool plane_geometry_ok(const char *who, int w, int h, int bpp, int black)
{
    if (w <= 0 || h <= 0 || (uint64_t)w * h >= (1u << 27)) { set_error("%s: %dx%d not supported", who, w, h); return false; }
    if (bpp < 1 || bpp > 16) { set_error("%s: unsupported bits_per_pixel %d", who, bpp); return false; }
    if (black < 0 || black > 65535) { set_error("%s: pedestal %d outside 0..65535", who, black); return false; }
    return true;
}

// the one geometry of frames first .. first + count - 1 and frame first's black level into p (false, with the error set: frames
// outside the clip, count outside 1..65536, unusable headers, more than one geometry)
bool clip_mean_geometry(const char *who, const void *reader, int first, int count, CalPlane &p)
{
    const int frames = mlvfs_amd_mlv_frame_count(reader);
    if (count < 1 || count > 65536) { set_error("%s: a mean of %d frames (1..65536)", who, count); return false; }
    if (first < 0 || (long long)first + count > frames) { set_error("%s: frames %d..%lld outside the clip (%d frames)", who, first, (long long)first + count - 1, frames); return false; }
    for (int k = 0; k < count; k++) {
        frame_headers fh;
        if (!mlvfs_amd_mlv_frame_headers(reader, first + k, &fh)) { set_error("%s: frame %d has no usable headers", who, first + k); return false; }
        const int fw = fh.rawi_hdr.xRes, fhh = fh.rawi_hdr.yRes, fb = fh.rawi_hdr.raw_info.bits_per_pixel;
        if (k == 0) {
            if (!plane_geometry_ok(who, fw, fhh, fb, fh.rawi_hdr.raw_info.black_level)) return false;
            p.w = fw; p.h = fhh; p.bpp = fb; p.black = fh.rawi_hdr.raw_info.black_level;
        } else if (fw != p.w || fhh != p.h || fb != p.bpp) {
            set_error("%s: frames of more than one geometry (frame %d)", who, first + k);
            return false;
        }
    }
    return true;
}

// the rounded mean of those frames as w * h 16-bit values at d_mean (16-byte aligned), summed in batches; s is drained on return
int clip_mean_dev(const void *reader, int first, int count, const CalPlane &p, int batch, int io_threads, uint16_t *d_mean, hipStream_t s)
{
    const uint32_t npix = (uint32_t)p.w * (uint32_t)p.h;
    const size_t dstride = up256((size_t)npix * 2);
    DevBuf frames, sums;
    if (const int rc0 = frames.reserve(dstride * (size_t)batch)) return rc0;
    if (const int rc0 = sums.reserve((size_t)npix * 4)) return rc0;
    MLV_HIP(hipMemsetAsync(sums.p, 0, (size_t)npix * 4, s));
    int rc = MLVFS_AMD_OK;
    std::vector<int> kind(count);
    for (int k = 0; k < count; k++) {
        frame_headers fh;
        (void)mlvfs_amd_mlv_frame_headers(reader, first + k, &fh);          // (the caller has read them all once)
        kind[k] = payload_kind(fh.file_hdr.videoClass);
    }
    for (int f0 = 0, n; rc == MLVFS_AMD_OK && f0 < count; f0 += n) {
        for (n = 1; n < batch && f0 + n < count && kind[f0 + n] == kind[f0]; n++) {}
        rc = reader_load_batch(reader, first + f0, n, p.w, p.h, p.bpp, frames.p, dstride, io_threads, s);
        if (rc == MLVFS_AMD_OK) rc = launch_dark_accum(frames.p, dstride, npix, n, (uint32_t *)sums.p, s);
    }
    if (rc == MLVFS_AMD_OK) rc = launch_dark_mean((const uint32_t *)sums.p, d_mean, npix, (uint32_t)count, s);
    (void)hipStreamSynchronize(s);                      // frames and sums go away here
    return rc;
}

// a dark frame: the mean, downloaded
int mean_of_clip(const void *reader, int first, int count, int batch, int io_threads, mlvfs_amd_dark &d)
{
    const uint32_t npix = (uint32_t)d.w * (uint32_t)d.h;
    LibcRandGuard rand_guard;                           // HIP code runs: the caller's rand() stream stays out of its reach
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    hipStream_t s = c->stream;
    DevBuf mean;
    if (const int rc0 = mean.reserve((size_t)npix * 2)) return rc0;
    const int rc = clip_mean_dev(reader, first, count, d, batch, io_threads, (uint16_t *)mean.p, s);
    if (rc != MLVFS_AMD_OK) return rc;
    d.plane.resize(npix);
    MLV_HIP(hipMemcpyAsync(d.plane.data(), mean.p, (size_t)npix * 2, hipMemcpyDeviceToHost, s));
    MLV_HIP(hipStreamSynchronize(s));
    return MLVFS_AMD_OK;
}

uint32_t signal_of(uint16_t f, int black_f) { return (uint32_t)std::max((int)f - black_f, 1); }

// the gain plane's definition, on the host: what k_flat_chan_sums and k_flat_gain compute
void gains_on_host(mlvfs_amd_flat &f, const uint16_t *plane)
{
    const size_t w = (size_t)f.w, h = (size_t)f.h;
    uint64_t sum[4] = { 0, 0, 0, 0 }, n[4] = { 0, 0, 0, 0 };
    for (size_t y = 0; y < h; y++)
        for (size_t x = 0; x < w; x++) {
            const int c = (int)((y & 1) * 2 + (x & 1));
            sum[c] += signal_of(plane[y * w + x], f.black);
            n[c]++;
        }
    for (int c = 0; c < 4; c++) f.mean[c] = n[c] ? (uint32_t)((sum[c] + n[c] / 2) / n[c]) : 0;
    f.plane.resize(w * h);
    for (size_t y = 0; y < h; y++)
        for (size_t x = 0; x < w; x++) {
            const uint32_t s = signal_of(plane[y * w + x], f.black), m = f.mean[(y & 1) * 2 + (x & 1)];
            f.plane[y * w + x] = (uint16_t)std::min<uint32_t>((m * 16384u + s / 2) / s, 65535u);
        }
}

// a flat field: the mean, the dark frame subtracted from it, the two gain kernels, one download: gain plane and means together
int gains_of_clip(const void *reader, int first, int count, const mlvfs_amd_dark_t *dark, int batch, int io_threads, mlvfs_amd_flat &f)
{
    const uint32_t npix = (uint32_t)f.w * (uint32_t)f.h;
    const size_t gain_bytes = ((size_t)npix * 2 + 15) / 16 * 16;
    LibcRandGuard rand_guard;                           // HIP code runs: the caller's rand() stream stays out of its reach
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    hipStream_t s = c->stream;
    Calib cal;
    if (int rc = calib_on_device(dark, nullptr, c, f.w, f.h, f.bpp, f.black, &cal)) return rc;
    DevBuf mean, out, sums;                             // out: [the gain plane][M_c[4]]
    if (const int rc0 = mean.reserve(gain_bytes)) return rc0;
    if (const int rc0 = out.reserve(gain_bytes + 16)) return rc0;
    if (const int rc0 = sums.reserve(4 * sizeof(unsigned long long))) return rc0;
    int rc = clip_mean_dev(reader, first, count, f, batch, io_threads, (uint16_t *)mean.p, s);
    if (rc == MLVFS_AMD_OK) rc = launch_cal_apply(mean.p, 0, npix, 1, cal, s);
    if (rc == MLVFS_AMD_OK)
        rc = launch_flat_gain((const uint16_t *)mean.p, (uint32_t)f.w, (uint32_t)f.h, f.black, (unsigned long long *)sums.p, (uint16_t *)out.p,
                              (uint32_t *)((uint8_t *)out.p + gain_bytes), s);
    if (rc != MLVFS_AMD_OK) { (void)hipStreamSynchronize(s); return rc; }
    std::vector<uint8_t> host(gain_bytes + 16);
    MLV_HIP(hipMemcpyAsync(host.data(), out.p, host.size(), hipMemcpyDeviceToHost, s));
    MLV_HIP(hipStreamSynchronize(s));
    f.plane.resize(npix);
    memcpy(f.plane.data(), host.data(), (size_t)npix * 2);
    memcpy(f.mean, host.data() + gain_bytes, sizeof f.mean);
    return MLVFS_AMD_OK;
}

// ---- what the two families of entry points do alike, `who` being the name their errors begin with ---------------------------
// _create and _from_clip: a fresh handle that fill() completes (false, with the error set: no handle)
template <class Handle, class Fill>
Handle *make_handle(const char *who, bool args, Fill fill)
{
    if (!args) { set_error("%s: null argument", who); return nullptr; }
    try {
        std::unique_ptr<Handle> p(new Handle);
        return fill(*p) ? p.release() : nullptr;
    } catch (const std::exception &e) { set_error("%s: %s", who, e.what()); return nullptr; }
}

bool geometry_given(const char *who, const mlvfs_amd_geom_t *geom, CalPlane &p)
{
    if (!plane_geometry_ok(who, geom->width, geom->height, geom->bpp, geom->black)) return false;
    p.w = geom->width; p.h = geom->height; p.bpp = geom->bpp; p.black = geom->black;
    return true;
}

int batch_of(int batch_frames, int count) { return std::min(batch_frames <= 0 ? 8 : batch_frames, count); }

int plane_info(const char *who, const CalPlane *p, mlvfs_amd_geom_t *geom, int *frames_averaged)
{
    if (!p) { set_error("%s: null argument", who); return MLVFS_AMD_ERR_ARG; }
    if (geom) *geom = mlvfs_amd_geom_t{ p->w, p->h, p->bpp, p->black, 0, 0, 0 };
    if (frames_averaged) *frames_averaged = p->averaged;
    return MLVFS_AMD_OK;
}

int plane_copy(const char *who, const CalPlane *p, uint16_t *h_plane, size_t cap_pixels)
{
    if (!p || !h_plane) { set_error("%s: null argument", who); return MLVFS_AMD_ERR_ARG; }
    if (cap_pixels < p->plane.size()) { set_error("%s: room for %zu pixels, the plane has %zu", who, cap_pixels, p->plane.size()); return MLVFS_AMD_ERR_ARG; }
    std::copy(p->plane.begin(), p->plane.end(), h_plane);
    return MLVFS_AMD_OK;
}

// the _dev entry points: what they check first ...
bool frames_given(const char *who, const CalPlane *p, const mlvfs_amd_geom_t *geom, const void *d_frames, int nframes)
{
    if (!p || !geom || !d_frames) { set_error("%s: null argument", who); return false; }
    if (nframes < 0) { set_error("%s: negative frame count", who); return false; }
    return true;
}

// ... and, once the handles were found to fit the geometry, how they end
int apply_dev(const char *who, const mlvfs_amd_dark_t *dark, const mlvfs_amd_flat_t *flat, const mlvfs_amd_geom_t *geom, void *d_frames,
              size_t stride, int nframes, void *stream)
{
    const uint32_t npix = (uint32_t)geom->width * (uint32_t)geom->height;
    if (((uintptr_t)d_frames & 1) || (nframes > 1 && (stride < (size_t)npix * 2 || (stride & 1)))) {
        set_error("%s: frames at an odd address, or stride %zu too small or odd", who, stride);
        return MLVFS_AMD_ERR_ARG;
    }
    if (nframes == 0) return MLVFS_AMD_OK;
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    Calib cal;
    if (int rc = calib_on_device(dark, flat, c, geom->width, geom->height, geom->bpp, geom->black, &cal)) return rc;
    return launch_cal_apply(d_frames, stride, npix, nframes, cal, pick_stream(stream, c));
}

}  // namespace

bool mlv::darkframe_fits(const mlvfs_amd_dark_t *dark, int w, int h, int bpp) { return dark->w == w && dark->h == h && dark->bpp == bpp; }
bool mlv::flatfield_fits(const mlvfs_amd_flat_t *flat, int w, int h) { return flat->w == w && flat->h == h; }

int mlv::calib_on_device(const mlvfs_amd_dark_t *dark, const mlvfs_amd_flat_t *flat, ThreadCtx *c, int w, int h, int bpp, int black, Calib *out)
{
    *out = Calib{ nullptr, dark ? dark->black : 0, nullptr, black, (1 << bpp) - 1 };
    if (dark && !darkframe_fits(dark, w, h, bpp)) {
        set_error("dark: the dark frame is %dx%d at %d bits, the frames are %dx%d at %d bits", dark->w, dark->h, dark->bpp, w, h, bpp);
        return MLVFS_AMD_ERR_ARG;
    }
    if (dark) if (int rc = dark->on_device("dark: uploading the plane", c, &out->d_dark)) return rc;
    if (flat && !flatfield_fits(flat, w, h)) {
        set_error("flat: the flat field is %dx%d, the frames are %dx%d", flat->w, flat->h, w, h);
        return MLVFS_AMD_ERR_ARG;
    }
    if (flat) if (int rc = flat->on_device("flat: uploading the gain plane", c, &out->d_gain)) return rc;
    return MLVFS_AMD_OK;
}

extern "C" {

mlvfs_amd_dark_t *mlvfs_amd_dark_create(const mlvfs_amd_geom_t *geom, const uint16_t *h_plane)
{
    return make_handle<mlvfs_amd_dark>("dark_create", geom && h_plane, [&](mlvfs_amd_dark &d) {
        if (!geometry_given("dark_create", geom, d)) return false;
        d.plane.assign(h_plane, h_plane + (size_t)d.w * d.h);
        return true;
    });
}

mlvfs_amd_flat_t *mlvfs_amd_flat_create(const mlvfs_amd_geom_t *geom, const uint16_t *h_plane)
{
    return make_handle<mlvfs_amd_flat>("flat_create", geom && h_plane, [&](mlvfs_amd_flat &f) {
        if (!geometry_given("flat_create", geom, f)) return false;
        gains_on_host(f, h_plane);
        return true;
    });
}

mlvfs_amd_dark_t *mlvfs_amd_dark_from_clip(const void *reader, int first, int count, int batch_frames, int io_threads)
{
    return make_handle<mlvfs_amd_dark>("dark_from_clip", reader, [&](mlvfs_amd_dark &d) {
        if (!clip_mean_geometry("dark_from_clip", reader, first, count, d)) return false;
        d.averaged = count;
        return mean_of_clip(reader, first, count, batch_of(batch_frames, count), io_threads, d) == MLVFS_AMD_OK;
    });
}

mlvfs_amd_flat_t *mlvfs_amd_flat_from_clip(const void *reader, int first, int count, const mlvfs_amd_dark_t *dark, int batch_frames,
                                           int io_threads)
{
    return make_handle<mlvfs_amd_flat>("flat_from_clip", reader, [&](mlvfs_amd_flat &f) {
        if (!clip_mean_geometry("flat_from_clip", reader, first, count, f)) return false;
        if (dark && !darkframe_fits(dark, f.w, f.h, f.bpp)) {
            set_error("flat_from_clip: %dx%d at %d bits is not the dark frame's geometry", f.w, f.h, f.bpp);
            return false;
        }
        f.averaged = count;
        return gains_of_clip(reader, first, count, dark, batch_of(batch_frames, count), io_threads, f) == MLVFS_AMD_OK;
    });
}

int mlvfs_amd_dark_info(const mlvfs_amd_dark_t *dark, mlvfs_amd_geom_t *geom, int *frames_averaged)
{
    return plane_info("dark_info", dark, geom, frames_averaged);
}

int mlvfs_amd_flat_info(const mlvfs_amd_flat_t *flat, mlvfs_amd_geom_t *geom, int *frames_averaged, uint32_t means[4])
{
    if (int rc = plane_info("flat_info", flat, geom, frames_averaged)) return rc;
    if (means) std::copy(flat->mean, flat->mean + 4, means);
    return MLVFS_AMD_OK;
}

int mlvfs_amd_dark_plane(const mlvfs_amd_dark_t *dark, uint16_t *h_plane, size_t cap_pixels) { return plane_copy("dark_plane", dark, h_plane, cap_pixels); }
int mlvfs_amd_flat_gain(const mlvfs_amd_flat_t *flat, uint16_t *h_gain, size_t cap_pixels) { return plane_copy("flat_gain", flat, h_gain, cap_pixels); }

void mlvfs_amd_dark_destroy(mlvfs_amd_dark_t *dark) { delete dark; }
void mlvfs_amd_flat_destroy(mlvfs_amd_flat_t *flat) { delete flat; }

int mlvfs_amd_dark_subtract_dev(const mlvfs_amd_dark_t *dark, const mlvfs_amd_geom_t *geom, void *d_frames, size_t stride, int nframes,
                                void *stream)
{
    if (!frames_given("dark_subtract", dark, geom, d_frames, nframes)) return MLVFS_AMD_ERR_ARG;
    if (!darkframe_fits(dark, geom->width, geom->height, geom->bpp)) {
        set_error("dark_subtract: the dark frame is %dx%d at %d bits, the frames are %dx%d at %d bits", dark->w, dark->h, dark->bpp, geom->width,
                  geom->height, geom->bpp);
        return MLVFS_AMD_ERR_ARG;
    }
    return apply_dev("dark_subtract", dark, nullptr, geom, d_frames, stride, nframes, stream);
}

int mlvfs_amd_flat_apply_dev(const mlvfs_amd_flat_t *flat, const mlvfs_amd_dark_t *dark, const mlvfs_amd_geom_t *geom, void *d_frames,
                             size_t stride, int nframes, void *stream)
{
    if (!frames_given("flat_apply", flat, geom, d_frames, nframes)) return MLVFS_AMD_ERR_ARG;
    if (!plane_geometry_ok("flat_apply", geom->width, geom->height, geom->bpp, geom->black)) return MLVFS_AMD_ERR_ARG;
    if (!flatfield_fits(flat, geom->width, geom->height)) {
        set_error("flat_apply: the flat field is %dx%d, the frames are %dx%d", flat->w, flat->h, geom->width, geom->height);
        return MLVFS_AMD_ERR_ARG;
    }
    if (dark && !darkframe_fits(dark, geom->width, geom->height, geom->bpp)) {
        set_error("flat_apply: %dx%d at %d bits is not the dark frame's geometry", geom->width, geom->height, geom->bpp);
        return MLVFS_AMD_ERR_ARG;
    }
    return apply_dev("flat_apply", dark, flat, geom, d_frames, stride, nframes, stream);
}

}  // extern "C"

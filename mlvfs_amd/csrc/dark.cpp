// dark.cpp -- dark frames: the handle (a host plane, uploaded once per device), the mean of a clip's frames summed on the GPU in
// batches, and the in-place subtraction on device frames (k_dark.hip).
//
//     out     = clamp(px - dark + black_d, 0, 2^bpp - 1)          black_d: the black level of the clip the plane was averaged from
//     dark[p] = (sum over n frames of px_f[p] + n / 2) / n        1 <= n <= 65536
// The plane is applied by position in the stored frame (xRes x yRes): panPosX/Y and cropPosX/Y are ignored.  The reference has no
// such stage.  The mount (mount.cpp) and the transcoder (mlvwriter.cpp) hand the handle's device plane to the reader's load
// (mlvreader.cpp: reader_load_list), which subtracts as stage 0.
//
// mlvfs_amd_dark_create / _info / _plane / _destroy and every argument check are host code: no HIP device is needed for them.
#include "clip.h"

#include <map>

using namespace mlv;

struct mlvfs_amd_dark {
    int w = 0, h = 0, bpp = 0, black = 0;
    int averaged = 0;                                   // frames the plane is the mean of; 0: given to mlvfs_amd_dark_create
    std::vector<uint16_t> plane;
    // the handle is const to its users: the per-device copies appear behind this mutex, on a device's first use
    mutable std::mutex mu;
    mutable std::map<int, void *> on_dev;
};

namespace {

size_t up256(size_t b) { return (b + 255) / 256 * 256; }

int mean_of_clip(const void *reader, int first, int count, int batch, int io_threads, mlvfs_amd_dark &d)
{
    const uint32_t npix = (uint32_t)d.w * (uint32_t)d.h;
    LibcRandGuard rand_guard;                           // HIP code runs: the caller's rand() stream stays out of its reach
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    hipStream_t s = c->stream;
    DevBuf mean;
    MLV_HIP(hipMalloc(&mean.p, (size_t)npix * 2));
    const int rc = clip_mean_dev(reader, first, count, d.w, d.h, d.bpp, batch, io_threads, (uint16_t *)mean.p, s);
    if (rc != MLVFS_AMD_OK) return rc;
    d.plane.resize(npix);
    MLV_HIP(hipMemcpyAsync(d.plane.data(), mean.p, (size_t)npix * 2, hipMemcpyDeviceToHost, s));
    MLV_HIP(hipStreamSynchronize(s));
    return MLVFS_AMD_OK;
}

}  // namespace

bool mlv::plane_geometry_ok(const char *who, int w, int h, int bpp, int black)
{
    if (w <= 0 || h <= 0 || (uint64_t)w * h >= (1u << 27)) { set_error("%s: %dx%d not supported", who, w, h); return false; }
    if (bpp < 1 || bpp > 16) { set_error("%s: unsupported bits_per_pixel %d", who, bpp); return false; }
    if (black < 0 || black > 65535) { set_error("%s: pedestal %d outside 0..65535", who, black); return false; }
    return true;
}

bool mlv::clip_mean_geometry(const char *who, const void *reader, int first, int count, int *w, int *h, int *bpp, int *black)
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
            *w = fw; *h = fhh; *bpp = fb; *black = fh.rawi_hdr.raw_info.black_level;
        } else if (fw != *w || fhh != *h || fb != *bpp) {
            set_error("%s: frames of more than one geometry (frame %d)", who, first + k);
            return false;
        }
    }
    return true;
}

int mlv::clip_mean_dev(const void *reader, int first, int count, int w, int h, int bpp, int batch, int io_threads, uint16_t *d_mean, hipStream_t s)
{
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    const size_t dstride = up256((size_t)npix * 2);
    DevBuf frames, sums;
    MLV_HIP(hipMalloc(&frames.p, dstride * (size_t)batch));
    MLV_HIP(hipMalloc(&sums.p, (size_t)npix * 4));
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
        rc = reader_load_batch(reader, first + f0, n, w, h, bpp, frames.p, dstride, io_threads, s);
        if (rc == MLVFS_AMD_OK) rc = launch_dark_accum(frames.p, dstride, npix, n, (uint32_t *)sums.p, s);
    }
    if (rc == MLVFS_AMD_OK) rc = launch_dark_mean((const uint32_t *)sums.p, d_mean, npix, (uint32_t)count, s);
    (void)hipStreamSynchronize(s);                      // frames and sums go away here
    return rc;
}

bool mlv::darkframe_fits(const mlvfs_amd_dark_t *dark, int w, int h, int bpp) { return dark->w == w && dark->h == h && dark->bpp == bpp; }

int mlv::darkframe_on_device(const mlvfs_amd_dark_t *dark, ThreadCtx *c, int w, int h, int bpp, DarkFrameDev *out)
{
    if (!darkframe_fits(dark, w, h, bpp)) {
        set_error("dark: the dark frame is %dx%d at %d bits, the frames are %dx%d at %d bits", dark->w, dark->h, dark->bpp, w, h, bpp);
        return MLVFS_AMD_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(dark->mu);
    void *&p = dark->on_dev[c->dev->id];
    if (!p) {
        void *fresh = nullptr;
        MLV_HIP(hipMalloc(&fresh, dark->plane.size() * 2));
        const hipError_t e = hipMemcpy(fresh, dark->plane.data(), dark->plane.size() * 2, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(fresh);
            set_error("dark: uploading the plane -> %s", hipGetErrorString(e));
            return MLVFS_AMD_ERR_HIP;
        }
        p = fresh;
    }
    *out = DarkFrameDev{ (const uint16_t *)p, dark->black, (1 << dark->bpp) - 1 };
    return MLVFS_AMD_OK;
}

extern "C" {

mlvfs_amd_dark_t *mlvfs_amd_dark_create(const mlvfs_amd_geom_t *geom, const uint16_t *h_plane)
{
    if (!geom || !h_plane) { set_error("dark_create: null argument"); return nullptr; }
    if (!plane_geometry_ok("dark_create", geom->width, geom->height, geom->bpp, geom->black)) return nullptr;
    try {
        std::unique_ptr<mlvfs_amd_dark> d(new mlvfs_amd_dark);
        d->w = geom->width; d->h = geom->height; d->bpp = geom->bpp; d->black = geom->black;
        d->plane.assign(h_plane, h_plane + (size_t)d->w * d->h);
        return d.release();
    } catch (const std::exception &e) { set_error("dark_create: %s", e.what()); return nullptr; }
}

mlvfs_amd_dark_t *mlvfs_amd_dark_from_clip(const void *reader, int first, int count, int batch_frames, int io_threads)
{
    if (!reader) { set_error("dark_from_clip: null argument"); return nullptr; }
    try {
        std::unique_ptr<mlvfs_amd_dark> d(new mlvfs_amd_dark);
        if (!clip_mean_geometry("dark_from_clip", reader, first, count, &d->w, &d->h, &d->bpp, &d->black)) return nullptr;
        d->averaged = count;
        const int batch = std::min(batch_frames <= 0 ? 8 : batch_frames, count);
        if (mean_of_clip(reader, first, count, batch, io_threads, *d) != MLVFS_AMD_OK) return nullptr;
        return d.release();
    } catch (const std::exception &e) { set_error("dark_from_clip: %s", e.what()); return nullptr; }
}

int mlvfs_amd_dark_info(const mlvfs_amd_dark_t *dark, mlvfs_amd_geom_t *geom, int *frames_averaged)
{
    if (!dark) { set_error("dark_info: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (geom) *geom = mlvfs_amd_geom_t{ dark->w, dark->h, dark->bpp, dark->black, 0, 0, 0 };
    if (frames_averaged) *frames_averaged = dark->averaged;
    return MLVFS_AMD_OK;
}

int mlvfs_amd_dark_plane(const mlvfs_amd_dark_t *dark, uint16_t *h_plane, size_t cap_pixels)
{
    if (!dark || !h_plane) { set_error("dark_plane: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (cap_pixels < dark->plane.size()) { set_error("dark_plane: room for %zu pixels, the plane has %zu", cap_pixels, dark->plane.size()); return MLVFS_AMD_ERR_ARG; }
    std::copy(dark->plane.begin(), dark->plane.end(), h_plane);
    return MLVFS_AMD_OK;
}

void mlvfs_amd_dark_destroy(mlvfs_amd_dark_t *dark)
{
    if (!dark) return;
    for (auto &kv : dark->on_dev) if (kv.second) (void)hipFree(kv.second);
    delete dark;
}

int mlvfs_amd_dark_subtract_dev(const mlvfs_amd_dark_t *dark, const mlvfs_amd_geom_t *geom, void *d_frames, size_t stride, int nframes,
                                void *stream)
{
    if (!dark || !geom || !d_frames) { set_error("dark_subtract: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("dark_subtract: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    if (!darkframe_fits(dark, geom->width, geom->height, geom->bpp)) {
        set_error("dark_subtract: the dark frame is %dx%d at %d bits, the frames are %dx%d at %d bits", dark->w, dark->h, dark->bpp, geom->width,
                  geom->height, geom->bpp);
        return MLVFS_AMD_ERR_ARG;
    }
    const size_t img = dark->plane.size() * 2;
    if (((uintptr_t)d_frames & 1) || (nframes > 1 && (stride < img || (stride & 1)))) {
        set_error("dark_subtract: frames at an odd address, or stride %zu too small or odd", stride);
        return MLVFS_AMD_ERR_ARG;
    }
    if (nframes == 0) return MLVFS_AMD_OK;
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    DarkFrameDev dd;
    if (int rc = darkframe_on_device(dark, c, geom->width, geom->height, geom->bpp, &dd)) return rc;
    return launch_dark_sub(d_frames, stride, (uint32_t)dark->plane.size(), nframes, dd, pick_stream(stream, c));
}

}  // extern "C"

// flat.cpp -- flat fields: the handle (a Q14 gain plane on the host, uploaded once per device), the gain plane of a plane given on the
// host or of the mean of a clip's frames on the GPU, and the in-place correction of device frames (k_flat.hip).
//
//     s[p]    = max(F[p] - black_f, 1)          black_f: the black level of the clip the flat plane F was averaged from
//     M_c     = (sum of s[p] over channel c + n_c / 2) / n_c          c = (y & 1) * 2 + (x & 1); 64-bit sums
//     gain[p] = min((M_c * 16384 + s[p] / 2) / s[p], 65535)           Q14: gains stop just under 4.0
//     out     = clamp(black + floor(((px - black) * gain[p] + 8192) / 16384), 0, 2^bpp - 1)       the frame's own black and bpp
// The plane is applied by position in the stored frame (xRes x yRes): panPosX/Y and cropPosX/Y are ignored.  The reference has no
// such stage.  The mount (mount.cpp) and the transcoder (mlvwriter.cpp) hand the handle's device plane to the reader's load
// (mlvreader.cpp: reader_load_list), which corrects as stage 0b, directly after the dark frame.
//
// mlvfs_amd_flat_create / _info / _gain / _destroy and every argument check are host code: no HIP device is needed for them.
#include "clip.h"

#include <cstring>
#include <map>

using namespace mlv;

struct mlvfs_amd_flat {
    int w = 0, h = 0, bpp = 0, black = 0;              // of the flat plane; the gain plane itself has no depth
    int averaged = 0;                                   // frames the flat plane is the mean of; 0: given to mlvfs_amd_flat_create
    uint32_t mean[4] = { 0, 0, 0, 0 };                  // M_c; 0 for a channel without pixels
    std::vector<uint16_t> gain;
    // the handle is const to its users: the per-device copies appear behind this mutex, on a device's first use
    mutable std::mutex mu;
    mutable std::map<int, void *> on_dev;
};

namespace {

uint32_t signal_of(uint16_t f, int black_f) { return (uint32_t)std::max((int)f - black_f, 1); }

// the definition, on the host: what k_flat_chan_sums and k_flat_gain compute
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
    f.gain.resize(w * h);
    for (size_t y = 0; y < h; y++)
        for (size_t x = 0; x < w; x++) {
            const uint32_t s = signal_of(plane[y * w + x], f.black), m = f.mean[(y & 1) * 2 + (x & 1)];
            f.gain[y * w + x] = (uint16_t)std::min<uint32_t>((m * 16384u + s / 2) / s, 65535u);
        }
}

// the mean of the clip's frames, the dark frame subtracted from it, the two gain kernels, one download: gain plane and means together
int gains_of_clip(const void *reader, int first, int count, const mlvfs_amd_dark_t *dark, int batch, int io_threads, mlvfs_amd_flat &f)
{
    const uint32_t npix = (uint32_t)f.w * (uint32_t)f.h;
    const size_t gain_bytes = ((size_t)npix * 2 + 15) / 16 * 16;
    LibcRandGuard rand_guard;                           // HIP code runs: the caller's rand() stream stays out of its reach
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    hipStream_t s = c->stream;
    DarkFrameDev dd{};
    if (dark) if (int rc = darkframe_on_device(dark, c, f.w, f.h, f.bpp, &dd)) return rc;
    DevBuf mean, out, sums;                             // out: [the gain plane][M_c[4]]
    MLV_HIP(hipMalloc(&mean.p, gain_bytes));
    MLV_HIP(hipMalloc(&out.p, gain_bytes + 16));
    MLV_HIP(hipMalloc(&sums.p, 4 * sizeof(unsigned long long)));
    int rc = clip_mean_dev(reader, first, count, f.w, f.h, f.bpp, batch, io_threads, (uint16_t *)mean.p, s);
    if (rc == MLVFS_AMD_OK && dark) rc = launch_dark_sub(mean.p, 0, npix, 1, dd, s);
    if (rc == MLVFS_AMD_OK)
        rc = launch_flat_gain((const uint16_t *)mean.p, (uint32_t)f.w, (uint32_t)f.h, f.black, (unsigned long long *)sums.p, (uint16_t *)out.p,
                              (uint32_t *)((uint8_t *)out.p + gain_bytes), s);
    if (rc != MLVFS_AMD_OK) { (void)hipStreamSynchronize(s); return rc; }
    std::vector<uint8_t> host(gain_bytes + 16);
    MLV_HIP(hipMemcpyAsync(host.data(), out.p, host.size(), hipMemcpyDeviceToHost, s));
    MLV_HIP(hipStreamSynchronize(s));
    f.gain.resize(npix);
    memcpy(f.gain.data(), host.data(), (size_t)npix * 2);
    memcpy(f.mean, host.data() + gain_bytes, sizeof f.mean);
    return MLVFS_AMD_OK;
}

}  // namespace

bool mlv::flatfield_fits(const mlvfs_amd_flat_t *flat, int w, int h) { return flat->w == w && flat->h == h; }

int mlv::flatfield_on_device(const mlvfs_amd_flat_t *flat, ThreadCtx *c, int w, int h, const uint16_t **d_gain)
{
    if (!flatfield_fits(flat, w, h)) {
        set_error("flat: the flat field is %dx%d, the frames are %dx%d", flat->w, flat->h, w, h);
        return MLVFS_AMD_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(flat->mu);
    void *&p = flat->on_dev[c->dev->id];
    if (!p) {
        void *fresh = nullptr;
        MLV_HIP(hipMalloc(&fresh, flat->gain.size() * 2));
        const hipError_t e = hipMemcpy(fresh, flat->gain.data(), flat->gain.size() * 2, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(fresh);
            set_error("flat: uploading the gain plane -> %s", hipGetErrorString(e));
            return MLVFS_AMD_ERR_HIP;
        }
        p = fresh;
    }
    *d_gain = (const uint16_t *)p;
    return MLVFS_AMD_OK;
}

extern "C" {

mlvfs_amd_flat_t *mlvfs_amd_flat_create(const mlvfs_amd_geom_t *geom, const uint16_t *h_plane)
{
    if (!geom || !h_plane) { set_error("flat_create: null argument"); return nullptr; }
    if (!plane_geometry_ok("flat_create", geom->width, geom->height, geom->bpp, geom->black)) return nullptr;
    try {
        std::unique_ptr<mlvfs_amd_flat> f(new mlvfs_amd_flat);
        f->w = geom->width; f->h = geom->height; f->bpp = geom->bpp; f->black = geom->black;
        gains_on_host(*f, h_plane);
        return f.release();
    } catch (const std::exception &e) { set_error("flat_create: %s", e.what()); return nullptr; }
}

mlvfs_amd_flat_t *mlvfs_amd_flat_from_clip(const void *reader, int first, int count, const mlvfs_amd_dark_t *dark, int batch_frames,
                                           int io_threads)
{
    if (!reader) { set_error("flat_from_clip: null argument"); return nullptr; }
    try {
        std::unique_ptr<mlvfs_amd_flat> f(new mlvfs_amd_flat);
        if (!clip_mean_geometry("flat_from_clip", reader, first, count, &f->w, &f->h, &f->bpp, &f->black)) return nullptr;
        if (dark && !darkframe_fits(dark, f->w, f->h, f->bpp)) {
            set_error("flat_from_clip: %dx%d at %d bits is not the dark frame's geometry", f->w, f->h, f->bpp);
            return nullptr;
        }
        f->averaged = count;
        const int batch = std::min(batch_frames <= 0 ? 8 : batch_frames, count);
        if (gains_of_clip(reader, first, count, dark, batch, io_threads, *f) != MLVFS_AMD_OK) return nullptr;
        return f.release();
    } catch (const std::exception &e) { set_error("flat_from_clip: %s", e.what()); return nullptr; }
}

int mlvfs_amd_flat_info(const mlvfs_amd_flat_t *flat, mlvfs_amd_geom_t *geom, int *frames_averaged, uint32_t means[4])
{
    if (!flat) { set_error("flat_info: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (geom) *geom = mlvfs_amd_geom_t{ flat->w, flat->h, flat->bpp, flat->black, 0, 0, 0 };
    if (frames_averaged) *frames_averaged = flat->averaged;
    if (means) std::copy(flat->mean, flat->mean + 4, means);
    return MLVFS_AMD_OK;
}

int mlvfs_amd_flat_gain(const mlvfs_amd_flat_t *flat, uint16_t *h_gain, size_t cap_pixels)
{
    if (!flat || !h_gain) { set_error("flat_gain: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (cap_pixels < flat->gain.size()) { set_error("flat_gain: room for %zu pixels, the plane has %zu", cap_pixels, flat->gain.size()); return MLVFS_AMD_ERR_ARG; }
    std::copy(flat->gain.begin(), flat->gain.end(), h_gain);
    return MLVFS_AMD_OK;
}

void mlvfs_amd_flat_destroy(mlvfs_amd_flat_t *flat)
{
    if (!flat) return;
    for (auto &kv : flat->on_dev) if (kv.second) (void)hipFree(kv.second);
    delete flat;
}

int mlvfs_amd_flat_apply_dev(const mlvfs_amd_flat_t *flat, const mlvfs_amd_dark_t *dark, const mlvfs_amd_geom_t *geom, void *d_frames,
                             size_t stride, int nframes, void *stream)
{
    if (!flat || !geom || !d_frames) { set_error("flat_apply: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("flat_apply: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    if (!plane_geometry_ok("flat_apply", geom->width, geom->height, geom->bpp, geom->black)) return MLVFS_AMD_ERR_ARG;
    if (!flatfield_fits(flat, geom->width, geom->height)) {
        set_error("flat_apply: the flat field is %dx%d, the frames are %dx%d", flat->w, flat->h, geom->width, geom->height);
        return MLVFS_AMD_ERR_ARG;
    }
    if (dark && !darkframe_fits(dark, geom->width, geom->height, geom->bpp)) {
        set_error("flat_apply: %dx%d at %d bits is not the dark frame's geometry", geom->width, geom->height, geom->bpp);
        return MLVFS_AMD_ERR_ARG;
    }
    const size_t img = flat->gain.size() * 2;
    if (((uintptr_t)d_frames & 1) || (nframes > 1 && (stride < img || (stride & 1)))) {
        set_error("flat_apply: frames at an odd address, or stride %zu too small or odd", stride);
        return MLVFS_AMD_ERR_ARG;
    }
    if (nframes == 0) return MLVFS_AMD_OK;
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    FlatFieldDev fd{ nullptr, geom->black, (1 << geom->bpp) - 1 };
    if (int rc = flatfield_on_device(flat, c, geom->width, geom->height, &fd.d_gain)) return rc;
    DarkFrameDev dd{};
    if (dark) if (int rc = darkframe_on_device(dark, c, geom->width, geom->height, geom->bpp, &dd)) return rc;
    return launch_flat_apply(d_frames, stride, (uint32_t)flat->gain.size(), nframes, fd, dark ? &dd : nullptr, pick_stream(stream, c));
}

}  // extern "C"

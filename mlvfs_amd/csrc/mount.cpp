// mount.cpp -- a clip served as MLVFS serves it: process_frame (mlvfs/main.c:908-1005) and the two dng_get_header_data calls of it,
// batch by batch, for every mount option that shapes a frame's .dng file -- and, behind the last of those stages, what MLVFS does not
// serve: the frames losslessly compressed, binned to proxies, or rendered to TIFF and JPEG files.
//
// The file holds the handle, its setters and size calls, and one path for every serving call: an exported call states what it asks for
// (Serve), mount_serve checks it and settles under the handle's lock what the handle decides -- for a rendering its route (mount_route:
// the size kind of the call and the handle's two demosaic settings) and from the route's geometry the size that comes out, once --,
// and serve_batch runs the stages and hands the final frames to the plain copy, fetch_lossless or fetch_rgb.  What a route takes, how it
// words a refusal and which launcher it has is render_route.h's; the device entry points that render without a mount are there too.
//
// Per batch, in main.c's order: read + decode / unpack (the reader's staging, mlvreader.cpp; with a dark frame or a flat field set -- which main.c does
// not know -- the subtraction, stage 0, and the gain, stage 0b, in the same load: k_cal.hip), deflicker (one histogram launch, one
// median launch, log2 on the host), the frame's header, pattern noise (12 launches per sub-batch), dual ISO (the batched preview,
// or the batched full conversion), then per frame the route main.c takes: a converted frame gets the header again (x4 levels) and
// chroma smoothing (preview only) + stripes; any other frame focus pixels, bad pixels, chroma smoothing (not under dual_iso = 2),
// stripes.  Chroma smoothing and stripes run as the fused pass over runs of consecutive frames of one route and level set.
//
// Order-dependent state, as a fresh process builds it from the frames it serves in order:
//   stripes       one correction per mount, from the first frame that reaches the stage (stripes.c:31-69, main.c:979-993)
//   bad pixels    the process's map per clip GUID (dropin.cpp, cs.c:233-312), detected by the first frame that reaches a repair; under
//                 dual_iso = 2 a converted frame repairs inside the conversion, so until the map exists frames are served one by one
//   dual ISO      the table caches of dualiso.cpp (process-wide), filled by the first frame that converts
//
// mlvfs_amd_mount_dng_lossless serves the same frames through the same stages; only the last step differs: the batch's final frames
// are encoded where they lie (lje_encode_batch, k_lj92enc.hip) and their streams, not their pixels, cross the link.
//
// mlvfs_amd_mount_set_proxy(2): one stage more behind the last, the 2x2 binning within each CFA colour (k_proxy.hip).  Each final frame
// is binned into its other slot (O when it lies in F, and the reverse -- free by then); the download, the encoder and the headers take
// the binned frame and its geometry.  Nothing in front of it knows.
//
// mlvfs_amd_mount_rgb serves the same frames through the same stages as TIFF files of 8-bit sRGB at half size: each final frame is
// developed into its other slot (k_render.hip) with the parameters its headers give in their final state (mlvfs_amd_rgb_params), and
// only the 3 W' H' bytes cross the link.  No .dng header is written on that route; nothing in front of the last step knows.
//
// mlvfs_amd_mount_jpeg renders in the same way and then encodes each rendering where it lies (jpg_encode_batch, k_jpeg.hip): the stream
// goes into the slot the frame was developed from, which is free by then, and only the stream crosses the link.  A file that would be
// larger than the TIFF is served as the TIFF.
//
// mlvfs_amd_mount_rgb_full and mlvfs_amd_mount_jpeg_full are the same two routes at the frame's own size: each final frame is demosaiced
// (k_demosaic.hip, the same parameters) into a buffer of its own, d_full -- 3 W H bytes do not fit the frame's other slot --, and a
// JPEG call's streams lie in that buffer behind the batch's renderings.  A handle that never makes a full-size call never allocates it.
//
// mlvfs_amd_mount_rgb_scaled and mlvfs_amd_mount_jpeg_scaled are the half-size routes at ow x oh, at most the half size: each final frame
// is balanced, area-averaged and developed in one pass (k_scale.hip, the same parameters) into its other slot, exactly where the
// half-size rendering would lie, and only 3 ow oh bytes or the stream cross the link.  Nothing is allocated for it.
//
// mlvfs_amd_mount_rgb_resampled and mlvfs_amd_mount_jpeg_resampled serve ow x oh up to the frame's own size: each final frame is demosaiced,
// area-averaged and developed in one pass (k_resample.hip, the same parameters).  Such a rendering can exceed the frame's other slot, so
// it goes into d_full as the full-size ones do, sized for ow x oh.
//
// mlvfs_amd_mount_set_demosaic(1): the three full-size calls demosaic with AMaZE (amaze_render.cpp: balance, amaze_launch, tone, in the
// calling thread's work memory) instead of k_demosaic.hip's linear filter; the renderings lie in d_full as before and everything behind
// them -- the JPEG encoder, the headers, the copies -- is the same.  No other call knows.
//
// mlvfs_amd_mount_set_resample_demosaic(1): the three resampled calls render through balance, amaze_launch and the resampling pass behind
// it (amaze_render.cpp, k_amaze_resample.hip) instead of k_resample.hip, whatever set_demosaic says; placement, growth and everything
// behind the renderings are the resampled route's.  At 0 (the default) the resampled calls are what they were, refused under set_demosaic(1).
//
// mlvfs_amd_mount_tensor leaves the frame where it lies: the same stages and, for an RGB tensor, the same rendering in the same place,
// then one launch of the tensor pass (k_tensor.hip) per run of frames into the caller's device memory in the place of the downloads; a
// Bayer tensor is read from the final frames.  No header is written, nothing crosses the link, and no other call knows.
#include "fused_pass.h"
#include "lj92enc.h"
#include "jpeg.h"
#include "render_route.h"
#include "tensor.h"

#include <cstring>
#include <string>
#include <vector>

using namespace mlv;

namespace {

struct Mount {
    const void *reader = nullptr;
    mlvfs_amd_mount_opts_t o{};
    std::vector<char> basename;              // dng_get_header_data takes a char *
    std::mutex mu;
    bool stripes_known = false;              // stripes_get_correction(mlv_filename) != NULL
    int stripes_needed = 0;
    int32_t coef[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    const mlvfs_amd_dark_t *dark = nullptr;  // stage 0 (mlvfs_amd_mount_set_dark): subtracted inside the reader's load
    const mlvfs_amd_flat_t *flat = nullptr;  // stage 0b (mlvfs_amd_mount_set_flat): the gain, in the same pass of the load
    const mlvfs_amd_look_t *look = nullptr;  // step 4 of every rendering (mlvfs_amd_mount_set_look); no serve-order state: it may change between calls
    bool served = false;                     // a call has reached the device: the dark frame, the flat field and the proxy stay what they are
    int proxy = 1;                           // mlvfs_amd_mount_set_proxy: 2 = the served frames are binned to half size
    int demosaic = 0;                        // mlvfs_amd_mount_set_demosaic: 1 = the full-size calls demosaic with AMaZE; no serve-order state
    int resample_demosaic = 0;               // mlvfs_amd_mount_set_resample_demosaic: 1 = the resampled calls demosaic with AMaZE; no serve-order state
    int jpeg_sampling = MLVFS_AMD_JPEG_420;  // mlvfs_amd_mount_set_jpeg_sampling: the chroma sampling of every JPEG call; no serve-order state
    int device = -1;
    DevBuf d_frames, d_out, d_scratch;
    DevBuf d_bits;                           // the encoder's bit streams, sized from a batch's histograms
    DevBuf d_rgb;                            // mlvfs_amd_mount_rgb: RGB_PARAMS int32 per frame of a batch
    std::vector<int32_t> rgb_host;           // what the upload reads: it outlives every call
    DevBuf d_full;                           // the full-size calls: a batch's renderings of 3 W H bytes (6 W H once a 16-bit call needs
                                             // them), a JPEG call's streams behind them

    void release() { for (DevBuf *b : { &d_frames, &d_out, &d_scratch, &d_bits, &d_rgb, &d_full }) b->release(); }

    int ensure(int dev, size_t fbytes, size_t sbytes)
    {
        if (dev != device) { release(); device = dev; }
        for (DevBuf *b : { &d_frames, &d_out })
            if (const int rc = b->reserve(fbytes)) return rc;
        return d_scratch.reserve(sbytes);
    }
    // after ensure(): the device is this handle's
    int ensure_rgb(int frames) { return d_rgb.reserve((size_t)frames * RGB_PARAMS * sizeof(int32_t)); }
};

// what a serving call asks for, beyond its frames and its room.  mount_serve fills in what the handle decides (the route's demosaic,
// the chroma sampling) and the size of a rendering, once; a batch gets a copy whose sizes and flags begin at its own frame 0
struct Serve {
    bool lossless = false;                   // mlvfs_amd_mount_dng_lossless: sizes and flags are the encoder's answers
    int gain_q8 = 0;                         // != 0: served rendered, and no .dng header is written -- a file may be smaller than one
    int quality = 0;                         // != 0: as JPEG files; sizes and flags are that encoder's answers
    RenderRoute route{};                     // which rendering
    const mlvfs_amd_look16_t *deep = nullptr;    // as 16-bit TIFF files through this deep look (never m.look, never JPEG)
    size_t *sizes = nullptr;
    int *flags = nullptr;
    int sampling = MLVFS_AMD_JPEG_420;       // the handle's, as the call found it
    const mlvfs_amd_tensor_spec_t *tensor = nullptr;     // mlvfs_amd_mount_tensor: h_out is the caller's device memory, no file is written
    int pw = 0, ph = 0;                      // the rendering's size

    bool in_full() const { return route.size == RenderRoute::FULL || route.size == RenderRoute::RESAMPLED; }     // the renderings lie in d_full
    size_t bpx() const { return deep ? 6 : 3; }
    Serve from(int f0) const
    {
        Serve b = *this;
        if (sizes) { b.sizes += f0; b.flags += f0; }
        return b;
    }
};

// the encoder's room in a mount: the bit streams in a buffer of their own that grows with what a batch needs, the streams
// (one frame stride each) behind the encoder's fixed scratch in d_scratch
struct MountRoom : LjeRoom {
    Mount &m;
    explicit MountRoom(Mount &m_) : m(m_) {}
    int get(size_t bits_bytes, size_t, void **d_bits, uint8_t **, size_t *) override
    {
        if (const int rc = m.d_bits.reserve(bits_bytes)) return rc;
        *d_bits = m.d_bits;
        return MLVFS_AMD_OK;
    }
};

bool same_levels(const frame_headers &a, const frame_headers &b)
{
    return a.rawi_hdr.raw_info.black_level == b.rawi_hdr.raw_info.black_level && a.rawi_hdr.raw_info.white_level == b.rawi_hdr.raw_info.white_level;
}

// pattern-noise scratch of a batch: whole frames, at most pattern_noise_scratch_cap() (sub-batches beyond that)
size_t o_pn_bytes(const mlvfs_amd_mount_opts_t &o, int w, int h, int batch)
{
    if (!o.fix_pattern_noise) return 0;
    const size_t per = pattern_noise_batch_frame_bytes(w, h);
    return per * std::max<size_t>(1, std::min<size_t>((size_t)batch, pattern_noise_scratch_cap() / per));
}

// The batch's final frames as lossless-JPEG streams: encoded where they lie, one copy of lengths and states, then the streams.
// hdr_max[k]: the max_size the frame's header was last written with.  A frame that is not to be served compressed gets its pixels.
// w x h: the frames at final_at as they are served -- the clip's size, or with a proxy set the binned one
int fetch_lossless(Mount &m, ThreadCtx *c, frame_headers *fh, int n, size_t dstride, const std::vector<uint8_t *> &final_at,
                   const std::vector<size_t> &hdr_max, uint8_t *h_out, size_t out_stride, const Serve &ll, int w, int h)
{
    hipStream_t s = c->stream;
    const size_t img = (size_t)w * h * 2, hdr = dng_get_header_size();
    const bool pairs = !(h & 1);                                       // 2w x h/2: the row above is the same colour
    const int jw = pairs ? 2 * w : w, jh = pairs ? h / 2 : h;
    std::vector<LjeResult> res(n);
    const size_t cap = img / 4 * 4;                                    // a stream longer than the pixels is not worth serving
    bool encode = jw <= 65535 && jh <= 65535 && (uint64_t)w * h < (1u << 27) && cap >= 128;
    uint8_t *d_streams = (uint8_t *)m.d_scratch + lje_fixed_bytes((uint32_t)(img / 2), n);
    if (encode) {
        std::vector<const uint16_t *> src(n);
        for (int k = 0; k < n; k++) src[k] = (const uint16_t *)final_at[k];
        MountRoom room(m);
        size_t stream_stride = dstride;
        const int rc = lje_encode_batch(src.data(), n, jw, jh, 16, nullptr, 0, m.d_scratch, room, &d_streams, &stream_stride, res.data(), s);
        if (rc) return rc;
    }
    for (int k = 0; k < n; k++) {
        uint8_t *file = h_out + k * out_stride;
        const bool plain = !encode || res[k].status != LJE_OK || res[k].max_class >= 16 || res[k].length > cap;
        ll.flags[k] = plain ? 1 : 0;
        if (plain) {
            ll.sizes[k] = hdr + img;
            MLV_HIP(hipMemcpyAsync(file + hdr, final_at[k], img, hipMemcpyDeviceToHost, s));
            continue;
        }
        ll.sizes[k] = hdr + res[k].length;
        if (m.proxy == 2) (void)mlvfs_amd_dng_header_proxy(&fh[k], file, 0, hdr_max[k], m.o.fps, m.basename.data(), 2, res[k].length);
        else (void)mlvfs_amd_dng_header_lossless(&fh[k], file, 0, hdr_max[k], m.o.fps, m.basename.data(), res[k].length);
        MLV_HIP(hipMemcpyAsync(file + hdr, d_streams + k * dstride, res[k].length, hipMemcpyDeviceToHost, s));
    }
    MLV_HIP(hipStreamSynchronize(s));
    return MLVFS_AMD_OK;
}

// the route a call of size kind `size` takes on a handle with these two demosaic settings, and the only place that knows how they
// apply: set_demosaic's AMaZE is for the full-size calls, the resampled calls have set_resample_demosaic's own, the others neither.
// *unserved (where asked for): AMaZE is set for the full-size calls alone, which leaves the resampled calls refused
RenderRoute mount_route(RenderRoute::Size size, int ow, int oh, int demosaic, int resample_demosaic, bool *unserved = nullptr)
{
    const bool resampled = size == RenderRoute::RESAMPLED;
    if (unserved) *unserved = resampled && demosaic == 1 && resample_demosaic != 1;
    return { size, resampled ? resample_demosaic == 1 : size == RenderRoute::FULL && demosaic == 1, ow, oh };
}

// what the encoder's row buffer has to hold for streams of at most `room` bytes: the rows unstuffed, each begun on a dword
size_t jpg_rowcap(size_t room, int ph, int sampling) { return room + 4 * (((size_t)ph + kJpgModes[sampling].mch - 1) / kJpgModes[sampling].mch) + 4; }
// the stream's room in a JPEG file that is to be no larger than the TIFF (0: there is none)
size_t jpg_room(int pw, int ph)
{
    const size_t tiff = mlvfs_amd_rgb_header_size() + (size_t)3 * pw * ph;
    return tiff > (size_t)JPG_HEADER_BYTES + 2 ? tiff - JPG_HEADER_BYTES : 0;
}

// from one rendering to the next in d_full; bpx: 3 bytes per pixel, or 6 in a 16-bit call
size_t full_stride(int pw, int ph, size_t bpx) { return up256(bpx * pw * ph); }

// The batch's final frames as rendered TIFF files: the parameters of every frame from its headers as they are now, one upload, runs of
// frames that lie on one side of the slot pair developed into the other side in one launch, then header + bpx W' H' bytes per file.
// With a look set (m.look) the launchers take the look kernels; nothing else differs.
// sv.quality: as JPEG files -- the run's renderings encoded into the slots they were developed from, then header + stream per file, or
// the TIFF where that is the smaller file.
// HALF, SCALED: developed into the other slots, which a rendering of at most the half size always fits -- at 6 bytes per pixel too:
// 6 W' H' <= 1.5 W H
// FULL, RESAMPLED: the renderings go into d_full, full_stride(pw, ph) apart, and their streams behind the batch's renderings
int fetch_rgb(Mount &m, ThreadCtx *c, const frame_headers *fh, int n, size_t dstride, const std::vector<uint8_t *> &final_at, uint8_t *h_out,
              size_t out_stride, int w, int h, const Serve &sv)
{
    hipStream_t s = c->stream;
    uint8_t *const F = (uint8_t *)m.d_frames, *const O = (uint8_t *)m.d_out;
    const bool full = sv.in_full(), deep = sv.deep != nullptr;
    const int pw = sv.pw, ph = sv.ph;
    const size_t rstride = full ? full_stride(pw, ph, sv.bpx()) : dstride;              // from one rendering to the next
    const size_t sstride = full ? up256(jpg_room(pw, ph)) : dstride;                    // from one stream to the next
    std::vector<int32_t> &params = m.rgb_host;
    params.resize((size_t)n * RGB_PARAMS);
    for (int k = 0; k < n; k++) {
        const int rc = mlvfs_amd_rgb_params(&fh[k], sv.gain_q8, params.data() + (size_t)k * RGB_PARAMS);
        if (rc) return rc;
    }
    MLV_HIP(hipMemcpyAsync(m.d_rgb, params.data(), params.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    LookArg look;
    if (deep) { if (const int rc = look16_on_device(sv.deep, c, &look)) return rc; }
    else if (m.look) if (const int rc = look_on_device(m.look, c, &look)) return rc;
    const LookArg *lk = deep || m.look ? &look : nullptr;
    const size_t hdr = mlvfs_amd_rgb_header_size(), served = sv.bpx() * pw * ph;
    for (int k0 = 0, k1; k0 < n; k0 = k1) {
        const bool in_f = final_at[k0] == F + k0 * dstride;
        for (k1 = k0 + 1; k1 < n && (final_at[k1] == F + k1 * dstride) == in_f; k1++) {}
        uint8_t *dst = full ? (uint8_t *)m.d_full + k0 * rstride : (in_f ? O : F) + k0 * dstride;
        uint8_t *streams = full ? (uint8_t *)m.d_full + n * rstride + k0 * sstride : final_at[k0];
        const int32_t *par = (const int32_t *)m.d_rgb + (size_t)k0 * RGB_PARAMS;
        const int rc = route_launch(sv.route, c, final_at[k0], dstride, par, dst, rstride, w, h, k1 - k0, s, lk, deep);
        if (rc) return rc;
        if (sv.tensor) {                                               // the rendering stays where it lies: the pass in the place of the downloads
            const int rt = launch_tensor_rgb(dst, rstride, pw, ph, deep ? 16 : 8, sv.tensor->dtype, sv.tensor->layout, tensor_affine(*sv.tensor),
                                             h_out + k0 * out_stride, out_stride, k1 - k0, s);
            if (rt) return rt;
            continue;
        }
        std::vector<JpgOut> res(k1 - k0, JpgOut{ 0, 1 });
        const size_t room = sv.quality ? std::min(jpg_room(pw, ph), sstride) : 0;
        if (room) {
            const JpgLayout l = jpg_layout(pw, ph, jpg_rowcap(room, ph, sv.sampling), sv.sampling);
            const int rj = jpg_encode_batch(dst, rstride, pw, ph, sv.quality, streams, sstride, room, m.d_scratch, l, res.data(), k1 - k0, s, sv.sampling);
            if (rj) return rj;
        }
        for (int k = k0; k < k1; k++) {
            uint8_t *file = h_out + k * out_stride;
            if (sv.quality) {
                const JpgOut &r = res[k - k0];
                sv.flags[k] = r.status ? 1 : 0;
                sv.sizes[k] = r.status ? hdr + served : (size_t)JPG_HEADER_BYTES + r.length;
                if (!r.status) {
                    (void)mlvfs_amd_jpeg_header_sampled(pw, ph, sv.quality, sv.sampling, file, JPG_HEADER_BYTES);
                    MLV_HIP(hipMemcpyAsync(file + JPG_HEADER_BYTES, streams + (size_t)(k - k0) * sstride, r.length, hipMemcpyDeviceToHost, s));
                    continue;
                }
            }
            if (deep) (void)mlvfs_amd_rgb16_header(pw, ph, file, hdr);
            else (void)mlvfs_amd_rgb_header(pw, ph, file, hdr);
            MLV_HIP(hipMemcpyAsync(file + hdr, dst + (size_t)(k - k0) * rstride, served, hipMemcpyDeviceToHost, s));
        }
    }
    MLV_HIP(hipStreamSynchronize(s));
    return MLVFS_AMD_OK;
}

// The batch's final frames as Bayer tensors: black, range and unit of every frame from its headers as they are now, one upload, runs of
// frames that lie on one side of the slot pair in one launch each
int fetch_bayer_tensor(Mount &m, ThreadCtx *c, const frame_headers *fh, int n, size_t dstride, const std::vector<uint8_t *> &final_at, uint8_t *d_out,
                       size_t out_stride, int w, int h, const Serve &sv)
{
    hipStream_t s = c->stream;
    uint8_t *const F = (uint8_t *)m.d_frames;
    std::vector<int32_t> &levels = m.rgb_host;
    levels.resize((size_t)n * TENSOR_LEVELS);
    for (int k = 0; k < n; k++)
        if (const int rc = mlvfs_amd_tensor_bayer_params(&fh[k], levels.data() + (size_t)k * TENSOR_LEVELS)) return rc;
    MLV_HIP(hipMemcpyAsync(m.d_rgb, levels.data(), levels.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    for (int k0 = 0, k1; k0 < n; k0 = k1) {
        const bool in_f = final_at[k0] == F + k0 * dstride;
        for (k1 = k0 + 1; k1 < n && (final_at[k1] == F + k1 * dstride) == in_f; k1++) {}
        const int rc = launch_tensor_bayer(final_at[k0], dstride, w, h, (const int32_t *)m.d_rgb + (size_t)k0 * TENSOR_LEVELS, sv.tensor->dtype,
                                           sv.tensor->layout, tensor_affine(*sv.tensor), d_out + k0 * out_stride, out_stride, k1 - k0, s);
        if (rc) return rc;
    }
    MLV_HIP(hipStreamSynchronize(s));
    return MLVFS_AMD_OK;
}

// frames [f0, f0 + n) of the call, whose headers are fh[0 .. n), already in m.d_frames (frame k at k * dstride); sv: what the call asks
// for, its sizes and flags beginning at this batch
int serve_batch(Mount &m, ThreadCtx *c, frame_headers *fh, int n, size_t dstride, uint8_t *h_out, size_t out_stride, int *results, const Serve &sv)
{
    const mlvfs_amd_mount_opts_t &o = m.o;
    hipStream_t s = c->stream;
    const int w = fh[0].rawi_hdr.xRes, h = fh[0].rawi_hdr.yRes, bpp = fh[0].rawi_hdr.raw_info.bits_per_pixel;
    const size_t img = (size_t)w * h * 2, hdr = dng_get_header_size();
    uint8_t *const F = (uint8_t *)m.d_frames, *const O = (uint8_t *)m.d_out;
    int rc = MLVFS_AMD_OK;
    // deflicker (main.c:943): before the header, which writes exposure_bias as BaselineExposure
    if (o.deflicker) {
        std::vector<uint16_t> med(n);
        rc = deflicker_batch_device(F, dstride, n, bpp, img, m.d_scratch, m.d_scratch.bytes, med.data(), s);
        if (rc) return rc;
        for (int k = 0; k < n; k++) deflicker_bias(o.deflicker, fh[k].rawi_hdr.raw_info.black_level, med[k], fh[k].rawi_hdr.raw_info.exposure_bias);
    }
    // the frame's header: the proxy's where one is served, with the max_size the full-size write has
    auto write_header = [&](int k, size_t max_size) {
        if (sv.gain_q8 || sv.tensor) return;
        if (m.proxy == 2) (void)mlvfs_amd_dng_header_proxy(&fh[k], h_out + k * out_stride, 0, max_size, o.fps, m.basename.data(), 2, 0);
        else (void)dng_get_header_data(&fh[k], h_out + k * out_stride, 0, max_size, o.fps, m.basename.data());
    };
    for (int k = 0; k < n; k++) write_header(k, hdr);                  // main.c:944
    // pattern noise (main.c:946-949): runs of one white level
    if (o.fix_pattern_noise && w >= 2 && h >= 2 && !(w & 1) && !(h & 1)) {
        for (int k0 = 0, k1; k0 < n; k0 = k1) {
            for (k1 = k0 + 1; k1 < n && fh[k1].rawi_hdr.raw_info.white_level == fh[k0].rawi_hdr.raw_info.white_level; k1++) {}
            rc = launch_pattern_noise_batch(F + k0 * dstride, dstride, k1 - k0, w, h, fh[k0].rawi_hdr.raw_info.white_level, m.d_scratch,
                                            m.d_scratch.bytes, s);
            if (rc) return rc;
        }
    }
    // dual ISO (main.c:951-960)
    std::vector<int> conv(n, 0);
    std::vector<size_t> hdr_max(n, hdr);
    if (o.dual_iso == 1) {
        for (int k0 = 0, k1; k0 < n; k0 = k1) {
            for (k1 = k0 + 1; k1 < n && same_levels(fh[k1], fh[k0]); k1++) {}
            const auto &ri = fh[k0].rawi_hdr.raw_info;
            const Geom g{ w, h, bpp, ri.black_level, ri.white_level };
            const size_t hist = up256(4 * (size_t)((uint16_t)g.white + 1) * sizeof(unsigned) * (k1 - k0));
            rc = hdr_preview_batch_device(c, g, F + k0 * dstride, O + k0 * dstride, dstride, k1 - k0, img, (unsigned *)m.d_scratch,
                                          (HdrPreviewParams *)((uint8_t *)m.d_scratch + hist), fh + k0, conv.data() + k0, s);
            if (rc) return rc;
        }
        for (int k = 0; k < n; k++)
            if (conv[k]) MLV_HIP(hipMemcpyAsync(F + k * dstride, O + k * dstride, img, hipMemcpyDeviceToDevice, s));
    } else if (o.dual_iso == 2) {
        // the drop-in's repairs before the conversion (focus map, fix_bad_pixels mode) need the frame's headers: one frame at a time
        bool per_frame = o.fix_bad_pixels != 0;
        for (int k = 0; k < n && !per_frame; k++) per_frame = focus_map_applies(&fh[k], c, 1);
        for (int k0 = 0, k1; k0 < n; k0 = k1) {
            for (k1 = k0 + 1; !per_frame && k1 < n && same_levels(fh[k1], fh[k0]); k1++) {}
            const auto &ri = fh[k0].rawi_hdr.raw_info;
            rc = cr2hdr20_batch_fh(c, per_frame ? &fh[k0] : nullptr, F + k0 * dstride, per_frame ? img : dstride, k1 - k0, w, h, ri.black_level,
                                   ri.white_level, o.hdr_interpolation_method, !o.hdr_no_fullres, !o.hdr_no_alias_map, o.chroma_smooth,
                                   o.fix_bad_pixels, s, conv.data() + k0);
            if (rc < 0) return rc;
            rc = MLVFS_AMD_OK;
        }
    }
    for (int k = 0; k < n; k++) {
        if (results) results[k] = conv[k] == 1;
        if (conv[k] != 1) continue;
        fh[k].rawi_hdr.raw_info.black_level *= 4;                      // hdr.c:223-224, 1951-1952
        fh[k].rawi_hdr.raw_info.white_level *= 4;
        write_header(k, img);                                          // main.c:962-966
        hdr_max[k] = img;
    }
    // frames that were not converted: focus pixels, bad pixels (main.c:967-975), in serve order
    for (int k = 0; k < n; k++) {
        if (conv[k] == 1) continue;
        rc = focus_pixels_device(&fh[k], c, F + k * dstride, 0, nullptr);
        if (!rc && o.fix_bad_pixels) rc = bad_pixels_device(&fh[k], c, F + k * dstride, o.fix_bad_pixels == 2, 0, nullptr);
        if (rc) return rc;
    }
    // chroma smoothing (main.c:977-980) and stripes (main.c:982-995): the fused pass over runs of one route and level set
    std::vector<uint8_t *> final_at(n);
    auto cs_of = [&](int k) {
        const int cs = o.chroma_smooth;
        if (!cs || o.dual_iso == 2) return 0;
        if (cs != 2 && cs != 3 && cs != 5) { fprintf(stderr, "Unsupported chroma smooth method\n"); return 0; }
        if (black_too_large(fh[k].rawi_hdr.raw_info.black_level)) { fprintf(stderr, "Black level too large for processing\n"); return 0; }
        return cs;
    };
    for (int k0 = 0, k1; k0 < n; k0 = k1) {
        const int cs = cs_of(k0);
        for (k1 = k0 + 1; k1 < n && same_levels(fh[k1], fh[k0]) && (conv[k1] == 1) == (conv[k0] == 1) && cs_of(k1) == cs; k1++) {}
        const auto &ri = fh[k0].rawi_hdr.raw_info;
        const Geom g{ w, h, ri.bits_per_pixel, ri.black_level, ri.white_level };
        int a = k0;
        if (o.fix_stripes && !m.stripes_known) {
            // the clip's correction from this frame as it is after chroma smoothing (stripes_compute_correction), then applied to it
            uint8_t *src = F + a * dstride;
            if (cs) {
                rc = run_fused_pass(c->dev, fused_pass_of(g, 0, cs, nullptr, false, 0, nullptr), src, img, O + a * dstride, img, 1, nullptr, s);
                if (rc) return rc;
                src = O + a * dstride;
            }
            Clip cl;
            cl.g = g;
            cl.pan_x = fh[a].vidf_hdr.panPosX;
            cl.pan_y = fh[a].vidf_hdr.panPosY;
            cl.device = c->dev->id;
            rc = cl.stripes_compute(src, ri.frame_size, o.rand_mode ? 1 : 0, s);
            if (rc) return rc;                                     // a library failure: the handle has no correction yet, the call fails
            memcpy(m.coef, cl.coef, sizeof m.coef);
            m.stripes_needed = cl.needed;
            m.stripes_known = true;
            if (stripes_apply_to(true, m.stripes_needed, w)) {
                rc = launch_stripes_apply(src, img, (size_t)w * h, w, g.black, g.white, m.coef, 1, s);
                if (rc) return rc;
            }
            final_at[a] = src;
            a++;
        }
        const FusedPass p = fused_pass_of(g, 0, cs, nullptr, o.fix_stripes, m.stripes_needed, m.coef);     // (no map: the repairs ran above)
        for (int k = a; k < k1; k++) final_at[k] = p.idle() ? F + k * dstride : O + k * dstride;
        if (a < k1 && !p.idle()) {
            rc = run_fused_pass(c->dev, p, F + a * dstride, dstride, O + a * dstride, dstride, k1 - a, nullptr, s);
            if (rc) return rc;
        }
    }
    // the proxy: the last stage, each final frame binned into its other slot, runs of frames that lie on one side in one launch
    int sw = w, sh = h;
    if (m.proxy == 2) {
        if (!proxy_geom(w, h, &sw, &sh)) { set_error("mount: a proxy takes frames of 4x4 and more, not %dx%d", w, h); return MLVFS_AMD_ERR_ARG; }
        for (int k0 = 0, k1; k0 < n; k0 = k1) {
            const bool in_f = final_at[k0] == F + k0 * dstride;
            for (k1 = k0 + 1; k1 < n && (final_at[k1] == F + k1 * dstride) == in_f; k1++) {}
            uint8_t *dst = (in_f ? O : F) + k0 * dstride;
            rc = launch_bin2(final_at[k0], dstride, dst, dstride, w, h, k1 - k0, s);
            if (rc) return rc;
            for (int k = k0; k < k1; k++) final_at[k] = dst + (size_t)(k - k0) * dstride;
        }
    }
    if (sv.gain_q8) return fetch_rgb(m, c, fh, n, dstride, final_at, h_out, out_stride, w, h, sv);
    if (sv.tensor) return fetch_bayer_tensor(m, c, fh, n, dstride, final_at, h_out, out_stride, w, h, sv);
    if (sv.lossless) return fetch_lossless(m, c, fh, n, dstride, final_at, hdr_max, h_out, out_stride, sv, sw, sh);
    const size_t served = (size_t)sw * sh * 2;
    for (int k = 0; k < n; k++) MLV_HIP(hipMemcpyAsync(h_out + k * out_stride + hdr, final_at[k], served, hipMemcpyDeviceToHost, s));
    MLV_HIP(hipStreamSynchronize(s));
    return MLVFS_AMD_OK;
}

// what mlvfs_amd_mount_set_dark, _set_flat and _set_proxy do alike: the handle locked and refused once it has served frames (what:
// "the dark frame"); a setting that is switched on (wanted) checked against frame 0's headers if the clip has frames -- fits(fh):
// false with the error set --; then taken: take(m)
template <class Fits, class Take>
int mount_set(void *mount, const char *what, bool wanted, Fits fits, Take take)
{
    if (!mount) { set_error("mount: null argument"); return MLVFS_AMD_ERR_ARG; }
    Mount &m = *(Mount *)mount;
    std::lock_guard<std::mutex> lk(m.mu);
    if (m.served) { set_error("mount: the handle has served frames already: %s cannot change any more", what); return MLVFS_AMD_ERR_ARG; }
    frame_headers fh;
    if (wanted && mlvfs_amd_mlv_frame_count(m.reader) > 0) {
        if (!mlvfs_amd_mlv_frame_headers(m.reader, 0, &fh)) { set_error("mount: frame 0 has no usable headers"); return MLVFS_AMD_ERR_ARG; }
        if (!fits(fh)) return MLVFS_AMD_ERR_ARG;
    }
    take(m);
    return MLVFS_AMD_OK;
}

}  // namespace

extern "C" {

void *mlvfs_amd_mount_open(const void *reader, const mlvfs_amd_mount_opts_t *opts, const char *mlv_basename)
{
    if (!reader || !opts) { set_error("mount: null argument"); return nullptr; }
    const mlvfs_amd_mount_opts_t &o = *opts;
    if (o.chroma_smooth < 0 || o.fix_bad_pixels < 0 || o.fix_bad_pixels > 2 || o.dual_iso < 0 || o.dual_iso > 2 ||
        o.hdr_interpolation_method < 0 || o.hdr_interpolation_method > 1 || o.deflicker < 0 || o.rand_mode < 0 || o.rand_mode > 1 ||
        !(o.fps >= 0.0)) {
        set_error("mount: option out of range");
        return nullptr;
    }
    Mount *m = new Mount;
    m->reader = reader;
    m->o = o;
    const char *b = mlv_basename ? mlv_basename : "";
    m->basename.assign(b, b + strlen(b) + 1);
    return m;
}

void mlvfs_amd_mount_close(void *mount) { delete (Mount *)mount; }

int mlvfs_amd_mount_set_dark(void *mount, const mlvfs_amd_dark_t *dark)
{
    return mount_set(mount, "the dark frame", dark != nullptr, [&](const frame_headers &fh) {
        if (darkframe_fits(dark, fh.rawi_hdr.xRes, fh.rawi_hdr.yRes, fh.rawi_hdr.raw_info.bits_per_pixel)) return true;
        set_error("mount: the dark frame does not have the clip's geometry (%dx%d at %d bits)", fh.rawi_hdr.xRes, fh.rawi_hdr.yRes,
                  fh.rawi_hdr.raw_info.bits_per_pixel);
        return false;
    }, [&](Mount &m) { m.dark = dark; });
}

int mlvfs_amd_mount_set_flat(void *mount, const mlvfs_amd_flat_t *flat)
{
    return mount_set(mount, "the flat field", flat != nullptr, [&](const frame_headers &fh) {
        if (flatfield_fits(flat, fh.rawi_hdr.xRes, fh.rawi_hdr.yRes)) return true;
        set_error("mount: the flat field does not have the clip's geometry (%dx%d)", fh.rawi_hdr.xRes, fh.rawi_hdr.yRes);
        return false;
    }, [&](Mount &m) { m.flat = flat; });
}

int mlvfs_amd_mount_set_proxy(void *mount, int factor)
{
    if (mount && factor != 1 && factor != 2) { set_error("mount: a proxy factor of %d (1: off, 2: half size)", factor); return MLVFS_AMD_ERR_ARG; }
    return mount_set(mount, "the proxy", factor == 2, [&](const frame_headers &fh) {
        int pw, ph;
        if (proxy_geom(fh.rawi_hdr.xRes, fh.rawi_hdr.yRes, &pw, &ph)) return true;
        set_error("mount: a proxy takes frames of 4x4 and more, not %dx%d", fh.rawi_hdr.xRes, fh.rawi_hdr.yRes);
        return false;
    }, [&](Mount &m) { m.proxy = factor; });
}

int mlvfs_amd_mount_set_look(void *mount, const mlvfs_amd_look_t *look)
{
    if (!mount) { set_error("mount: null argument"); return MLVFS_AMD_ERR_ARG; }
    Mount &m = *(Mount *)mount;
    std::lock_guard<std::mutex> lk(m.mu);                // between serving calls: a call in flight holds the mutex
    m.look = look;
    return MLVFS_AMD_OK;
}

int mlvfs_amd_mount_set_demosaic(void *mount, int which)
{
    if (!mount) { set_error("mount: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (which != 0 && which != 1) { set_error("mount: a demosaic of %d (0: the linear filter, 1: AMaZE)", which); return MLVFS_AMD_ERR_ARG; }
    Mount &m = *(Mount *)mount;
    std::lock_guard<std::mutex> lk(m.mu);                // between serving calls: a call in flight holds the mutex
    m.demosaic = which;
    return MLVFS_AMD_OK;
}

int mlvfs_amd_mount_set_resample_demosaic(void *mount, int which)
{
    if (!mount) { set_error("mount: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (which != 0 && which != 1) { set_error("mount: a resample demosaic of %d (0: the linear filter, 1: AMaZE)", which); return MLVFS_AMD_ERR_ARG; }
    Mount &m = *(Mount *)mount;
    std::lock_guard<std::mutex> lk(m.mu);                // between serving calls: a call in flight holds the mutex
    m.resample_demosaic = which;
    return MLVFS_AMD_OK;
}

int mlvfs_amd_mount_set_jpeg_sampling(void *mount, int sampling)
{
    if (!mount) { set_error("mount: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (!jpg_sampling_ok(sampling)) { set_error("mount: a JPEG sampling of %d (0: 4:2:0, 1: 4:2:2, 2: 4:4:4)", sampling); return MLVFS_AMD_ERR_ARG; }
    Mount &m = *(Mount *)mount;
    std::lock_guard<std::mutex> lk(m.mu);                // between serving calls: a call in flight holds the mutex
    m.jpeg_sampling = sampling;
    return MLVFS_AMD_OK;
}

size_t mlvfs_amd_mount_dng_size(const void *mount, int index)
{
    if (!mount) { set_error("mount: null argument"); return 0; }
    Mount &m = *(Mount *)mount;
    frame_headers fh;
    if (index < 0 || !mlvfs_amd_mlv_frame_headers(m.reader, index, &fh)) { set_error("mount: frame %d has no usable headers", index); return 0; }
    int proxy;
    {
        std::lock_guard<std::mutex> lk(m.mu);
        proxy = m.proxy;
    }
    if (proxy != 2) return dng_get_size(&fh);
    int pw, ph;
    if (!proxy_geom(fh.rawi_hdr.xRes, fh.rawi_hdr.yRes, &pw, &ph)) { set_error("mount: a proxy takes frames of 4x4 and more, not %dx%d", fh.rawi_hdr.xRes, fh.rawi_hdr.yRes); return 0; }
    return dng_get_header_size() + (size_t)pw * ph * 2;
}

int mlvfs_amd_proxy_geom(int width, int height, int factor, int *pw, int *ph)
{
    if (!pw || !ph) { set_error("proxy_geom: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (factor != 2) { set_error("proxy_geom: a factor of %d (only 2 is built)", factor); return MLVFS_AMD_ERR_ARG; }
    int w2, h2;
    if (!proxy_geom(width, height, &w2, &h2)) { set_error("proxy_geom: %dx%d not supported (4x4 up to 2^27 pixels)", width, height); return MLVFS_AMD_ERR_ARG; }
    *pw = w2;
    *ph = h2;
    return MLVFS_AMD_OK;
}

int mlvfs_amd_bin2_dev(const void *d_frames, size_t stride, int width, int height, void *d_out, size_t out_stride, int nframes, void *stream)
{
    if (!d_frames || !d_out) { set_error("bin2: null argument"); return MLVFS_AMD_ERR_ARG; }
    if (nframes < 0) { set_error("bin2: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    int pw, ph;
    if (!proxy_geom(width, height, &pw, &ph)) { set_error("bin2: %dx%d not supported (4x4 up to 2^27 pixels)", width, height); return MLVFS_AMD_ERR_ARG; }
    const size_t img = (size_t)width * height * 2, pimg = (size_t)pw * ph * 2;
    if (((uintptr_t)d_frames & 1) || ((uintptr_t)d_out & 1) || (nframes > 1 && (stride < img || out_stride < pimg || ((stride | out_stride) & 1)))) {
        set_error("bin2: strides %zu / %zu too small or odd", stride, out_stride);
        return MLVFS_AMD_ERR_ARG;
    }
    if (nframes == 0) return MLVFS_AMD_OK;
    const uintptr_t a0 = (uintptr_t)d_frames, a1 = a0 + (size_t)(nframes - 1) * stride + img;
    const uintptr_t b0 = (uintptr_t)d_out, b1 = b0 + (size_t)(nframes - 1) * out_stride + pimg;
    if (a0 < b1 && b0 < a1) { set_error("bin2: the source and the destination overlap (the binning does not work in place)"); return MLVFS_AMD_ERR_ARG; }
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    return launch_bin2(d_frames, stride, d_out, out_stride, width, height, nframes, pick_stream(stream, c));
}

// every serving entry point; sv: what the call asks for, as the entry point states it -- the route's demosaic, the chroma sampling
// and the rendering's size are settled here, under the handle's lock
static int mount_serve(void *mount, int first, int count, void *h_out, size_t out_stride, int batch_frames, int io_threads, int *results, Serve sv)
{
    if (!mount || !h_out || ((sv.lossless || sv.quality) && (!sv.sizes || !sv.flags))) { set_error("mount: null argument"); return MLVFS_AMD_ERR_ARG; }
    Mount &m = *(Mount *)mount;
    if (count < 0) { set_error("mount: negative frame count"); return MLVFS_AMD_ERR_ARG; }
    if (count == 0) return MLVFS_AMD_OK;
    const int frames = mlvfs_amd_mlv_frame_count(m.reader);
    if (first < 0 || (long long)first + count > frames) { set_error("mount: frames %d..%d outside the clip (%d frames)", first, first + count - 1, frames); return MLVFS_AMD_ERR_ARG; }
    std::vector<frame_headers> fh(count);
    for (int k = 0; k < count; k++)
        if (!mlvfs_amd_mlv_frame_headers(m.reader, first + k, &fh[k])) { set_error("mount: frame %d has no usable headers", first + k); return MLVFS_AMD_ERR_ARG; }
    const int w = fh[0].rawi_hdr.xRes, h = fh[0].rawi_hdr.yRes, bpp = fh[0].rawi_hdr.raw_info.bits_per_pixel;
    if (w <= 0 || h <= 0 || bpp < 1 || bpp > 16) { set_error("mount: unsupported frame %dx%d at %d bits", w, h, bpp); return MLVFS_AMD_ERR_ARG; }
    for (int k = 1; k < count; k++)
        if (fh[k].rawi_hdr.xRes != w || fh[k].rawi_hdr.yRes != h || fh[k].rawi_hdr.raw_info.bits_per_pixel != bpp) {
            set_error("mount: frames of more than one geometry in one call (frame %d)", first + k);
            return MLVFS_AMD_ERR_ARG;
        }
    if (batch_frames <= 0) batch_frames = 8;
    batch_frames = std::min(batch_frames, count);
    LibcRandGuard rand_guard;                      // HIP code runs: the caller's rand() stream stays out of its reach (rand_mode 0 draws from it)
    std::lock_guard<std::mutex> lk(m.mu);
    size_t size = dng_get_size(&fh[0]);
    if (m.proxy == 2) {                                                // the proxy file: anything from its size up is room enough
        int pw, ph;
        if (!proxy_geom(w, h, &pw, &ph)) { set_error("mount: a proxy takes frames of 4x4 and more, not %dx%d", w, h); return MLVFS_AMD_ERR_ARG; }
        size = dng_get_header_size() + (size_t)pw * ph * 2;
    }
    const bool full = sv.in_full();
    if (sv.tensor && m.proxy == 2) { set_error("mount: a handle that serves proxies does not serve tensors"); return MLVFS_AMD_ERR_ARG; }
    if (sv.gain_q8) {
        if (m.proxy == 2) { set_error("mount: a handle that serves proxies does not render"); return MLVFS_AMD_ERR_ARG; }
        bool unserved;
        sv.route = mount_route(sv.route.size, sv.route.ow, sv.route.oh, m.demosaic, m.resample_demosaic, &unserved);
        if (unserved) { set_error("mount: with AMaZE set (mlvfs_amd_mount_set_demosaic) the resampled calls are not served"); return MLVFS_AMD_ERR_ARG; }
        if (!route_geom(sv.route, w, h, &sv.pw, &sv.ph)) return route_refuse("mount", sv.route, w, h);
        sv.sampling = m.jpeg_sampling;
        size = mlvfs_amd_rgb_header_size() + sv.bpx() * sv.pw * sv.ph;
        if (!sv.tensor && out_stride < size) { set_error("mount: out_stride %zu smaller than a rendered file (%zu)", out_stride, size); return MLVFS_AMD_ERR_ARG; }
    }
    if (sv.tensor) {                                                   // the tensor's bytes in the place of a file's
        const size_t es = tensor_elem(sv.tensor->dtype);
        if (!sv.gain_q8) {
            if (w < 2 || h < 2 || (uint64_t)w * (uint64_t)h >= (1u << 28)) { set_error("mount: a Bayer tensor takes frames of 2x2 up to 2^28 pixels, not %dx%d", w, h); return MLVFS_AMD_ERR_ARG; }
            int32_t levels[TENSOR_LEVELS];
            for (int k = 0; k < count; k++)
                if (const int rl = mlvfs_amd_tensor_bayer_params(&fh[k], levels)) return rl;
        }
        size = sv.gain_q8 ? (size_t)3 * sv.pw * sv.ph * es : (size_t)4 * (w / 2) * (h / 2) * es;
        if (out_stride < size || out_stride % es || (uintptr_t)h_out % es) {
            set_error("mount: out_stride %zu smaller than a tensor (%zu), or the stride or the destination off the element's boundary", out_stride, size);
            return MLVFS_AMD_ERR_ARG;
        }
    }
    if (out_stride < size) { set_error("mount: out_stride %zu smaller than a .dng file (%zu)", out_stride, size); return MLVFS_AMD_ERR_ARG; }
    if (m.dark && !darkframe_fits(m.dark, w, h, bpp)) { set_error("mount: the dark frame does not have the geometry of frame %d (%dx%d at %d bits)", first, w, h, bpp); return MLVFS_AMD_ERR_ARG; }
    if (m.flat && !flatfield_fits(m.flat, w, h)) { set_error("mount: the flat field does not have the geometry of frame %d (%dx%d)", first, w, h); return MLVFS_AMD_ERR_ARG; }
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    if (sv.tensor) {                                                   // device memory on the handle's device, its first byte and its last
        const uint8_t *ends[2] = { (const uint8_t *)h_out, (const uint8_t *)h_out + (size_t)(count - 1) * out_stride + size - 1 };
        for (const uint8_t *p : ends) {
            hipPointerAttribute_t at{};
            if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != c->dev->id) {
                (void)hipGetLastError();
                set_error("mount: d_out is not device memory on the handle's device (%d)", c->dev->id);
                return MLVFS_AMD_ERR_ARG;
            }
        }
    }
    const size_t img = (size_t)w * h * 2, dstride = up256(img);
    const size_t pn = o_pn_bytes(m.o, w, h, batch_frames);
    size_t scratch = std::max(pn, deflicker_batch_scratch_bytes(bpp > 15 ? 15 : bpp, batch_frames));
    scratch = std::max(scratch, up256(4 * (size_t)65536 * sizeof(unsigned) * batch_frames) + up256(sizeof(HdrPreviewParams) * batch_frames));
    if (sv.lossless) scratch = std::max(scratch, lje_fixed_bytes((uint32_t)(img / 2), batch_frames) + dstride * batch_frames);
    size_t full_bytes = full ? full_stride(sv.pw, sv.ph, sv.bpx()) * batch_frames : 0;  // d_full: the batch's renderings ...
    if (sv.quality) {
        const int pw = sv.pw, ph = sv.ph;
        if (pw > 65535 || ph > 65535) { set_error("mount: a JPEG file takes renderings of up to 65535 a side, not %dx%d", pw, ph); return MLVFS_AMD_ERR_ARG; }
        if (const size_t room = full ? jpg_room(pw, ph) : std::min(jpg_room(pw, ph), dstride))
            scratch = std::max(scratch, jpg_scratch_bytes(jpg_layout(pw, ph, jpg_rowcap(room, ph, sv.sampling), sv.sampling), batch_frames));
        if (full) full_bytes += up256(jpg_room(pw, ph)) * batch_frames;                  // ... and their streams behind them
    }
    m.served = true;
    Calib cal;
    int rc = calib_on_device(m.dark, m.flat, c, w, h, bpp, 0, &cal);
    if (rc == MLVFS_AMD_OK) rc = m.ensure(c->dev->id, dstride * batch_frames, scratch);
    if (rc == MLVFS_AMD_OK && (sv.gain_q8 || sv.tensor)) rc = m.ensure_rgb(batch_frames);
    if (rc == MLVFS_AMD_OK && full) rc = m.d_full.reserve(full_bytes);
    for (int f0 = 0; rc == MLVFS_AMD_OK && f0 < count;) {
        int n = std::min(batch_frames, count - f0);
        if (m.o.dual_iso == 2 && m.o.fix_bad_pixels) {
            std::shared_ptr<Clip> known;
            if (!cached_bad_clip(&fh[f0], c, m.o.fix_bad_pixels == 2, &known)) n = 1;     // until the map exists: strictly in serve order
        }
        if (m.flat) {                                                                      // the frames' own black level: one per load
            cal.black = fh[f0].rawi_hdr.raw_info.black_level;
            for (int k = 1; k < n; k++) if (fh[f0 + k].rawi_hdr.raw_info.black_level != cal.black) { n = k; break; }
        }
        rc = reader_load_batch(m.reader, first + f0, n, w, h, bpp, m.d_frames, dstride, io_threads, c->stream, &cal);
        if (rc == MLVFS_AMD_OK)
            rc = serve_batch(m, c, fh.data() + f0, n, dstride, (uint8_t *)h_out + (size_t)f0 * out_stride, out_stride, results ? results + f0 : nullptr,
                             sv.from(f0));
        f0 += n;
    }
    if (rc != MLVFS_AMD_OK) (void)hipStreamSynchronize(c->stream);
    return rc;
}

// what the rendering entry points check before mount_serve, one rule each, in this order: the deep look of a 16-bit call, the gain, a
// JPEG call's quality, the size of a scaled or a resampled rendering
static bool gain_ok(int gain_q8)
{
    if (gain_q8 >= 1 && gain_q8 <= 65535) return true;
    set_error("mount: a gain_q8 of %d (1 .. 65535, 256 is unity)", gain_q8);
    return false;
}
static bool quality_ok(int quality)
{
    if (quality >= 1 && quality <= 100) return true;
    set_error("mount: a JPEG quality of %d (1 .. 100)", quality);
    return false;
}
static bool size_ok(const RenderRoute &r)
{
    if (!r.sized() || (r.ow >= 1 && r.oh >= 1)) return true;
    set_error("mount: a %s rendering of %dx%d", r.size == RenderRoute::SCALED ? "scaled" : "resampled", r.ow, r.oh);
    return false;
}
enum class As { TIFF, TIFF16, JPEG };
static int mount_render(void *mount, int first, int count, void *h_out, size_t out_stride, int batch_frames, int io_threads, int *results, As as,
                        const Serve &sv)
{
    if (as == As::TIFF16 && !sv.deep) { set_error("mount: null argument (a 16-bit rendering takes a deep look)"); return MLVFS_AMD_ERR_ARG; }
    if (!gain_ok(sv.gain_q8) || (as == As::JPEG && !quality_ok(sv.quality)) || !size_ok(sv.route)) return MLVFS_AMD_ERR_ARG;
    return mount_serve(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, sv);
}
static Serve rendered(int gain_q8, RenderRoute::Size size, int ow = 0, int oh = 0)
{
    Serve sv;
    sv.gain_q8 = gain_q8;
    sv.route = { size, false, ow, oh };
    return sv;
}
static Serve rendered16(int gain_q8, const mlvfs_amd_look16_t *look, RenderRoute::Size size, int ow = 0, int oh = 0)
{
    Serve sv = rendered(gain_q8, size, ow, oh);
    sv.deep = look;
    return sv;
}
static Serve jpeg(int gain_q8, int quality, size_t *sizes, int *flags, RenderRoute::Size size, int ow = 0, int oh = 0)
{
    Serve sv = rendered(gain_q8, size, ow, oh);
    sv.quality = quality;
    sv.sizes = sizes;
    sv.flags = flags;
    return sv;
}

int mlvfs_amd_mount_dng(void *mount, int first, int count, void *h_out, size_t out_stride, int batch_frames, int io_threads, int *results)
{
    return mount_serve(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, Serve());
}

int mlvfs_amd_mount_dng_lossless(void *mount, int first, int count, void *h_out, size_t out_stride, size_t *sizes, int *flags,
                                 int batch_frames, int io_threads, int *results)
{
    Serve sv;
    sv.lossless = true;
    sv.sizes = sizes;
    sv.flags = flags;
    return mount_serve(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, sv);
}

int mlvfs_amd_mount_rgb(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int batch_frames, int io_threads,
                        int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::TIFF, rendered(gain_q8, RenderRoute::HALF));
}

int mlvfs_amd_mount_jpeg(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int quality, size_t *sizes, int *flags,
                         int batch_frames, int io_threads, int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::JPEG,
                        jpeg(gain_q8, quality, sizes, flags, RenderRoute::HALF));
}

int mlvfs_amd_mount_rgb_full(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int batch_frames, int io_threads,
                             int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::TIFF, rendered(gain_q8, RenderRoute::FULL));
}

int mlvfs_amd_mount_jpeg_full(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int quality, size_t *sizes,
                              int *flags, int batch_frames, int io_threads, int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::JPEG,
                        jpeg(gain_q8, quality, sizes, flags, RenderRoute::FULL));
}

int mlvfs_amd_mount_rgb_scaled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int ow, int oh, int batch_frames,
                               int io_threads, int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::TIFF,
                        rendered(gain_q8, RenderRoute::SCALED, ow, oh));
}

int mlvfs_amd_mount_jpeg_scaled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int quality, int ow, int oh,
                                size_t *sizes, int *flags, int batch_frames, int io_threads, int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::JPEG,
                        jpeg(gain_q8, quality, sizes, flags, RenderRoute::SCALED, ow, oh));
}

int mlvfs_amd_mount_rgb_resampled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int ow, int oh, int batch_frames,
                                  int io_threads, int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::TIFF,
                        rendered(gain_q8, RenderRoute::RESAMPLED, ow, oh));
}

int mlvfs_amd_mount_jpeg_resampled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int quality, int ow, int oh,
                                   size_t *sizes, int *flags, int batch_frames, int io_threads, int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::JPEG,
                        jpeg(gain_q8, quality, sizes, flags, RenderRoute::RESAMPLED, ow, oh));
}

int mlvfs_amd_mount_rgb16(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, const mlvfs_amd_look16_t *look,
                          int batch_frames, int io_threads, int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::TIFF16,
                        rendered16(gain_q8, look, RenderRoute::HALF));
}

int mlvfs_amd_mount_rgb16_full(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, const mlvfs_amd_look16_t *look,
                               int batch_frames, int io_threads, int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::TIFF16,
                        rendered16(gain_q8, look, RenderRoute::FULL));
}

int mlvfs_amd_mount_rgb16_scaled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int ow, int oh,
                                 const mlvfs_amd_look16_t *look, int batch_frames, int io_threads, int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::TIFF16,
                        rendered16(gain_q8, look, RenderRoute::SCALED, ow, oh));
}

int mlvfs_amd_mount_rgb16_resampled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int ow, int oh,
                                    const mlvfs_amd_look16_t *look, int batch_frames, int io_threads, int *results)
{
    return mount_render(mount, first, count, h_out, out_stride, batch_frames, io_threads, results, As::TIFF16,
                        rendered16(gain_q8, look, RenderRoute::RESAMPLED, ow, oh));
}

// what a tensor call's spec asks of the mount, beyond tensor_spec_ok: the kind, and for an RGB tensor the size kind, the size and the gain
static bool tensor_mount_spec_ok(const mlvfs_amd_tensor_spec_t *spec)
{
    if (!spec) { set_error("mount: null argument"); return false; }
    if (spec->kind != MLVFS_AMD_TENSOR_RGB && spec->kind != MLVFS_AMD_TENSOR_BAYER) { set_error("mount: a tensor kind of %d (0: RGB, 1: Bayer)", spec->kind); return false; }
    const bool bayer = spec->kind == MLVFS_AMD_TENSOR_BAYER;
    if (!tensor_spec_ok("mount", spec, bayer || spec->look16 ? 16 : 8, bayer ? 4 : 3)) return false;
    if (bayer) return true;
    if (spec->size < MLVFS_AMD_TENSOR_HALF || spec->size > MLVFS_AMD_TENSOR_RESAMPLED) { set_error("mount: a tensor size kind of %d (0 .. 3)", spec->size); return false; }
    return gain_ok(spec->gain_q8) && size_ok({ (RenderRoute::Size)spec->size, false, spec->ow, spec->oh });
}
static_assert(RenderRoute::HALF == MLVFS_AMD_TENSOR_HALF && RenderRoute::FULL == MLVFS_AMD_TENSOR_FULL && RenderRoute::SCALED == MLVFS_AMD_TENSOR_SCALED &&
              RenderRoute::RESAMPLED == MLVFS_AMD_TENSOR_RESAMPLED, "a spec's size kind is a route's");

int mlvfs_amd_mount_tensor(void *mount, int first, int count, void *d_out, size_t out_stride, const mlvfs_amd_tensor_spec_t *spec, int batch_frames,
                           int io_threads, int *results)
{
    if (!tensor_mount_spec_ok(spec)) return MLVFS_AMD_ERR_ARG;
    Serve sv;
    if (spec->kind == MLVFS_AMD_TENSOR_RGB) sv = spec->look16 ? rendered16(spec->gain_q8, spec->look16, (RenderRoute::Size)spec->size, spec->ow, spec->oh)
                                                              : rendered(spec->gain_q8, (RenderRoute::Size)spec->size, spec->ow, spec->oh);
    sv.tensor = spec;
    return mount_serve(mount, first, count, d_out, out_stride, batch_frames, io_threads, results, sv);
}

size_t mlvfs_amd_mount_tensor_bytes(const void *mount, int index, const mlvfs_amd_tensor_spec_t *spec)
{
    if (!mount) { set_error("mount: null argument"); return 0; }
    if (!tensor_mount_spec_ok(spec)) return 0;
    Mount &m = *(Mount *)mount;
    frame_headers fh;
    if (index < 0 || !mlvfs_amd_mlv_frame_headers(m.reader, index, &fh)) { set_error("mount: frame %d has no usable headers", index); return 0; }
    const int w = fh.rawi_hdr.xRes, h = fh.rawi_hdr.yRes;
    const size_t es = tensor_elem(spec->dtype);
    if (spec->kind == MLVFS_AMD_TENSOR_BAYER) {
        if (w < 2 || h < 2 || (uint64_t)w * (uint64_t)h >= (1u << 28)) { set_error("mount: a Bayer tensor takes frames of 2x2 up to 2^28 pixels, not %dx%d", w, h); return 0; }
        return (size_t)4 * (w / 2) * (h / 2) * es;
    }
    RenderRoute route;
    {
        std::lock_guard<std::mutex> lk(m.mu);
        route = mount_route((RenderRoute::Size)spec->size, spec->ow, spec->oh, m.demosaic, m.resample_demosaic);
    }
    int pw, ph;
    if (!route_geom(route, w, h, &pw, &ph)) { (void)route_refuse("mount", route, w, h); return 0; }
    return (size_t)3 * pw * ph * es;
}

// the size of a rendered 8-bit TIFF file of frame `index`: the handle's route for that size kind and its geometry.  A rendering's size
// does not depend on whether the handle's settings let the call be served
static size_t mount_rgb_size(const void *mount, int index, RenderRoute::Size size, int ow = 0, int oh = 0)
{
    if (!mount) { set_error("mount: null argument"); return 0; }
    Mount &m = *(Mount *)mount;
    frame_headers fh;
    if (index < 0 || !mlvfs_amd_mlv_frame_headers(m.reader, index, &fh)) { set_error("mount: frame %d has no usable headers", index); return 0; }
    RenderRoute route;
    {
        std::lock_guard<std::mutex> lk(m.mu);
        route = mount_route(size, ow, oh, m.demosaic, m.resample_demosaic);
    }
    int pw, ph;
    if (!route_geom(route, fh.rawi_hdr.xRes, fh.rawi_hdr.yRes, &pw, &ph)) { (void)route_refuse("mount", route, fh.rawi_hdr.xRes, fh.rawi_hdr.yRes); return 0; }
    return mlvfs_amd_rgb_header_size() + (size_t)3 * pw * ph;
}

size_t mlvfs_amd_mount_rgb_size(const void *mount, int index) { return mount_rgb_size(mount, index, RenderRoute::HALF); }
size_t mlvfs_amd_mount_rgb_full_size(const void *mount, int index) { return mount_rgb_size(mount, index, RenderRoute::FULL); }
size_t mlvfs_amd_mount_rgb_scaled_size(const void *mount, int index, int ow, int oh) { return mount_rgb_size(mount, index, RenderRoute::SCALED, ow, oh); }
size_t mlvfs_amd_mount_rgb_resampled_size(const void *mount, int index, int ow, int oh) { return mount_rgb_size(mount, index, RenderRoute::RESAMPLED, ow, oh); }

// a 16-bit file has the 8-bit file's header and twice its pixel bytes
static size_t twice_the_pixels(size_t size8) { return size8 ? 2 * size8 - mlvfs_amd_rgb_header_size() : 0; }
size_t mlvfs_amd_mount_rgb16_size(const void *mount, int index) { return twice_the_pixels(mlvfs_amd_mount_rgb_size(mount, index)); }
size_t mlvfs_amd_mount_rgb16_full_size(const void *mount, int index) { return twice_the_pixels(mlvfs_amd_mount_rgb_full_size(mount, index)); }
size_t mlvfs_amd_mount_rgb16_scaled_size(const void *mount, int index, int ow, int oh)
{
    return twice_the_pixels(mlvfs_amd_mount_rgb_scaled_size(mount, index, ow, oh));
}
size_t mlvfs_amd_mount_rgb16_resampled_size(const void *mount, int index, int ow, int oh)
{
    return twice_the_pixels(mlvfs_amd_mount_rgb_resampled_size(mount, index, ow, oh));
}

}  // extern "C"

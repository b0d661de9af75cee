// fused_pass.cpp -- the fused pass (pixel repair, chroma smoothing, stripes in one launch over packed or 16-bit frames) as the host runs
// it, and its entry points for a clip's frames in device and in host memory (PART 2 of include/mlvfs_amd.h).
#include "fused_pass.h"

#include <map>

namespace mlv {

int run_fused_pass(const Device *dev, const FusedPass &p, const void *src, size_t src_stride, void *dst, size_t dst_stride, int nframes,
                   void *patches, hipStream_t stream, Clip *layout_of)
{
    const Geom &g = p.g;
    const bool packed = p.src_bpp != 0;
    if (p.idle()) {
        if (packed) return launch_unpack(src, src_stride, dst, dst_stride, 0, (uint32_t)g.w * g.h, p.src_bpp, nframes, stream);
        MLV_HIP(hipMemcpy2DAsync(dst, dst_stride, src, src_stride, (size_t)g.w * g.h * 2, nframes, hipMemcpyDeviceToDevice, stream));
        return MLVFS_AMD_OK;
    }
    const int geo = frame_geo_of(p.cs);
    PatchView pv{};
    if (p.map) {
        int rc = launch_pixfix_for_frame_kernel(*p.map, geo, g, p.src_bpp, src, src_stride, patches, nframes, dev->luts, stream);
        if (rc) return rc;
        pv = PatchView{ Clip::cells_of(patches, p.map->n_entries, nframes), p.map->n_rec[geo], p.map->d_tile_off[geo] };
    }
    if (layout_of && p.cs != 0 && layout_of->t16_layout == 0) {
        // the clip's T16 layout: decided once, from the first frame it processes with chroma smoothing (30 % of the sampled pixels
        // 1 .. 511 above black: the spread layout, k_frame.hip), unless the caller fixed it; synchronises the stream
        int share = 0;
        int rc = dark_share(p.src_bpp, src, g.w, g.h, g.black, stream, &share);
        if (rc) return rc;
        layout_of->t16_layout = share >= 307 ? 2 : 1;
    }
    return launch_frame(dev, g, packed, src, src_stride, dst, dst_stride, nframes, p.cs, p.map ? &pv : nullptr, p.stripes, p.coef, stream,
                        layout_of && layout_of->t16_layout == 2);
}

}  // namespace mlv

using namespace mlv;

// the pass over frames in device memory for a caller that owns the clip: the patch list is the clip's, the layout is decided on the way
static int run_on_clip(ThreadCtx *c, Clip *clip, const FusedPass &p, const void *src, size_t src_stride, void *dst, size_t dst_stride,
                       int nframes, hipStream_t s)
{
    if (p.map)
        if (const int rc = clip->d_patches.reserve(clip->patch_buffer_bytes(nframes))) return rc;
    return run_fused_pass(c->dev, p, src, src_stride, dst, dst_stride, nframes, clip->d_patches, s, clip);
}

extern "C" {

int mlvfs_amd_process_frames_dev(mlvfs_amd_clip_t *clip_, const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride,
                                 int nframes, int cs_method, int fix_pixels, int apply_stripes, void *stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    Clip *clip = reinterpret_cast<Clip *>(clip_);
    hipStream_t s = pick_stream(stream, c);
    const FusedPass p = fused_pass_of(*clip, clip->g.bpp, cs_method, fix_pixels, apply_stripes);
    if (!p.idle() && !frame_kernel_takes(clip->g, d_packed, packed_stride, d_out, out_stride, nframes)) {
        // n-bit clips (dng.c:813-843 handles any depth) and 12- / 10-bit ones in geometries the fused loader does not take: unpack
        // first, then the same stages on 16-bit frames
        const size_t ustride = ((size_t)clip->g.w * clip->g.h * 2 + 255) / 256 * 256;
        int rc = clip->d_unpacked.reserve(ustride * nframes);
        if (rc) return rc;
        rc = launch_unpack(d_packed, packed_stride, clip->d_unpacked, ustride, 0, (uint32_t)clip->g.w * clip->g.h, clip->g.bpp, nframes, s);
        if (rc) return rc;
        return mlvfs_amd_process_unpacked_dev(clip_, clip->d_unpacked, ustride, d_out, out_stride, nframes, p.cs, fix_pixels,
                                              apply_stripes, stream);
    }
    return run_on_clip(c, clip, p, d_packed, packed_stride, d_out, out_stride, nframes, s);
}

// the same stages on frames that are already 16-bit in HBM (decoded LJ92 payloads, csrc/lj92.cpp)
int mlvfs_amd_process_unpacked_dev(mlvfs_amd_clip_t *clip_, const void *d_frames, size_t stride, void *d_out, size_t out_stride,
                                   int nframes, int cs_method, int fix_pixels, int apply_stripes, void *stream)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    Clip *clip = reinterpret_cast<Clip *>(clip_);
    if (nframes <= 0) return MLVFS_AMD_OK;
    return run_on_clip(c, clip, fused_pass_of(*clip, 0, cs_method, fix_pixels, apply_stripes), d_frames, stride, d_out, out_stride, nframes,
                       pick_stream(stream, c));
}

// ---- frames that live in HOST memory: chunked, triple-buffered H2D -> fused kernel -> D2H ------------------------
namespace {
struct HostPipe {                       // per host thread and device
    // One stream per STAGE (uploads, kernels, downloads), a ring of NS buffer slots, events between the stages.  All uploads
    // queue on one stream and all downloads on another, so each direction of the link carries one transfer at a time, back to
    // back (tools/pcie_bw.py: 48.6 GB/s each way when both run); with one stream per SLOT, each doing upload -> kernel ->
    // download, transfers of the same direction interleaved and the pipeline stopped at 67 GB/s for both directions together.
    static constexpr int NS = 4;
    hipStream_t s[3] = { nullptr, nullptr, nullptr };       // 0 upload, 1 kernels, 2 download
    hipEvent_t up[NS] = {}, run[NS] = {}, down[NS] = {};
    DevBuf d_in[NS], d_out[NS], d_patch[NS];
    int device = 0;
    HostPipe() { (void)hipGetDevice(&device); }
    HostPipe(const HostPipe &) = delete;
    ~HostPipe()                                               // with the host thread that owned it
    {
        for (int k = 0; k < 3; k++)
            if (s[k]) { (void)hipStreamSynchronize(s[k]); release_stream_state(device, s[k]); (void)hipStreamDestroy(s[k]); }
        for (int k = 0; k < NS; k++) {
            if (up[k]) (void)hipEventDestroy(up[k]);
            if (run[k]) (void)hipEventDestroy(run[k]);
            if (down[k]) (void)hipEventDestroy(down[k]);
        }
    }
    int ensure(size_t in_bytes, size_t out_bytes, size_t patch_bytes)
    {
        for (int k = 0; k < 3; k++)
            if (!s[k]) MLV_HIP(hipStreamCreateWithFlags(&s[k], hipStreamNonBlocking));
        for (int k = 0; k < NS; k++)
            if (!up[k]) {
                MLV_HIP(hipEventCreateWithFlags(&up[k], hipEventDisableTiming));
                MLV_HIP(hipEventCreateWithFlags(&run[k], hipEventDisableTiming));
                MLV_HIP(hipEventCreateWithFlags(&down[k], hipEventDisableTiming));
            }
        for (int k = 0; k < NS; k++) {
            if (const int rc = d_in[k].reserve(in_bytes)) return rc;
            if (const int rc = d_out[k].reserve(out_bytes)) return rc;
            if (const int rc = d_patch[k].reserve(patch_bytes)) return rc;
        }
        return MLVFS_AMD_OK;
    }
};
thread_local std::map<int, HostPipe> t_pipe;
}  // namespace

int mlvfs_amd_process_frames_host(mlvfs_amd_clip_t *clip_, const void *h_packed, size_t packed_stride, void *h_out, size_t out_stride,
                                  int nframes, int cs_method, int fix_pixels, int apply_stripes, int chunk_frames)
{
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    Clip *clip = reinterpret_cast<Clip *>(clip_);
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (chunk_frames <= 0) chunk_frames = 8;
    if (chunk_frames > nframes) chunk_frames = nframes;
    const size_t row_bytes = (size_t)clip->g.w * clip->g.h * 2;
    const size_t dstride_in = (packed_stride + 15) / 16 * 16, dstride_out = (row_bytes + 15) / 16 * 16;
    HostPipe &hp = t_pipe[c->dev->id];
    const bool piped = clip->g.bpp == 14;
    const FusedPass p = fused_pass_of(*clip, 14, cs_method, fix_pixels, apply_stripes);
    int rc = hp.ensure(dstride_in * chunk_frames + 16, dstride_out * chunk_frames, piped && p.map ? clip->patch_buffer_bytes(chunk_frames) : 0);
    if (rc) return rc;
    if (!piped) {
        // other bit depths: chunks go through the device entry point (unpack + stages on 16-bit frames), one stream, no overlap
        for (int f0 = 0; f0 < nframes; f0 += chunk_frames) {
            const int n = std::min(chunk_frames, nframes - f0);
            hipStream_t s0 = hp.s[0];
            MLV_HIP(hipMemcpy2DAsync(hp.d_in[0], dstride_in, (const uint8_t *)h_packed + (size_t)f0 * packed_stride, packed_stride, packed_stride, n, hipMemcpyHostToDevice, s0));
            rc = mlvfs_amd_process_frames_dev(clip_, hp.d_in[0], dstride_in, hp.d_out[0], dstride_out, n, cs_method, fix_pixels, apply_stripes, s0);
            if (rc) return rc;
            MLV_HIP(hipMemcpy2DAsync((uint8_t *)h_out + (size_t)f0 * out_stride, out_stride, hp.d_out[0], dstride_out, row_bytes, n, hipMemcpyDeviceToHost, s0));
            MLV_HIP(hipStreamSynchronize(s0));
        }
        return MLVFS_AMD_OK;
    }
    for (int f0 = 0, k = 0; f0 < nframes; f0 += chunk_frames, k++) {
        const int n = std::min(chunk_frames, nframes - f0), slot = k % HostPipe::NS;
        const uint8_t *src = (const uint8_t *)h_packed + (size_t)f0 * packed_stride;
        uint8_t *dst = (uint8_t *)h_out + (size_t)f0 * out_stride;
        // upload: the slot's input buffer is free once the kernels of its previous chunk have run
        hipStream_t s = hp.s[0];
        if (k >= HostPipe::NS) MLV_HIP(hipStreamWaitEvent(s, hp.run[slot], 0));
        if (packed_stride == dstride_in) MLV_HIP(hipMemcpyAsync(hp.d_in[slot], src, packed_stride * n, hipMemcpyHostToDevice, s));
        else MLV_HIP(hipMemcpy2DAsync(hp.d_in[slot], dstride_in, src, packed_stride, packed_stride, n, hipMemcpyHostToDevice, s));
        MLV_HIP(hipEventRecord(hp.up[slot], s));
        // kernels: after the upload, and after the slot's previous output has been downloaded; one patch buffer per slot
        s = hp.s[1];
        MLV_HIP(hipStreamWaitEvent(s, hp.up[slot], 0));
        if (k >= HostPipe::NS) MLV_HIP(hipStreamWaitEvent(s, hp.down[slot], 0));
        rc = run_fused_pass(c->dev, p, hp.d_in[slot], dstride_in, hp.d_out[slot], dstride_out, n, hp.d_patch[slot], s, clip);
        if (rc) return rc;
        MLV_HIP(hipEventRecord(hp.run[slot], s));
        // download
        s = hp.s[2];
        MLV_HIP(hipStreamWaitEvent(s, hp.run[slot], 0));
        if (out_stride == dstride_out) MLV_HIP(hipMemcpyAsync(dst, hp.d_out[slot], out_stride * n, hipMemcpyDeviceToHost, s));
        else MLV_HIP(hipMemcpy2DAsync(dst, out_stride, hp.d_out[slot], dstride_out, row_bytes, n, hipMemcpyDeviceToHost, s));
        MLV_HIP(hipEventRecord(hp.down[slot], s));
    }
    for (int k = 0; k < 3; k++) MLV_HIP(hipStreamSynchronize(hp.s[k]));
    return MLVFS_AMD_OK;
}

}  // extern "C"

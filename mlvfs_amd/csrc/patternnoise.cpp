// patternnoise.cpp -- drop-in fix_pattern_noise (mlvfs/patternnoise.c:357-380) on
// top of the kernels of k_pnoise.hip: the int16 frame on the device -- the copy the unpack left there, or an upload --,
// the column pass and the row pass (transposed) in place, back to the host unless a frame bracket is open (dropin.cpp).  debug_flags != 0 (MLVFS
// passes 0, main.c:948): one direction only and the reference's debug views (patternnoise.c:215-240, 363-379), reproduced as well.
#include "clip.h"

#include <atomic>

namespace mlv {
size_t pattern_noise_scratch_bytes(int w, int h);
int launch_pattern_noise(void *d_raw, int w, int h, int white, void *d_scratch, hipStream_t stream, int flags);
}

using namespace mlv;

extern "C" void fix_pattern_noise(int16_t *raw, int w, int h, int white, int debug_flags)
{
    LibcRandGuard rand_guard;                      // HIP code may run: keep the caller's rand() stream out of its reach
    printf("Fixing pattern noise...\n");                                   // patternnoise.c:359
    if (w < 2 || h < 2 || (w & 1) || (h & 1)) { set_error("fix_pattern_noise: %dx%d frame not supported", w, h); return; }
    ThreadCtx *c = thread_ctx();
    if (!c) return;
    const size_t bytes = (size_t)w * h * 2;
    void *d_frame = nullptr;
    int which = 0;
    bool was_dirty = false;
    if (inplace_stage_begin(c, STAGE_PNOISE, raw, bytes, &d_frame, &which, &was_dirty)) return;       // the unpack's device copy, or an upload
    const bool done = c->ensure(0, pattern_noise_scratch_bytes(w, h)) == MLVFS_AMD_OK &&
                      launch_pattern_noise(d_frame, w, h, white, c->d_b, c->stream, debug_flags) == MLVFS_AMD_OK;
    inplace_stage_end(c, STAGE_PNOISE, raw, bytes, which, was_dirty, done, true);                              // downloads unless a frame bracket is open
}

static std::atomic<size_t> g_pn_cap_override{ 0 };

size_t mlv::pattern_noise_scratch_cap()
{
    static const size_t cap = [] { const char *e = getenv("MLVFS_AMD_PN_SCRATCH_MB"); const long v = e ? atol(e) : 0; return (size_t)(v > 0 ? v : 256) << 20; }();
    const size_t o = g_pn_cap_override.load();
    return o ? o : cap;
}

// test hook: the scratch cap of batched pattern noise in bytes (0: the default again); returns the cap before
extern "C" size_t mlvfs_amd_test_pn_scratch_cap(size_t bytes)
{
    const size_t before = pattern_noise_scratch_cap();
    g_pn_cap_override = bytes;
    return before;
}

// `nframes` device frames of one geometry, `stride` bytes apart, in place: the 12 launches of one frame per sub-batch (the scratch of
// a sub-batch, 8 bytes per pixel and frame, stays under MLVFS_AMD_PN_SCRATCH_MB, default 256).  Synchronises the stream (the scratch
// is the calling thread's).
extern "C" int mlvfs_amd_fix_pattern_noise_dev(const mlvfs_amd_geom_t *geom, void *d_frames, size_t stride, int nframes, void *stream)
{
    if (!geom || !d_frames || nframes < 0) { set_error("fix_pattern_noise_dev: null argument"); return MLVFS_AMD_ERR_ARG; }
    const int w = geom->width, h = geom->height;
    if (w < 2 || h < 2 || (w & 1) || (h & 1)) { set_error("fix_pattern_noise_dev: %dx%d frame not supported", w, h); return MLVFS_AMD_ERR_ARG; }
    if (nframes > 1 && (stride < (size_t)w * h * 2 || (stride & 1))) { set_error("fix_pattern_noise_dev: stride smaller than a frame or odd"); return MLVFS_AMD_ERR_ARG; }
    if (nframes > 16383) { set_error("fix_pattern_noise_dev: at most 16383 frames per call"); return MLVFS_AMD_ERR_ARG; }
    if (nframes == 0) return MLVFS_AMD_OK;
    ThreadCtx *c = thread_ctx();
    if (!c) return MLVFS_AMD_ERR_HIP;
    const size_t per = pattern_noise_batch_frame_bytes(w, h), cap = pattern_noise_scratch_cap();
    const size_t bytes = per * (size_t)std::max<size_t>(1, std::min<size_t>((size_t)nframes, cap / per));
    if (c->ensure(0, bytes)) return MLVFS_AMD_ERR_HIP;
    hipStream_t s = pick_stream(stream, c);
    const int rc = launch_pattern_noise_batch(d_frames, nframes > 1 ? stride : (size_t)w * h * 2, nframes, w, h, geom->white, c->d_b, bytes, s);
    if (rc) return rc;
    MLV_HIP(hipStreamSynchronize(s));
    return MLVFS_AMD_OK;
}

// clip.h -- per-clip state (stripe coefficients + ordered pixel map) and the
// launcher prototypes shared between the host files and the kernel files.
#pragma once

#include "common.h"

#include <algorithm>
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

namespace mlv {

// tile geometry of the fused kernel (k_frame.hip); the per-tile patch lists are built
// on the host with the same numbers
// One tile height since round 4: 15 cell rows (15 rows x 17 lanes of the 5x5 medians, 15 x 17 loader items: k_frame.hip).  The
// two-geometry plumbing of rounds 2-3 (16 rows without 5x5) is kept: both entries are the same now.
constexpr int FRAME_TCW = 64, FRAME_TCH = 15, FRAME_TCH5 = 15, FRAME_HC = 2;
constexpr int FRAME_GEOS = 2;                                   // tile geometries: 0 = FRAME_TCH rows, 1 = FRAME_TCH5 rows
inline int frame_tile_rows(int geo) { return geo == 1 ? FRAME_TCH5 : FRAME_TCH; }
inline int frame_geo_of(int method) { return method == 5 ? 1 : 0; }
inline int frame_tiles_x(int w) { return (w + 2 * FRAME_TCW - 1) / (2 * FRAME_TCW); }
inline int frame_tiles_y(int h, int geo) { return (h + 2 * frame_tile_rows(geo) - 1) / (2 * frame_tile_rows(geo)); }

// A Bayer cell that holds repaired pixels, as the fused kernel's tile lists name it: the pixel-map entry of each of its four
// pixels (index into the clip's ordered entry list; -1: the pixel keeps the frame's value)
struct CellRec {
    int cell;       // cell column | cell row << 16
    int e[4];       // pixel (x & 1) + 2 * (y & 1)
};

struct PatchView {            // what the fused kernel needs to apply a clip's pixel map (one tile geometry)
    const void *cells;        // int4[nframes][n_rec] {cell, R | G1 << 16, G2 | B << 16, -}: k_pixfix_cells
    int n_rec;
    const int *tile_off;      // CSR over the tiles of one frame: records of the cells that lie in the tile + halo
};

struct PixEntry {
    int pos;        // y * w + x in frame coordinates (-1: not applied)
    int kind;       // 0 skip, 1 cross (interpolate_pixel), 2 along x, 3 along y, 4 copy x+2, 5 copy x-2
    int emit;       // 1: this entry's value is the final value of its position
    int dep[12];    // per tap: index of the entry whose repaired value must be read, or -1
};

struct ThreadCtx;
struct Clip {
    Geom g{};
    int pan_x = 0, pan_y = 0;
    int device = 0;
    std::mutex mu;
    // stripes (mlvfs/stripes.h:30-36)
    int needed = 0;
    int32_t coef[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    // pixel map
    std::vector<int32_t> xy;
    int rules = 0, dual_iso = 0;
    int n_entries = 0, n_levels = 0, n_level0 = 0;       // n_level0: entries without a dependency (they come first)
    DevBuf d_entries;                // PixEntry[n_entries], then {pos, kind | emit << 8} per entry
    DevBuf d_level_off;              // int[n_levels + 1]
    // per tile geometry: the cells with repaired pixels, listed tile by tile (a cell in the halo of a neighbouring tile is
    // listed there too)
    DevBuf d_tile_off[FRAME_GEOS];   // int
    DevBuf d_tile_rec[FRAME_GEOS];   // CellRec
    int n_rec[FRAME_GEOS] = { 0, 0 };
    // One buffer per call holds the patch list {position, value} of every frame and, behind it, the cell values of every
    // frame for the tile geometry in use
    size_t patch_buffer_bytes(int nframes) const
    {
        return (size_t)nframes * ((size_t)n_entries * 8 + (size_t)std::max(n_rec[0], n_rec[1]) * 16) + 16;
    }
    static void *cells_of(void *patches, int n_entries, int nframes)
    {
        return (uint8_t *)patches + ((size_t)nframes * (size_t)n_entries * 8 + 15) / 16 * 16;
    }
    PatchView patch_view(void *patches, int nframes, int geo) const
    {
        return PatchView{ cells_of(patches, n_entries, nframes), n_rec[geo], d_tile_off[geo] };
    }
    DevBuf d_patches, d_scratch;
    // T16 layout of the fused kernel: 0 = not decided yet (from the first frame the clip processes), 1 = plain, 2 = spread
    int t16_layout = 0;
    DevBuf d_unpacked;               // 10 / 12-bit clips: frames unpacked to 16 bits before the fused kernel

    int set_pixel_map(const int32_t *xy, size_t count, int rules, int dual_iso);
    int detect_bad_pixels(const void *d_frame, int aggressive, int dual_iso, hipStream_t stream);
    int fix_pixels(void *d_frames, size_t stride, int nframes, hipStream_t stream);
    // one frame, for callers that SHARE this clip between host threads (drop-in path): nothing of the clip is written --
    // the patch list lives in the calling thread's context, the black level is the frame's
    int fix_pixels_shared(void *d_frame, size_t stride, int black, ThreadCtx *c) const;
    int stripes_compute(const void *d_frame, int frame_size, int rand_mode, hipStream_t stream);
};

// one shard (rows [row0,row1)) of the stripes histogram computation
struct StripesWork {
    static constexpr int RECHECK_CAP = 1 << 16;
    Clip *owner = nullptr;
    Geom g{};
    int row0 = 0, row1 = 0, gpr = 0, n_groups = 0, nblk = 0;
    size_t o_counts = 0, o_bsum = 0, o_boff = 0, o_total = 0, o_hist = 0, o_num = 0, o_nre = 0, o_re = 0, o_copies = 0, bytes = 0;
    uint8_t *base = nullptr;
    int init(Clip *owner, const Geom &g, int row0, int row1);
    int count(const void *d_frame, long long *accepted, hipStream_t stream);
    int hist_dev(const void *d_frame, const void *d_rand, long long n_rand, int *d_hist, int *d_num, hipStream_t stream);
    int recheck_into(int32_t *hist_host_or_null, int *d_hist, hipStream_t stream);
    int hist_to_host(const void *d_frame, const void *d_rand, long long n_rand, int32_t *hist, int32_t num[8],
                     hipStream_t stream);
};

// device-level pixel repair shared by the drop-in symbols and the dual-ISO path (dropin.cpp)
struct ThreadCtx;
bool focus_map_applies(struct frame_headers *fh, ThreadCtx *c, int dual_iso);      // a map file exists and has entries for this frame
// n_patched (optional): entries of the patch list the repair left in c->d_patch ({position or -1, value} each)
int focus_pixels_device(struct frame_headers *fh, ThreadCtx *c, void *d_frame, int dual_iso, bool *changed, int *n_patched = nullptr);
int bad_pixels_device(struct frame_headers *fh, ThreadCtx *c, void *d_frame, int aggressive, int dual_iso, bool *changed, int *n_patched = nullptr);

void glibc_rand_stream(uint16_t *out, size_t n, uint64_t skip, unsigned seed);
int stripes_solve(const int32_t *hist, const int32_t num[8], int frame_size, int32_t coeffs[8]);

// optional HIP-event timing of the dominant kernel (mlvfs_amd_timer_*)
struct KernelTimer {
    std::vector<hipEvent_t> ev;      // pairs: start, stop
    int used = 0;
    bool on = false;
};
KernelTimer &kernel_timer();

// kernel launchers (k_*.hip)
int launch_unpack(const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride, uint32_t first_px,
                  uint32_t npix, int bpp, int nframes, hipStream_t stream);
int launch_frame(const Device *dev, const Geom &g, bool packed, const void *src, size_t src_stride, void *dst,
                 size_t dst_stride, int nframes, int method, const PatchView *pv, bool stripes,
                 const int32_t *coef, hipStream_t stream, bool spread = false);       // spread: T16 layout for dark clips (k_frame.hip)
// tiles that k_frame_p / k_frame_p5 have listed for the list-mode k_frame on `stream` of the current device since the stream's state
// was created, as the launches that have ended reported them (status word 0: k_frame.hip); MLVFS_AMD_ERR_ARG: no such word yet
int stream_listed_tiles(hipStream_t stream, long long *tiles);
// share of sampled pixels of one frame that lie 1 .. 511 above black, in 1/1024 (synchronises the stream)
int dark_share(int packed_bpp, const void *d_frame, int w, int h, int black, hipStream_t stream, int *share_1024);      // packed_bpp 0: 16-bit frames
// does the fused kernel read this packed stream itself (k_frame.hip), or does it take an unpack pass first?
bool frame_kernel_takes(const Geom &g, const void *src, size_t src_stride, const void *dst, size_t dst_stride, int nframes);
// packed: 0 = 16-bit frames, 1 (`true`) = 14-bit stream, else the stream's bits per pixel (12, 10)
int launch_pixfix(int packed, const void *frames, size_t stride, int w, int black, const void *entries,
                  const int *level_off, int n_levels, int n_level0, int n_entries, void *patches, void *scatter,
                  size_t scatter_stride, int nframes, const DeviceLuts &luts, hipStream_t stream);
// both of the above for the fused kernel (one launch when the map is small)
int launch_pixfix_for_frame_kernel(int packed, const void *frames, size_t stride, int w, int h, int black, const void *entries,
                                   const int *level_off, int n_levels, int n_level0, int n_entries, void *patches,
                                   const CellRec *recs, int n_rec, void *cells, int nframes, const DeviceLuts &luts, hipStream_t stream);
// the four pixels of every listed cell after the repair (for the fused kernel): after launch_pixfix, on the same stream
int launch_pixfix_cells(int packed, const void *frames, size_t stride, int w, int h, const CellRec *recs, int n_rec,
                        const void *patches, int n_entries, void *cells, int nframes, hipStream_t stream);
int launch_deflicker_hist(const void *d_frame, uint32_t samples, uint32_t white, unsigned *d_hist, hipStream_t s);
// batches of frames `fstride` bytes apart (k_hdr.hip): the deflicker histograms of every frame in one launch and their medians (the
// reference's 16-bit counters, one workgroup per frame) into d_med[nframes]
int launch_deflicker_batch(const void *d_frames, size_t fstride, int nframes, uint32_t samples, uint32_t white, uint32_t middle, unsigned *d_hist,
                           uint16_t *d_med, hipStream_t s);
// the dual-ISO preview's fit of one frame of a batch (hdr.c:98-176); active = 0: not dual ISO, the frame is left alone
struct HdrPreviewParams {
    double a, b;
    int dark_row_start, shadow, active, pad;
};
int launch_hdr_row_hist_batch(const void *d_frames, size_t fstride, int nframes, int w, int h, int white, unsigned *d_hist, hipStream_t stream);
int launch_hdr_preview_batch(const void *d_frames, void *d_out, size_t fstride, int nframes, int w, int h, int black, int white,
                             const HdrPreviewParams *d_params, size_t shift_count, hipStream_t stream);
// pattern noise on batches (k_pnoise.hip): scratch per frame of a sub-batch, and the 12 launches per sub-batch
size_t pattern_noise_batch_frame_bytes(int w, int h);
// bytes of scratch a batch of pattern noise may use (MLVFS_AMD_PN_SCRATCH_MB, default 256; mlvfs_amd_test_pn_scratch_cap)
size_t pattern_noise_scratch_cap();
int launch_pattern_noise_batch(void *d_frames, size_t fstride, int nframes, int w, int h, int white, void *d_scratch, size_t scratch_bytes,
                               hipStream_t stream);
// the dual-ISO preview of a batch on the device (hdr.cpp): results[f] = 1 converted (written to d_out + f * fstride), 0 not;
// fhs (optional, per frame): the converted frames get the dual-ISO focus-pixel repair before the matching (hdr.c:104)
int hdr_preview_batch_device(ThreadCtx *c, const Geom &g, void *d_frames, void *d_out, size_t fstride, int nframes, size_t max_size,
                             unsigned *d_hist, HdrPreviewParams *d_params, struct frame_headers *fhs, int *results, hipStream_t stream);
// the deflicker medians of a batch (hdr.cpp; synchronises the stream once): med[f] for every frame
int deflicker_batch_device(const void *d_frames, size_t fstride, int nframes, int bpp, size_t size_bytes, void *d_scratch, size_t scratch_bytes,
                           uint16_t *med, hipStream_t stream);
size_t deflicker_batch_scratch_bytes(int bpp, int nframes);
void deflicker_bias(int target, int black_level, uint16_t median, int32_t exposure_bias[2]);
// what a frame's payload is, from its chunk's videoClass (mlv.h:30-31: LZMA 0x80, LJ92 0x100; main.c:573 tests the LZMA flag first)
enum { PAYLOAD_PLAIN = 0, PAYLOAD_LZMA = 1, PAYLOAD_LJ92 = 2 };
inline int payload_kind(uint16_t video_class) { return (video_class & 0x80) ? PAYLOAD_LZMA : (video_class & 0x100) ? PAYLOAD_LJ92 : PAYLOAD_PLAIN; }
// The calibration stage (cal.cpp, k_cal.hip) as the kernels take it: a dark FRAME (a sensor's offset pattern to
// subtract, stage 0; not the "dark clips" of dark_share and the T16 layout, which are low-light footage) and a flat field's Q14 gain
// plane (stage 0b) on the current device; a null plane: that stage is off.  black_d: the dark plane's pedestal; black, top: the black
// level and 2^bpp - 1 of the FRAMES (a dark frame has the frames' depth; a gain plane has none of its own)
struct Calib {
    const uint16_t *d_dark = nullptr;
    int black_d = 0;
    const uint16_t *d_gain = nullptr;
    int black = 0, top = 0;
    bool on() const { return d_dark || d_gain; }
};
// the handles' planes (either may be null) on the calling thread's device, each uploaded on the device's first use, for frames of
// w x h at bpp bits and this black level; a handle of another geometry is refused
int calib_on_device(const mlvfs_amd_dark_t *dark, const mlvfs_amd_flat_t *flat, ThreadCtx *c, int w, int h, int bpp, int black, Calib *out);
bool darkframe_fits(const mlvfs_amd_dark_t *dark, int w, int h, int bpp);
bool flatfield_fits(const mlvfs_amd_flat_t *flat, int w, int h);
// in place, both stages in one pass; packed payloads in, corrected 16-bit frames out
int launch_cal_apply(void *d_frames, size_t stride, uint32_t npix, int nframes, const Calib &cal, hipStream_t stream);
int launch_cal_unpack(const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride, uint32_t npix, int bpp, int nframes,
                      const Calib &cal, hipStream_t stream);
int launch_dark_accum(const void *d_frames, size_t stride, uint32_t npix, int nframes, uint32_t *d_sums, hipStream_t stream);
int launch_dark_mean(const uint32_t *d_sums, uint16_t *d_dark, uint32_t npix, uint32_t n, hipStream_t stream);
int launch_flat_gain(const uint16_t *d_plane, uint32_t w, uint32_t h, int black_f, unsigned long long *d_sums, uint16_t *d_gain,
                     uint32_t *d_means, hipStream_t stream);
// the mount's reader half (mlvreader.cpp): frames of one geometry from the file to 16-bit pixels in HBM.  On return everything that
// reads the reader's staging has ended on s; without `cal` s is drained.  cal: the calibration stage, every frame corrected
// as it arrives -- plain and LZMA payloads inside the unpack pass (s drained on return), LJ92 payloads in a pass behind the decoder
// that may still be in flight on s on return: the caller goes on on s, or synchronises it
// A change of bit depth on the way (the transcoder, mlvfs_amd_mlv_transcode_bits; k_mlvpack.hip): plain and LZMA
// payloads leave the load at out_bpp bits, shifted after the dark frame was subtracted -- as 16-bit frames, or (packed) as packed
// payloads `dstride` bytes apart, ceil(w * h * out_bpp / 16) words each.  LJ92 payloads are not touched by it: their pixels are
// shifted by the pass that follows the decoder (launch_mlv_pack, launch_mlv_tile).
struct LoadBits {
    int out_bpp;
    bool packed;
};
// cal: the calibration stage, both of its halves in one pass: plain and LZMA payloads in launch_cal_unpack, LJ92 payloads in one
// launch_cal_apply behind the decoder.  A gain is not combined with `bits`: the caller shifts afterwards.
int reader_load_batch(const void *reader, int first, int count, int w, int h, int bpp, void *d_frames, size_t dstride, int io_threads,
                      hipStream_t s, const Calib *cal = nullptr);
// the same for frames named one by one (all of one geometry and payload kind); stage_locked: the caller holds reader_stage_mutex
int reader_load_list(const void *reader, const int *list, int count, int w, int h, int bpp, void *d_frames, size_t dstride, int io_threads,
                     hipStream_t s, bool stage_locked, const Calib *cal = nullptr, const LoadBits *bits = nullptr);
// what the transcoder (mlvwriter.cpp) asks of an opened clip: its path and chunk files, where a frame's VIDF block lies, the bytes of
// its payload as read_frames (lj92: as the LJ92 decoder) takes it, packed payloads of plain and LZMA frames (host only), and the
// mutex that serialises the reader's streaming calls
const char *reader_path(const void *reader);
int reader_chunk_fd(const void *reader, int chunk);
bool reader_frame_place(const void *reader, int index, int *chunk, uint64_t *offset);
bool reader_payload_bytes(const void *reader, int index, bool lj92, size_t *bytes);
int reader_read_list(const void *reader, const int *list, int count, uint8_t *dst, size_t stride, int io_threads);
// every block of every chunk in file order, exactly as the reader's own index scan walks them (NULL blocks included):
// visit(chunk, position, tag, block size, the MLVI block's header or nullptr); false ends the walk
void reader_walk_blocks(const void *reader, const std::function<bool(int, uint64_t, const uint8_t *, uint32_t, const mlv_file_hdr_t *)> &visit);
std::mutex &reader_stage_mutex(const void *reader);
// quadrant tiling and bit packing (k_mlvpack.hip), with a change of bit depth inside where one is asked for (d = out_bpp - bpp;
// > 0: << d, < 0: >> -d, 0: none); neither writes its source
int launch_mlv_tile(const void *d_frames, size_t stride, void *d_out, size_t out_stride, int w, int h, int d, int nframes, hipStream_t stream);
int launch_mlv_pack(const void *d_frames, size_t stride, void *d_packed, size_t packed_stride, uint32_t npix, int bpp, int out_bpp, int nframes,
                    hipStream_t stream);
// packed payloads at one depth -> packed payloads or 16-bit frames at another, the dark frame (optional) subtracted on the way
int launch_mlv_repack(const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride, uint32_t npix, int bpp, int out_bpp, int nframes,
                      const Calib *cal, hipStream_t stream);
int launch_mlv_unpack_shift(const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride, uint32_t npix, int bpp, int out_bpp,
                            int nframes, const Calib *cal, hipStream_t stream);
void preload_k_mlvpack();
// half-size Bayer proxies (k_proxy.hip): W' x H' of a w x h frame, false below 4x4 and from 2^27 pixels on; the binning pass
inline bool proxy_geom(int w, int h, int *pw, int *ph)
{
    if (w < 4 || h < 4 || (uint64_t)w * (uint64_t)h >= (1u << 27)) return false;
    *pw = 2 * (w / 4);
    *ph = 2 * (h / 4);
    return true;
}
int launch_bin2(const void *d_frames, size_t stride, void *d_out, size_t out_stride, int w, int h, int nframes, hipStream_t stream);
// rendered half-size sRGB frames (k_render.hip): W' x H' of a w x h frame, false below 2x2 and from 2^27 pixels on; the developing pass
// (d_params: mlvfs_amd_rgb_params' 13 int32 per frame)
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
// the clip's bad-pixel map if it has been detected already (dropin.cpp)
bool cached_bad_clip(struct frame_headers *fh, ThreadCtx *c, int aggressive, std::shared_ptr<Clip> *out);
int cr2hdr20_batch_fh(ThreadCtx *c, struct frame_headers *fh, void *d_frames, size_t img_stride, int nframes, int w, int H, int black14,
                      int white14, int interp_method, int use_fullres, int use_alias_map, int chroma_smooth, int bad_pixels_mode,
                      hipStream_t stream, int *results);
int launch_hist_add(const void *d_frame, uint32_t first, uint32_t step, uint32_t samples, uint32_t white, unsigned *d_hist, hipStream_t s);
int launch_badpix_detect(const void *d_frame, int w, int h, int black, int aggressive, int crop_x, int crop_y,
                         void *d_mask, int words_per_row, int *d_row_count, void *d_list, int cap,
                         const DeviceLuts &luts, hipStream_t stream);
int stripes_groups_per_row(int w);
int launch_stripes_count(const void *d_frame, int w, int row0, int row1, int black, int white, unsigned char *d_counts,
                         int *d_block_sum, long long *d_block_off, long long *d_total, hipStream_t stream);
constexpr int RAND_CHUNK = 31 * 32;      // values per thread of the device generator of the rand() % 1024 stream
int launch_rand_stream(const uint32_t *d_start, const uint32_t *d_pow2, int npow, uint32_t nchunks, uint32_t *d_states, uint16_t *d_out,
                       size_t n, hipStream_t stream);
int rand_stream_device(uint16_t *d_out, size_t n, uint64_t skip, unsigned seed, hipStream_t stream);
size_t stripes_hist_copies_bytes();
int launch_hist_bump(int *d_hist, const int *d_idx, int n, hipStream_t stream);
int launch_stripes_hist(const void *d_frame, int w, int row0, int row1, int black, int white, const unsigned char *d_counts,
                        const long long *d_block_off, const void *d_rand, long long n_rand, int *d_hist, int *d_num,
                        void *d_recheck, int recheck_cap, int *d_n_recheck, void *d_copies, hipStream_t stream);
int launch_stripes_apply(void *d_frames, size_t stride, size_t npix, int w, int black, int white, const int32_t *coef,
                         int nframes, hipStream_t stream);

}  // namespace mlv

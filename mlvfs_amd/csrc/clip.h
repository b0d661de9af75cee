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
bool focus_map_applies(struct frame_headers *fh, ThreadCtx *c, int dual_iso);      // a map file exists and has entries for this frame
// n_patched (optional): entries of the patch list the repair left in c->d_patch ({position or -1, value} each)
int focus_pixels_device(struct frame_headers *fh, ThreadCtx *c, void *d_frame, int dual_iso, bool *changed, int *n_patched = nullptr);
int bad_pixels_device(struct frame_headers *fh, ThreadCtx *c, void *d_frame, int aggressive, int dual_iso, bool *changed, int *n_patched = nullptr);


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
// both of the above for the fused kernel (one launch when the map is small): map's entries and tile lists of geometry `geo`, frames of g
int launch_pixfix_for_frame_kernel(const Clip &map, int geo, const Geom &g, int packed, const void *frames, size_t stride, void *patches,
                                   int nframes, const DeviceLuts &luts, hipStream_t stream);
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
// the rand() % 1024 stream (rand_stream.cpp): a generator state, its words oldest first (next = x[0] + x[28])
struct RandState { uint32_t x[31]; };
int rand_stream_device(uint16_t *d_out, size_t n, uint64_t skip, unsigned seed, hipStream_t stream);
// n values from state `s0` on; *after, if wanted: the state behind them
int rand_stream_device_from(const RandState &s0, uint16_t *d_out, size_t n, hipStream_t stream, RandState *after);
size_t stripes_hist_copies_bytes();
int launch_hist_bump(int *d_hist, const int *d_idx, int n, hipStream_t stream);
int launch_stripes_hist(const void *d_frame, int w, int row0, int row1, int black, int white, const unsigned char *d_counts,
                        const long long *d_block_off, const void *d_rand, long long n_rand, int *d_hist, int *d_num,
                        void *d_recheck, int recheck_cap, int *d_n_recheck, void *d_copies, hipStream_t stream);
int launch_stripes_apply(void *d_frames, size_t stride, size_t npix, int w, int black, int white, const int32_t *coef,
                         int nframes, hipStream_t stream);

}  // namespace mlv

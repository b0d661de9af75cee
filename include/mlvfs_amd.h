/*
 * mlvfs_amd.h -- C ABI of libmlvfs_amd.so, the MI355X (gfx950) implementation of
 * MLVFS's per-frame raw-processing path.  Plain pointers and sizes only.
 *
 * PART 1 -- drop-in symbols.  Same names, prototypes, ownership and error
 *   behaviour as the reference's dng.o / cs.o / stripes.o / hdr.o / histogram.o /
 *   patternnoise.o for the hot path, so MLVFS's unchanged main.c links against
 *   this library instead (the binding a maintainer adds is shown in
 *   INTEGRATION.md).  They work IN PLACE ON HOST MEMORY and are synchronous:
 *   each call stages the frame to the GPU, runs the HIP kernels and copies back.
 *   Any HIP failure is reported on stderr and returns the reference's failure
 *   value (0 / no-op) -- there is NO CPU fallback in this library.
 *
 * PART 2 -- device-resident API (mlvfs_amd_*).  The same stages on frames that
 *   already live in HBM, batched over many frames per launch, plus the fused
 *   steady-state pipeline.  This is what bench.py times and what a frame
 *   prefetcher would call.  All device calls are asynchronous
 *   on the given hipStream_t (passed as void*; NULL = HIP's default stream)
 *   unless stated otherwise.
 */
#ifndef MLVFS_AMD_H
#define MLVFS_AMD_H

#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>

#include "mlvfs_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ======================================================================== */
/* PART 1: drop-in symbols                                                   */

/* replaces mlvfs/dng.h:31 (dng.c:854-872): unpack bpp-bit packed pixels to u16 */
size_t dng_get_image_data(struct frame_headers *frame_headers, uint16_t *packed_bits,
                          uint8_t *output_buffer, off_t offset, size_t max_size);
/* replaces mlvfs/dng.h:29 (dng.c:597-789): the 65536-byte CinemaDNG header (TIFF IFD0 + EXIF IFD) of one frame,
 * built on the host from the MLV block headers; copies min(max_size, 65536) bytes starting at `offset` and returns
 * that count.  May rewrite frame_headers->rawi_hdr.raw_info.active_area like the reference does.  Host only:
 * works without a HIP device.                                                       */
size_t dng_get_header_data(struct frame_headers *frame_headers, uint8_t *output_buffer, off_t offset, size_t max_size,
                           double fps_override, char *mlv_basename);
/* dng_get_header_data for a frame whose strip is one lossless-JPEG stream of stream_bytes bytes: the same 65536 bytes except the
 * value fields of two IFD0 entries, Compression (259) = 7 and StripByteCounts (279) = stream_bytes.  BitsPerSample stays 16 (the
 * stream's precision), StripOffsets 65536, one strip.  Host code.                                                              */
size_t mlvfs_amd_dng_header_lossless(struct frame_headers *frame_headers, uint8_t *output_buffer, off_t offset, size_t max_size,
                                     double fps_override, const char *mlv_basename, uint32_t stream_bytes);
/* replaces mlvfs/dng.h:30,32,33 (dng.c:797-800, 879-891) */
size_t dng_get_header_size(void);
size_t dng_get_image_size(struct frame_headers *frame_headers);
size_t dng_get_size(struct frame_headers *frame_headers);

/* replaces mlvfs/cs.h:27-30 (cs.c:49-84, 220-331, 336-503) */
void chroma_smooth(struct frame_headers *frame_headers, uint16_t *image_data, int method);
void fix_bad_pixels(struct frame_headers *frame_headers, uint16_t *image_data, int aggressive, int dual_iso);
void fix_focus_pixels(struct frame_headers *frame_headers, uint16_t *image_data, int dual_iso);
void free_focus_pixel_maps(void);

/* replaces mlvfs/stripes.h:30-43 (stripes.c:29-266) */
struct stripes_correction {
    struct stripes_correction *next;
    char *mlv_filename;
    int correction_needed;
    int coeffficients[8];          /* sic: the reference's spelling is part of the ABI */
};
struct stripes_correction *stripes_get_correction(const char *mlv_filename);
struct stripes_correction *stripes_new_correction(const char *mlv_filename);
void stripes_free_corrections(void);
void stripes_compute_correction(struct frame_headers *frame_headers, struct stripes_correction *correction,
                                uint16_t *image_data, off_t offset, size_t size);
void stripes_apply_correction(struct frame_headers *frame_headers, struct stripes_correction *correction,
                              uint16_t *image_data, off_t offset, size_t size);

/* replaces mlvfs/hdr.h:27 (hdr.c:40-227): fast dual-ISO preview; 1 = converted */
int hdr_convert_data(struct frame_headers *frame_headers, uint16_t *image_data, off_t offset, size_t max_size);

/* replaces mlvfs/hdr.h:28 (hdr.c:1932-1957): full dual-ISO conversion (cr2hdr 20-bit).
 * Every configuration main.c can ask for is built: interp_method 0 (AMaZE + edge-directed interpolation, --amaze-edge) and
 * 1 (mean23), fullres / alias map on or off, chroma_smooth 0 / 2 / 3 / 5 (any other value only logs, like hdr.c:1915-1927),
 * fix_bad_pixels_mode 0 / 1 / 2 (focus + bad pixel repair in dual-ISO mode first, hdr.c:1784-1790).  Returns 1 when the
 * frame was converted (levels in frame_headers are then multiplied by 4, hdr.c:1949-1950), 0 when the frame is not dual ISO
 * or cannot be converted -- a width that is not a multiple of 4 with interp_method 0 has no defined result in the
 * reference's SSE2 AMaZE and is refused --; the frame is then left untouched.                          */
int cr2hdr20_convert_data(struct frame_headers *frame_headers, uint16_t *image_data, int interp_method, int fullres,
                          int use_alias_map, int chroma_smooth, int fix_bad_pixels_mode);

/* replaces mlvfs/patternnoise.h:16 (patternnoise.c:357-380) */
void fix_pattern_noise(int16_t *raw, int w, int h, int white, int debug_flags);

/* replaces mlvfs/histogram.h:26-36 (histogram.c:33-84); host-side helper used by
 * main.c's deflicker (main.c:895-906)                                         */
struct histogram { uint16_t white; uint32_t count; uint16_t *data; };
struct histogram *hist_create(uint16_t white);
void hist_add(struct histogram *hist, uint16_t *data, uint32_t size, uint16_t skip);
uint16_t hist_median(struct histogram *hist);
void hist_destroy(struct histogram *hist);

/* Imported from the caller when present (weak): mlvfs/mlvfs.h:90-92, defined in
 * main.c:128-196.  When the caller provides them the device tables are built
 * from the caller's arrays; otherwise from the same formulas with the host libm. */
int *get_raw2ev(int black);
int *get_ev2raw(void);

/* ======================================================================== */
/* PART 2: device-resident API                                               */

#define MLVFS_AMD_OK            0
#define MLVFS_AMD_ERR_HIP      -1     /* a HIP call failed (see mlvfs_amd_last_error) */
#define MLVFS_AMD_ERR_ARG      -2     /* bad geometry / argument                      */
#define MLVFS_AMD_ERR_LUT      -3     /* host libm tables fail the compression check  */
#define MLVFS_AMD_ERR_NOMEM    -4
#define MLVFS_AMD_ERR_IO       -5     /* a file could not be created, read or written (mlvfs_amd_mlv_transcode) */

typedef struct {
    int32_t width, height;        /* rawi_hdr.xRes / yRes                         */
    int32_t bpp;                  /* raw_info.bits_per_pixel                       */
    int32_t black, white;         /* raw_info.black_level / white_level            */
    int32_t pan_x, pan_y;         /* vidf_hdr.panPosX / panPosY (pixel-map crop)   */
} mlvfs_amd_geom_t;

/* context: one per (host thread, device); created lazily */
int         mlvfs_amd_device_count(void);
/* PCI bus id ("0000:c1:00.0") of visible device `device` into out (len >= 16): the physical card, whatever the enumeration order;
 * and the device the calling thread is bound to (-1: not yet).  Threads that do not choose a device (mlvfs_amd_init) are spread
 * round-robin over the visible GPUs in the order of their PCI bus ids; the mapping is printed once (MLVFS_AMD_QUIET=1: not). */
int mlvfs_amd_device_pci_bus_id(int device, char *out, int len);
int mlvfs_amd_thread_device(void);
int         mlvfs_amd_init(int device);              /* binds the calling thread to `device` */
const char *mlvfs_amd_last_error(void);
const char *mlvfs_amd_version(void);

/* per-clip artefacts: stripe coefficients + ordered pixel map.
 * A handle also owns scratch that its calls reuse (the per-frame patch lists of the pixel repair): calls on ONE handle must
 * be ordered -- issue them on one stream, or serialise them --; to process one clip on several streams at once create a
 * handle per stream and give each the same stripes / pixel map.  (The drop-in symbols of PART 1 do that themselves: the
 * maps they cache per clip are shared read-only between libfuse's worker threads, each thread repairs into its own buffers.) */
typedef struct mlvfs_amd_clip mlvfs_amd_clip_t;
mlvfs_amd_clip_t *mlvfs_amd_clip_create(const mlvfs_amd_geom_t *geom);
void   mlvfs_amd_clip_destroy(mlvfs_amd_clip_t *clip);
int    mlvfs_amd_clip_set_stripes(mlvfs_amd_clip_t *clip, int needed, const int32_t coeffs[8]);
int    mlvfs_amd_clip_get_stripes(const mlvfs_amd_clip_t *clip, int *needed, int32_t coeffs[8]);
/* Layout of the raw2ev table inside the fused kernel: 0 = decide from the first frame this clip processes with
 * chroma smoothing (default; one stream synchronisation), 1 = plain, 2 = spread (dark footage).  Results are identical.   */
int    mlvfs_amd_clip_set_t16_layout(mlvfs_amd_clip_t *clip, int layout);
int    mlvfs_amd_clip_get_t16_layout(const mlvfs_amd_clip_t *clip);
/* xy = count (x,y) pairs in sensor coordinates (crop offsets included), list order
 * is application order.  kind: 0 = bad-pixel rules (cs.c:314-330), 1 = focus-pixel
 * rules incl. edges (cs.c:463-500).                                            */
int    mlvfs_amd_clip_set_pixel_map(mlvfs_amd_clip_t *clip, const int32_t *xy, size_t count, int kind, int dual_iso);
size_t mlvfs_amd_clip_get_pixel_map(const mlvfs_amd_clip_t *clip, int32_t *xy, size_t cap);

/* -- single stages on device frames ---------------------------------------- */
/* frames are `nframes` buffers spaced by the given strides (bytes)           */
int mlvfs_amd_unpack_dev(const mlvfs_amd_geom_t *geom, const void *d_packed, size_t packed_stride,
                         void *d_out, size_t out_stride, int nframes, void *stream);
/* the inverse of mlvfs_amd_unpack_dev (csrc/k_mlvpack.hip): 16-bit frames -> packed payloads of geom->bpp bits (1..16), pixel i in
 * bits [i * bpp, (i + 1) * bpp) of an MSB-first stream of little-endian 16-bit words.  Exactly ceil(width * height * bpp / 16) words
 * are written per frame -- the unused low bits of the last word are zero, nothing behind it is touched --; pixels are masked to bpp
 * bits.  14 / 12 / 10 bits with width * height a multiple of 16, d_frames 16-byte and d_packed 4-byte aligned (strides likewise)
 * take the fast form: 16 pixels in, bpp / 2 dwords out per lane.                                                             */
int mlvfs_amd_pack_dev(const mlvfs_amd_geom_t *geom, const void *d_frames, size_t stride, void *d_packed, size_t packed_stride,
                       int nframes, void *stream);
int mlvfs_amd_chroma_smooth_dev(const mlvfs_amd_geom_t *geom, const void *d_in, void *d_out, size_t stride,
                                int method, int nframes, void *stream);
/* detection on one frame; fills the clip's pixel map (synchronises the stream) */
int mlvfs_amd_detect_bad_pixels_dev(mlvfs_amd_clip_t *clip, const void *d_frame, int aggressive, void *stream);
/* ordered repair with the clip's pixel map, in place                         */
int mlvfs_amd_fix_pixels_dev(mlvfs_amd_clip_t *clip, void *d_frames, size_t stride, int nframes, void *stream);
/* stripes: histogram of rows [row0,row1) of one frame.
 *   count pass  -> number of accepted add_pixel calls (synchronises)
 *   hist  pass  -> adds into d_hist (int32[8][65536]) and d_num (int32[8]);
 *                  d_rand = device array of rand()%1024 values (uint16), entry
 *                  2*k and 2*k+1 belong to this shard's k-th accepted call     */
int mlvfs_amd_stripes_count_dev(const mlvfs_amd_geom_t *geom, const void *d_frame, int row0, int row1,
                                int64_t *accepted, void *stream);
int mlvfs_amd_stripes_hist_dev(const mlvfs_amd_geom_t *geom, const void *d_frame, int row0, int row1,
                               const void *d_rand, int64_t n_rand, void *d_hist, void *d_num, void *stream);
/* host: histograms -> coefficients (stripes.c:207-246); coeffs of under-filled
 * histograms are left as passed in                                           */
int mlvfs_amd_stripes_solve(const int32_t *hist, const int32_t num[8], int frame_size, int32_t coeffs[8]);
/* whole computation for one device frame into the clip.  rand_mode 0: consume
 * libc rand() like the reference; 1: private glibc-compatible stream, seed 1   */
int mlvfs_amd_stripes_compute_dev(mlvfs_amd_clip_t *clip, const void *d_frame, int frame_size, int rand_mode,
                                  void *stream);
int mlvfs_amd_stripes_apply_dev(const mlvfs_amd_clip_t *clip, void *d_frames, size_t stride, int nframes,
                                void *stream);
/* glibc TYPE_3 rand() restatement: out[i] = rand()%1024 for calls skip..skip+n-1
 * after srand(seed)                                                            */
void mlvfs_amd_rand_stream(uint16_t *out, size_t n, uint64_t skip, unsigned seed);
/* the same values generated on the device into d_out (16-byte aligned device memory); synchronises the stream */
int mlvfs_amd_rand_stream_dev(void *d_out, size_t n, uint64_t skip, unsigned seed, void *stream);

/* -- fused steady-state pipeline (process_frame order, main.c:942-997) ------ */
/* packed 14-bit stream -> [pixel map repair] -> [chroma smooth] -> [stripes
 * apply] -> 16-bit frames, one pass over HBM (3.75 B/px).  Stages are enabled
 * by cs_method (0,2,3,5), fix_pixels and apply_stripes (uses the clip state).
 * Clips of another bit depth (10, 12, ... bits: geom.bpp) are unpacked to 16 bits first and then take the kernel's
 * 16-bit input path (one more pass over HBM).                                */
int mlvfs_amd_process_frames_dev(mlvfs_amd_clip_t *clip, const void *d_packed, size_t packed_stride,
                                 void *d_out, size_t out_stride, int nframes,
                                 int cs_method, int fix_pixels, int apply_stripes, void *stream);

/* The same stages on frames that are already 16-bit pixels in HBM (e.g. decoded LJ92 payloads); d_out != d_frames. */
int mlvfs_amd_process_unpacked_dev(mlvfs_amd_clip_t *clip, const void *d_frames, size_t stride, void *d_out, size_t out_stride,
                                   int nframes, int cs_method, int fix_pixels, int apply_stripes, void *stream);

/* The same fused pipeline for frames in HOST memory (a reader that has MLV payloads in RAM): chunks
 * of chunk_frames frames (<= 0: 8) travel H2D -> kernels -> D2H on three streams so that both copy directions and the
 * kernels overlap; returns when h_out is complete.  Strides are bytes between frames.  Full PCIe speed needs page-locked
 * buffers (mlvfs_amd_host_alloc, or memory the caller registered with the HIP runtime); pageable memory works, slower. */
int mlvfs_amd_process_frames_host(mlvfs_amd_clip_t *clip, const void *h_packed, size_t packed_stride, void *h_out,
                                  size_t out_stride, int nframes, int cs_method, int fix_pixels, int apply_stripes,
                                  int chunk_frames);
/* Page-locked buffers, pooled: a freed buffer is kept (up to 2 GiB in all) and handed out again for the next request of its
 * size, so a host may allocate and free one per frame like process_frame does with malloc (main.c:931).  With frame buffers
 * from here the drop-in symbols of PART 1 copy at the link's speed instead of the pageable path's. */
void *mlvfs_amd_host_alloc(size_t bytes);
/* Gives the buffer back to the pool.  A pointer that did not come from mlvfs_amd_host_alloc, and a buffer freed a second time,
 * are reported on stderr and otherwise ignored (the library frees nothing it does not own). */
void mlvfs_amd_host_free(void *p);
/* 1 when [p, p + bytes) lies inside a live buffer of mlvfs_amd_host_alloc (page-locked and mapped: the GPU can address it), else 0 */
int mlvfs_amd_host_owns(const void *p, size_t bytes);
/* bytes from p to the end of the live mlvfs_amd_host_alloc buffer that holds it (its size rounded up to 64 KiB); 0: in none */
size_t mlvfs_amd_host_size(const void *p);
/* is p inside any buffer mlvfs_amd_host_alloc has handed out, live or already freed?  (the allocation shim's free(): a second free of a
 * pool buffer goes back to the pool, which reports it, never to the C library) */
int mlvfs_amd_host_knows(const void *p);
/* Returns the pool's cached (free) buffers to the runtime; result: bytes released. */
size_t mlvfs_amd_host_trim(void);

/* -- LJ92 payloads ---------------------------------------- */
/* Lossless-JPEG frames of a compressed clip (MLV_VIDEO_CLASS_FLAG_LJ92; main.c:617-681: lj92_open + lj92_decode + the
 * untiling loop) decoded on the GPU.  streams[i] / sizes[i]: frame i's JPEG stream in HOST memory (the VIDF payload
 * behind its 4-byte size word); output: xres x yres 16-bit pixels per frame at d_out + i * out_stride, in the layout
 * dng_get_image_data produces, ready for the stages above.  One component, one Huffman table, predictors 0..7, like the
 * reference's decoder (6, what MLV writers use, and 1 are the fast ones).  Synchronises `stream` before returning.  dims of mlvfs_amd_lj92_info:
 * {width, height, bits, predictor} of the JPEG itself.                                                             */
int mlvfs_amd_lj92_info(const void *stream, size_t size, int dims[4]);
int mlvfs_amd_lj92_decode_dev(const void *const *streams, const size_t *sizes, int nframes, int xres, int yres,
                              void *d_out, size_t out_stride, void *stream);

/* Test hook, host only: the LDS of the decoder's row kernel (csrc/lj92.h: lj_row_plan, the one rule its launcher and the kernel
 * share) for a row of w values in a launch whose widest frame has max_w, 1 <= w <= max_w <= 65535.  out[4] = {1 if the row is staged
 * in LDS (0: worked on in place in global memory), byte offset of the staged row behind the carries, byte offset up to which a staged
 * row reaches, LDS bytes of the launch}.  0, or MLVFS_AMD_ERR_ARG.                                                              */
int mlvfs_amd_test_lj92_row_plan(int w, int max_w, long long out[4]);

/* The reference decoder's own three calls (lj92.h:40-58), what get_image_data makes of an LJ92 frame (main.c:626-647: lj92_open,
 * lj92_decode into a temporary buffer, then its own untiling loop): with them `lj92.o` can leave MLVFS's link too and the decode
 * runs on the GPU.  Values in the decoder's own order, width x height of the JPEG.  Only what MLVFS passes is supported:
 * skiplen 0, linearize NULL (anything else: LJ92_ERROR_CORRUPT, -1).                                                 */
typedef struct _ljp *lj92;
int lj92_open(lj92 *lj, uint8_t *data, int datalen, int *width, int *height, int *bitdepth);
void lj92_close(lj92 lj);
int lj92_decode(lj92 lj, uint16_t *target, int tlen, int skiplen, uint16_t *linearize, int linlen);
/* The reference's encoder (lj92.h:65-68, lj92.c:711-1144; nothing in MLVFS calls it -- it completes the export table of lj92.o):
 * a width x height tile read from `image` in runs of readLength values skipLength apart, optionally through a delinearisation
 * table, written as one-component lossless JPEG with predictor 6 -- byte for byte the reference's stream, its peculiar Huffman
 * table included (csrc/lj92enc.cpp).  *encoded is malloc'd, the caller frees it.  Host memory in and out; histogram, bit packing
 * and byte stuffing run on the GPU (csrc/k_lj92enc.hip).  Returns 0, LJ92_ERROR_NO_MEMORY (-2), or LJ92_ERROR_CORRUPT (-1) where
 * the reference would leave its own arrays (17-bit differences, all 17 classes in use, values beyond the table) or HIP fails. */
int lj92_encode(uint16_t *image, int width, int height, int bitdepth, int readLength, int skipLength,
                uint16_t *delinearize, int delinearizeLength, uint8_t **encoded, int *encodedLength);
/* Optional (needs three changed lines in main.c): lj92_decode plus the untiling loop get_image_data runs behind it
 * (main.c:646-667: 8-22 ms per 3584x1320 frame on a host core) in one call: xres x yres pixels in host memory, decoded and untiled
 * on the GPU.  0, or the lj92.h error codes.                                                                             */
int mlvfs_amd_lj92_decode_untiled(lj92 lj, uint16_t *dst, int xres, int yres);
/* host-only test hook: the encoder's Huffman table for a histogram of the 17 classes; out[68] = bits[1..16], number of DHT
 * values, the 17 values, then length and code per class.  0, or -1 (error string set) where lj92_encode would refuse.          */
int mlvfs_amd_lj92_encode_table(const uint32_t hist[17], int npix, int *out);
/* Test hook, host only: how the encoder's kernels cut a frame of npix pixels, 1 <= npix < 2^27 (csrc/lj92enc.h, the constants the
 * kernels are built with).  out[4] = {pixels per block, blocks of the frame, threads of the workgroup that scans a frame's block
 * offsets, blocks each of its threads sums}.  0, or MLVFS_AMD_ERR_ARG.                                                          */
int mlvfs_amd_test_lj92_encode_plan(long long npix, long long out[4]);
/* The same encoder on a batch of frames that already lie in device memory: nframes frames of width x height uint16 values, `stride`
 * bytes apart, each to the COMPLETE stream (SOI .. EOI) lj92_encode writes for it with readLength = width * height, skipLength 0 and
 * no delinearisation table, at d_out + f * out_stride (device memory, 4-byte aligned, out_stride a multiple of 4).  One launch
 * sequence and one host round trip (the Huffman tables) serve the batch.  lengths[f]: bytes of the stream; status[f]: one of
 * MLVFS_AMD_LJ92ENC_*; max_class[f] (optional): the highest difference class SSSS in use, 17 for a 17-bit difference.  A frame the
 * reference cannot encode inside its arrays, or whose stream is longer than out_stride, says so in status[f] (length 0, its part of
 * d_out undefined) and does not disturb the others.  Class 16 is encoded as the reference encodes it, with 16 value bits behind the
 * code, which the JPEG standard does not do: callers that write files for other decoders check max_class.  Synchronises `stream`. */
#define MLVFS_AMD_LJ92ENC_OK      0
#define MLVFS_AMD_LJ92ENC_DIFF17  1     /* a difference of 17 bits */
#define MLVFS_AMD_LJ92ENC_TABLE   2     /* all 17 classes in use, or a Huffman code longer than 16 bits */
#define MLVFS_AMD_LJ92ENC_NOFIT   3     /* the stream is longer than out_stride */
int mlvfs_amd_lj92_encode_batch_dev(const void *d_frames, size_t stride, int nframes, int width, int height, int bitdepth, void *d_out,
                                    size_t out_stride, uint32_t *lengths, int *status, int *max_class, void *stream);
/* What an MLV writer hands to that encoder: the four Bayer channels of a frame as the four quadrants of one image, the inverse of
 * get_image_data's untiling loop (main.c:656-667).  Tiled row y, column x holds source pixel (ty, tx), ty = (2y) % H + (2y) / H,
 * tx = (2x) % W + (2x) / W.  nframes frames of width x height 16-bit pixels `stride` bytes apart -> the same at d_out, out_stride
 * bytes apart; d_out != d_frames.  For an odd width or height the reference's map is no bijection (H = 5: rows 1 and 3 are never
 * written): refused.  A width that is a multiple of 8 with 16-byte aligned buffers and strides takes the fast form.              */
int mlvfs_amd_lj92_tile_dev(const void *d_frames, size_t stride, void *d_out, size_t out_stride, int width, int height, int nframes,
                            void *stream);

/* -- LZMA payloads ----------------------------------------- */
/* One VIDF payload of an LZMA-compressed clip (MLV_VIDEO_CLASS_FLAG_LZMA; main.c:598-616): [u32 size of the packed frame][5 LZMA
 * property bytes][LZMA stream] -> the packed frame, exactly what LzmaUncompress leaves in lzma_out for dng_get_image_data.  Host
 * code (the entropy decoding of a frame is one serial chain; the reader decodes one frame per thread): no HIP device needed.
 * Returns 0 and the decoded size, or LzmaDecode's error code (1 data, 4 unsupported properties, 6 input ends early), or
 * MLVFS_AMD_ERR_ARG when the buffer is smaller than the size word says.                                             */
int mlvfs_amd_lzma_uncompress(const void *payload, size_t size, void *dst, size_t dst_cap, size_t *out_size);

/* -- MLV container reader and prefetcher (host code) -------- */
/* Opens <name>.MLV and its chunks .M00, .M01, ... (index.c:367-424) and builds, once, what MLVFS rebuilds for every
 * frame it serves: the XREF index (index.c:216-341; use_idx_file != 0: taken from <name>.IDX when that exists, written
 * there otherwise, like get_index) and the block headers that belong to each video frame (main.c:429-558).  NULL on
 * failure.  Needs no HIP device except for mlvfs_amd_mlv_process.                                                     */
void  *mlvfs_amd_mlv_open(const char *mlv_path, int use_idx_file);
void   mlvfs_amd_mlv_close(void *reader);
int    mlvfs_amd_mlv_frame_count(const void *reader);            /* = mlv_get_frame_count, index.c:488-527 */
int    mlvfs_amd_mlv_chunk_count(const void *reader);
/* the XREF block (header + entries) exactly as make_index builds it; returns its size, copies if cap suffices */
size_t mlvfs_amd_mlv_xref(const void *reader, void *dst, size_t cap);
/* = mlv_get_frame_headers(path, index, out): 1 = found and a RAWI block precedes it, 0 otherwise */
int    mlvfs_amd_mlv_frame_headers(const void *reader, int index, struct frame_headers *out);
/* payloads of `count` frames (uncompressed clips) into dst, `stride` bytes apart, read by io_threads threads (<= 0: 8) */
int    mlvfs_amd_mlv_read_frames(const void *reader, int first, int count, void *dst, size_t stride, int io_threads);
/* file -> fused pipeline -> h_out: batches of batch_frames frames (<= 0: 32) are read into page-locked staging by
 * io_threads threads while the previous batch goes through mlvfs_amd_process_frames_host (LJ92 clips: through the GPU
 * decoder and mlvfs_amd_process_unpacked_dev).  `clip` must have the frames' geometry; a reader's staging and device buffers
 * belong to the device of the thread that first streams from it.                                                     */
int    mlvfs_amd_mlv_process(const void *reader, mlvfs_amd_clip_t *clip, int first, int count, void *h_out, size_t out_stride,
                             int cs_method, int fix_pixels, int apply_stripes, int batch_frames, int io_threads);
/* A DUAL-ISO clip, file -> batched full conversion -> h_out (main.c:942 + 956-959 per frame, cr2hdr20 with the headers' levels):
 * batches of batch_frames frames (<= 0: 8) are read while the previous batch is unpacked and converted in ONE submission
 * (mlvfs_amd_cr2hdr20_batch_dev) and the batch before travels back.  results[i] = 1: frame first + i converted (black and white
 * level 4x the headers'), 0: no dual-ISO frame, h_out holds it unpacked.  Plain and LZMA clips. */
int    mlvfs_amd_mlv_process_dualiso(const void *reader, int first, int count, void *h_out, size_t out_stride, int interp_method,
                                     int fullres, int use_alias_map, int chroma_smooth, int batch_frames, int io_threads, int *results);
/* An opened clip, whatever its payloads are (plain, LZMA, LJ92), written again as an MLV with lossless-JPEG payloads (what
 * `mlv_dump -c` writes) or plain packed ones (`-d`) -- csrc/mlvwriter.cpp.  out_path ends in .MLV; source chunk i (.M00, ...) becomes
 * out_path with its last two characters replaced by the chunk's number.  Every output chunk holds its source chunk's blocks in the
 * source's file order, byte for byte, except: MLVI gets MLV_VIDEO_CLASS_FLAG_LJ92 (0x100) set or cleared and the LZMA flag (0x80)
 * cleared; VIDF keeps its header with frameSpace = 0 and blockSize = header + payload; NULL and XREF blocks are dropped; no .IDX is
 * written.  An LJ92 payload is [u32 = w * h * 2][the stream lj92_encode writes for the quadrant-tiled frame as one component of
 * w x h at bits_per_pixel precision] with nothing behind it; a plain one is ceil(w * h * bpp / 16) words.  Frames go through the GPU
 * in batches of batch_frames (<= 0: 8) frames of one geometry, in a chunk's file order: decode / unpack, mlvfs_amd_lj92_tile_dev and
 * the batch encoder, or (LJ92 to plain) mlvfs_amd_pack_dev.  Plain output of a plain or LZMA clip is host code and needs no HIP device.
 * MLVFS_AMD_ERR_ARG before any device work: a null argument, an out_path that does not end in .MLV / .mlv or names a file of the
 * source, an output file or <stem>.IDX that exists (nothing is overwritten), a video class other than raw or with the DELTA flag,
 * LJ92 output of a frame of odd width or height.  A frame the encoder cannot encode inside the reference's arrays, or one with a
 * difference of class 16 (the reference then writes value bits the JPEG standard does not have), fails the call; the error names the
 * frame.  A source block that cannot be read in full and an output file that cannot be created, written or closed are
 * MLVFS_AMD_ERR_IO.  After any failure none of the call's output files are left.  stats: {video frames written, payload bytes in the source,
 * payload bytes written, files written}.  Calls on one reader are serialised with its other streaming calls.                      */
#define MLVFS_AMD_MLV_PLAIN 0
#define MLVFS_AMD_MLV_LJ92  1
int    mlvfs_amd_mlv_transcode(const void *reader, const char *out_path, int payload, int batch_frames, int io_threads, long long stats[4]);

/* -- animated GIF preview (gif.c:82-244) ---------------------- */
/* = gif_get_size: size of the preview file of a clip with these frame headers                                        */
size_t mlvfs_amd_gif_size(const struct frame_headers *frame_headers);
/* The preview of 10 frames (host memory, `stride` bytes apart: packed payloads of geom->bpp bits with one word of slack behind
 * each when packed != 0, else 16-bit frames): the pixel picking and the gamma map run on the GPU, the file's framing on the host;
 * file receives mlvfs_amd_gif_size bytes, byte for byte what gif_get_data builds.  packed == 2: only the rows the preview reads
 * (it picks ONE pixel of every 4x4 block, gif.c:197): yres / 4 row pieces per frame, stride / (yres / 4) bytes each, piece y
 * starting at the 16-bit word of the payload that holds pixel y * 4 * (xres / 4 * 4) + 1 (mlvfs_amd_mlv_gif_data reads just those
 * from an uncompressed clip: a quarter of the file).                                                                  */
int mlvfs_amd_gif_render(const mlvfs_amd_geom_t *geom, const void *h_frames, size_t stride, int packed, int nframes, uint8_t *file);
/* = gif_get_data on an opened clip (frames k * count / 10, k = 0..9; uncompressed, LZMA and LJ92 clips): copies
 * min(max_size, size - offset) bytes from `offset` on, returns max_size (0 on failure).                              */
size_t mlvfs_amd_mlv_gif_data(const void *reader, uint8_t *output_buffer, off_t offset, size_t max_size);
/* gif.h:27-28, the two calls MLVFS makes for a clip's _PREVIEW.GIF (main.c:1018-1022, 1212): gif_get_data opens the clip at `path`
 * with the library's reader and is mlvfs_amd_mlv_gif_data on it; with them `gif.o` can leave the link too.             */
size_t gif_get_data(const char *path, uint8_t *output_buffer, off_t offset, size_t max_size);
size_t gif_get_size(struct frame_headers *frame_headers);

/* dual-ISO preview on one device frame (hdr.c:40-227); returns 1 / 0 / <0    */
int mlvfs_amd_hdr_preview_dev(const mlvfs_amd_geom_t *geom, void *d_frame, size_t max_size, void *stream);

/* deflicker of main.c:895-906 on one device frame: the median of every second pixel (the reference's
 * 16-bit histogram counters included) against `target` -> raw_info.exposure_bias = {(int)(log2(...) * 10000), 10000}, which
 * dng_get_header_data writes as BaselineExposure.  size_bytes: the frame's size in bytes, as main.c:943 passes it.
 * Synchronises the stream.                                                                                        */
int mlvfs_amd_deflicker_dev(const mlvfs_amd_geom_t *geom, const void *d_frame, size_t size_bytes, int target,
                            int32_t exposure_bias[2], void *stream);

/* full dual-ISO conversion of one device frame, in place (hdr.c:1774-1957 without the
 * pixel-map repairs); returns 1 converted / 0 not dual ISO or not convertible / <0 error.
 * mlvfs_amd_dualiso_reset forgets the per-black-level table caches (a fresh process).  */
int mlvfs_amd_cr2hdr20_dev(const mlvfs_amd_geom_t *geom, void *d_frame, int interp_method, int fullres, int use_alias_map,
                           int chroma_smooth, void *stream);
/* The same for `nframes` frames of one clip geometry, `stride` bytes apart, in ONE submission: every stage is launched once for the
 * whole batch (the frame index is a grid dimension; AMaZE runs nframes x 319 tiles at 3584x1320 instead of 319 with a two-tile
 * tail), the integer decisions of hdr.c:441-636, 250-300 and 638-772 (pattern, bright / dark fields, white levels, order
 * statistics, highlight rows, slope fit) are made by single-workgroup kernels, and ONE host round trip per batch remains -- the
 * libm scalars (log2 of the fitted slope and of the levels) and the reference's progress lines -- plus the final wait.
 * results[f] (host memory) = 1 converted / 0 left alone (not dual ISO, detection failed), like the reference's return value
 * frame by frame; the function returns 0, or < 0 on an error of the library.  Frames are processed as if in order: the table caches
 * take the white level of the first frame that converts (hdr.c:1080,1240,1575,1672).  Work memory: ~0.93 GB per 3584x1320 frame
 * of the batch with the AMaZE interpolation, kept by the calling thread. */
int mlvfs_amd_cr2hdr20_batch_dev(const mlvfs_amd_geom_t *geom, void *d_frames, size_t stride, int nframes, int interp_method,
                                 int fullres, int use_alias_map, int chroma_smooth, int *results, void *stream);
void mlvfs_amd_dualiso_reset(void);
/* gives back the dual-ISO work memory the calling thread holds (it grows with the largest batch and is otherwise kept until the
 * thread ends), and the work memory of its AMaZE renderings (mlvfs_amd_render1_amaze_dev) */
void mlvfs_amd_dualiso_trim(void);
/* the global decisions of the calling thread's last conversion: {RGGB?, is_bright[0..3] as bits 3..0, white, white of the bright
 * rows (20 bit), a, b of the exposure fit (hdr.c:638-823), ISO difference in EV, darkened white} */
void mlvfs_amd_dualiso_last_scalars(double out[8]);

/* AMaZE demosaic of a float RGGB plane in HBM (amaze_demosaic_RT.c:113, as called from hdr.c:1034 with
 * winx = winy = 0): d_raw and the three outputs are height rows of width floats (no row padding), values in
 * the caller's scale.  width must be a multiple of 4 (the reference's SSE2 build needs that for a fully
 * written green plane) and the plane at least 36x36.  Bit-identical to the x86-64 reference build.        */
int mlvfs_amd_amaze_demosaic_dev(const float *d_raw, int width, int height, float *d_red, float *d_green, float *d_blue, void *stream);
/* The split of a width x height plane between the two AMaZE kernels: the first nfx x nfy tiles (128-pixel grid, origin -16) are complete
 * -- 160 rows and columns inside the image, not the head of a chain of incomplete tiles -- and are row-streamed through LDS.  No GPU needed. */
void mlvfs_amd_amaze_rows_extent(int width, int height, int *nfx, int *nfy);
/* Test hook: tiles that head a chain of incomplete tiles WITHOUT output (widths that are a multiple of 128) through the row-streamed
 * kernel as well.  mode -1: MLVFS_AMD_AMAZE_ROWS_EXTRA decides (default off: measured 1 % slower per batch), 0 / 1: forced; returns
 * the mode before; *count (may be NULL): the number of such tiles of a width x height plane.  Results are bit-identical either way. */
int mlvfs_amd_amaze_rows_extra_mode(int mode, int width, int height, int *count);
/* Debug: the same with the tile planes copied out (26 planes per 160x160 tile, the layout of k_amaze.hip's block).  mode 0: every
 * tile through k_amaze.hip, blocks in tile order; mode 1: the complete tiles through k_amaze_rows.hip (LDS row streaming), their
 * planes numbered ty * nfx + tx; nfx x nfy = the complete tiles of the plane.  Synchronous. */
int mlvfs_amd_amaze_debug(const float *d_raw, int width, int height, float *d_red, float *d_green, float *d_blue, int mode,
                          float *d_planes, size_t planes_floats, int *nfx, int *nfy);

/* HIP-event timer around the dominant kernel (k_frame) of the calling thread's
 * launches, recorded on the stream the kernel is launched on (bench.py's
 * roofline figure).  begin: arm for up to max_launches launches.  end: waits for
 * the events, writes one duration in milliseconds per launch, returns the count. */
int mlvfs_amd_timer_begin(int max_launches);
int mlvfs_amd_timer_end(float *ms, int cap);

/* FRAME BRACKET.  process_frame (mlvfs/main.c:908-1005) brackets its stages with mlvfs_load_chunks (main.c:923) and
 * mlvfs_close_chunks (main.c:998, resource_manager.c:285-317) on the calling thread and nothing of MLVFS reads image_buffer->data
 * in between (deflicker's hist_add is served, see below).  Between mlvfs_amd_frame_begin() and mlvfs_amd_frame_end() on one thread
 * the drop-in stages of PART 1 therefore do not write the host buffer: unpack, bad-pixel repair (once the clip's map is known),
 * chroma smoothing and stripes are RECORDED and run as one launch of the fused kernel on the packed payload, and the frame is
 * downloaded once, inside mlvfs_amd_frame_end().  integration/mlvfs_amd_wrap.c + `-Wl,--wrap=mlvfs_load_chunks
 * -Wl,--wrap=mlvfs_close_chunks` make those two calls of the UNCHANGED main.c the bracket.
 * Outside a bracket every call completes before it returns -- gif_get_data (gif.c:90-221) uses load_chunks / close_chunks
 * directly and reads the frame right after get_image_data.  Both calls are cheap no-ops for a thread that does no pixel work in
 * between (mlv_get_frame_headers, main.c:434-555, brackets a header walk the same way); MLVFS_AMD_DEFER=0 in the environment
 * disables the deferral.  0 = ok / the host buffer is current. */
int mlvfs_amd_frame_begin(void);
int mlvfs_amd_frame_end(void);
/* inside a bracket: fetch the frame at `image_data` NOW (a host that wants the pixels before the bracket ends).  Does nothing
 * outside a bracket and for a buffer nothing is pending for.  0 = the host buffer is current. */
int mlvfs_amd_frame_sync(void *image_data);
/* out[0]: frames of this process whose recorded stages ran as ONE fused launch at the fetch; out[1]: frames whose recorded stages
 * had to run earlier (a call outside process_frame's order, the first frame of a clip, a focus-pixel map, pattern noise, dual ISO,
 * hist_add on the frame). */
void mlvfs_amd_dropin_stats(long long out[2]);
/* What the drop-in stages moved between host and device since the process started: {frame uploads, frame downloads, bytes up, bytes
 * down} (pixel repairs that fetch their few patched pixels are not counted).  Inside a frame bracket a frame costs one upload of its
 * payload and one download, whatever stages run in between. */
void mlvfs_amd_dropin_transfers(long long out[4]);
/* MLVFS_AMD_DROPIN_PROFILE=1 in the environment: where the wall time of the bracketed frames went, in ms summed over all threads:
 * {inside dng_get_image_data, of it the upload call, of it the wait for the upload's end, inside the recorded stage calls, inside
 * mlvfs_amd_frame_end, of it the fused launch's calls, of it the download call + the wait for it, number of frames}. */
void mlvfs_amd_dropin_profile(double out[8]);
/* Test hook: the calling thread's next fused launch of a bracketed frame (what = 1), next frame download (what = 2) or next growth
 * of one of the library's device or page-locked buffers (what = 3: the old block is freed, nothing is allocated) reports a HIP
 * error without touching the device.  What the caller of a drop-in stage then finds -- a zeroed frame and one line on stderr, never the bytes its
 * malloc returned -- is the library's failure policy ("When the device fails"; tests/test_failure_policy.py). */
void mlvfs_amd_test_fail_next(int what);
/* Test hook, host only: can the dither of stripes_compute_correction be taken from the application's libc generator in bulk
 * (glibc's TYPE_3 state layout, checked once per process on a generator of the library's own; csrc/runtime.cpp)?  1 yes, 0 no (the
 * values are then drawn by calling rand()).  Leaves the application's stream where it was.                              */
int mlvfs_amd_test_rand_layout(void);
/* Test hook, host only: which device the k-th worker thread without a device of its own choosing is bound to on a node whose cards
 * report `bus_ids[0..n)` (HIP ordinal -> PCI bus id): round-robin over the cards IN THE ORDER OF THEIR BUS IDS (csrc/runtime.cpp:
 * thread_ctx; resource_manager.c:111-118 is the pool this replaces).  device_of[0..workers) receives HIP ordinals.            */
int mlvfs_amd_test_device_order(const char *const *bus_ids, int n, int workers, int *device_of);

/* Test hook, host only: how the streaming forms of the fused pass (csrc/k_frame_s.hip, k_frame_p5 in csrc/k_frame_p.hip) cut a frame
 * into tasks -- columns of 62 items (8 pixels each), segments of seg_rows cell rows, `fold` segments of a narrow last column side by
 * side in one wave (a last column of <= 14 items: 4, <= 30 items: 2), tasks per frame.                                              */
int mlvfs_amd_test_stream_plan(int width, int height, int seg_rows, int *cols, int *segs, int *fold, int *tasks_per_frame);
/* Test hook, host only: the fused pass's plan for one launch (csrc/frame_plan.cpp), the switches MLVFS_AMD_KF_P / _KF_P5 / _KF_S read
 * from the environment as a launch reads them.  in[13] = {width, height, bits per pixel, black, chroma smoothing method, packed, input
 * layout (0 any, 1 / 2 rows of whole 16- / 8-pixel groups, 3 12-bit, 4 10-bit), pixel map, stripes (0 none, 1 packed form, 2 other),
 * frames, CUs, held back, some tiles listed}.  out[15] = {first kernel (0 none, 1 k_frame_p, 2 k_frame_p5, 3 k_frame_s), list-mode
 * k_frame follows, k_frame's grid, groups, run, singles, first kernel's grid, rows per task, columns, segments, fold, tasks, k_frame_s
 * steps, work-list entries, status word watched (-1 none)}.  0, or MLVFS_AMD_ERR_ARG for a launch the fused pass refuses.          */
int mlvfs_amd_test_frame_plan(const int *in, long long *out);
/* Test hook, host only: the plan that the calling thread's most recent launch of the fused pass took -- as committed on its stream,
 * the status words' verdicts included --, in the 15 fields of mlvfs_amd_test_frame_plan.  A thread-local copy made on the host; 0, or
 * MLVFS_AMD_ERR_ARG if the thread has launched nothing yet.                                                                      */
int mlvfs_amd_test_last_frame_plan(long long out[15]);
/* Test hook: how many of k_frame's tiles the cs5x5 first kernels (k_frame_p, k_frame_p5) have handed to the list-mode k_frame on
 * `stream` of the current device since the library first launched on it -- every tile with a strip whose packed median was not
 * provably exact, and every task region with more pixel-map records than a wave has lanes; k_frame does those again, so a first
 * kernel that lists everything still gives the right bytes.  Counts the launches that have ended (synchronise first); the difference
 * across a launch against that launch's tiles is what the back-off weighs.  0, or MLVFS_AMD_ERR_ARG before the stream's first cs5x5
 * launch with a first kernel.                                                                                                      */
int mlvfs_amd_test_stream_listed(void *stream, long long *tiles);
/* Test hook, host only: how a batch of `nframes` AMaZE dual-ISO conversions of width x height frames goes out (csrc/dualiso.cpp:
 * dualiso_parts), MLVFS_AMD_DI_PART read from the environment as a conversion reads it.  parts[2k] / parts[2k + 1]: first frame /
 * frames of part k; *tail: 1 if what follows each part's AMaZE runs on a second stream.  Returns the number of parts (at most
 * max_parts), or MLVFS_AMD_ERR_ARG.                                                                                                */
int mlvfs_amd_test_dualiso_parts(int width, int height, int nframes, int *parts, int max_parts, int *tail);

/* -- batched stages of process_frame that existed only per frame ------------- */
/* Pattern noise (patternnoise.c:357-380, debug_flags 0) on `nframes` device frames of one geometry (even width and height), `stride`
 * bytes apart, in place; geom->white = raw_info.white_level.  Every kernel has the frame as a grid dimension: a batch costs the 12
 * launches of one frame per sub-batch (scratch of about 8 bytes per pixel and frame, bounded).  Synchronises the stream.         */
int mlvfs_amd_fix_pattern_noise_dev(const mlvfs_amd_geom_t *geom, void *d_frames, size_t stride, int nframes, void *stream);
/* Test hook: the scratch a batch of mlvfs_amd_fix_pattern_noise_dev (and the mount) may use, in bytes (0: the default again, 256 MB or
 * MLVFS_AMD_PN_SCRATCH_MB); returns the cap before.  A batch that does not fit is cut into even sub-batches.                 */
size_t mlvfs_amd_test_pn_scratch_cap(size_t bytes);
/* Deflicker (main.c:895-906) of `nframes` device frames: one histogram launch, one median launch (a workgroup per frame, the
 * reference's 16-bit counters), one copy of the medians; exposure_bias[2 * f], [2 * f + 1] as mlvfs_amd_deflicker_dev gives them.
 * size_bytes: each frame's size in bytes as main.c:943 passes it.  Synchronises the stream.                                   */
int mlvfs_amd_deflicker_batch_dev(const mlvfs_amd_geom_t *geom, const void *d_frames, size_t stride, int nframes, size_t size_bytes,
                                  int target, int32_t *exposure_bias, void *stream);
/* Dual-ISO preview (hdr_convert_data, hdr.c:40-227, without the focus-pixel repair) of `nframes` device frames, in place: one
 * histogram launch, the fit per frame on the host, one conversion launch.  results[f] = 1 converted, 0 not dual ISO (the frame is
 * left untouched).  max_size as hdr_convert_data takes it (bytes).  Synchronises the stream.                                  */
int mlvfs_amd_hdr_preview_batch_dev(const mlvfs_amd_geom_t *geom, void *d_frames, size_t stride, int nframes, size_t max_size,
                                    int *results, void *stream);

/* -- a clip served as MLVFS serves it (main.c:908-1005) ------------------------ */
/* The mount options of struct mlvfs (mlvfs.h:32-48) that shape a frame's .dng file. */
typedef struct {
    int32_t chroma_smooth;              /* 0, 2, 3, 5 */
    int32_t fix_bad_pixels;             /* 0, 1, 2 (aggressive) */
    int32_t fix_stripes;
    int32_t dual_iso;                   /* 0, 1 preview (hdr_convert_data), 2 full (cr2hdr20_convert_data) */
    int32_t hdr_interpolation_method;   /* 0 AMaZE + edge-directed, 1 mean23 */
    int32_t hdr_no_fullres;
    int32_t hdr_no_alias_map;
    int32_t deflicker;                  /* target level, 0 = off (main.c:895-906, 943) */
    int32_t fix_pattern_noise;
    int32_t rand_mode;                  /* stripe dither: 0 = the application's rand(), like the drop-in symbols; 1 = a private stream
                                           seeded with 1 (what a fresh process draws) */
    double fps;                         /* header fps override, 0 = the clip's */
} mlvfs_amd_mount_opts_t;
/* One clip of an opened reader (mlvfs_amd_mlv_open) served with these options, as a fresh MLVFS process serves it: successive calls
 * serve frames in call order and the order-dependent state follows that order -- the stripe correction comes from the first frame
 * that reaches the stripes stage, the bad-pixel map (shared per clip GUID within the process, like cs.c's) from the first that
 * reaches fix_bad_pixels, the dual-ISO table caches (process-wide, mlvfs_amd_dualiso_reset) from the first that converts.
 * mlv_basename: what process_frame hands dng_get_header_data (the .dng path up to its last separator).  The reader must outlive the
 * handle.  NULL on bad arguments (mlvfs_amd_last_error).                                                                           */
void *mlvfs_amd_mount_open(const void *reader, const mlvfs_amd_mount_opts_t *opts, const char *mlv_basename);
/* Frames first .. first + count - 1 as their .dng files: dng_get_size bytes each (65536 header bytes, then the pixels) at
 * h_out + k * out_stride.  Batches of batch_frames frames (<= 0: 8) go file -> GPU (read, decode or unpack) -> deflicker -> pattern
 * noise -> dual ISO -> focus / bad pixels, chroma smoothing, stripes (the fused pass) -> host, the headers written on the host from
 * each frame's headers after its stages.  io_threads: reader threads (<= 0: 8).  results[k] (optional) = 1 when the frame was
 * converted as dual ISO.  Calls on one handle are serialised.                                                                       */
int mlvfs_amd_mount_dng(void *mount, int first, int count, void *h_out, size_t out_stride, int batch_frames, int io_threads, int *results);
/* The same frames as losslessly compressed .dng files: the pixel data of a file is ONE lossless-JPEG stream (TIFF Compression 7,
 * mlvfs_amd_lj92_encode_batch_dev at 16 bits) of the frame mlvfs_amd_mount_dng would serve, encoded where it lies after the fused
 * pass; only the stream crosses the link.  A w x h frame with even h is encoded as one component of 2w x h/2 (predictor 6 then
 * predicts from the same colour two sensor rows up), an odd h as w x h.  sizes[k]: bytes of file k (65536 + the stream); bytes of
 * h_out behind them are left untouched.  flags[k] bit 0: the frame is served UNCOMPRESSED, byte for byte mlvfs_amd_mount_dng's file
 * (sizes[k] = dng_get_size) -- a frame the encoder refuses, whose stream would be longer than its pixels, or whose highest
 * difference class is 16 (the reference's encoder writes value bits behind class 16 that other decoders do not expect).
 * out_stride >= dng_get_size as before.  The stages, their order and the order-dependent state are mlvfs_amd_mount_dng's: calls of
 * both kinds on one handle interleave in serve order.                                                                            */
int mlvfs_amd_mount_dng_lossless(void *mount, int first, int count, void *h_out, size_t out_stride, size_t *sizes, int *flags,
                                 int batch_frames, int io_threads, int *results);
void mlvfs_amd_mount_close(void *mount);

/* -- dark-frame subtraction (csrc/cal.cpp, csrc/k_cal.hip) ---- */
/* A dark frame: a plane of width x height 16-bit values of `bpp` bits with a pedestal black_d, the black level of the clip it was
 * averaged from.  Subtraction, per pixel in 32-bit signed arithmetic:   out = clamp(px - dark + black_d, 0, 2^bpp - 1).
 * The plane is applied by position in the stored frame (xRes x yRes); panPosX/Y and cropPosX/Y are ignored.  The frame's own levels,
 * its RAWI block and its DNG header do not change.  It is stage 0: after unpack / LZMA / LJ92 decode, before deflicker, pattern
 * noise, dual ISO, pixel repair, chroma smoothing and stripes, which all see subtracted pixels.  The reference has no such stage
 * (`mlv_dump -s` / `-a` do it a frame at a time on a host core).
 * A handle keeps the plane on the host and uploads it once per device, on that device's first use; afterwards it is read-only: it may
 * be shared between threads and mounts and must outlive the mounts that use it.                                                   */
typedef struct mlvfs_amd_dark mlvfs_amd_dark_t;
typedef struct mlvfs_amd_look mlvfs_amd_look_t;   /* "a look for the rendered frames" below */
typedef struct mlvfs_amd_look16 mlvfs_amd_look16_t;   /* "rendered frames at 16 bits" below */
/* geom: width, height, bpp (1..16) and black (= black_d, 0..65535) are used.  Host code: needs no HIP device.  NULL on a null
 * argument, a non-positive size (or 2^27 pixels and more), bpp or black out of range (mlvfs_amd_last_error).                      */
mlvfs_amd_dark_t *mlvfs_amd_dark_create(const mlvfs_amd_geom_t *geom, const uint16_t *h_plane);
/* The rounded mean of frames first .. first + count - 1 of an opened clip (plain, LZMA or LJ92 payloads), 1 <= count <= 65536:
 *     dark[p] = (sum of px_f[p] over the frames + count / 2) / count      (integer division; 32-bit unsigned sums)
 * summed on the GPU in batches of batch_frames frames (<= 0: 8); count = 1 gives the frame itself.  black_d is the black level of
 * frame `first`.  NULL: frames outside the clip, count > 65536, frames of more than one geometry, a read or device failure.      */
mlvfs_amd_dark_t *mlvfs_amd_dark_from_clip(const void *reader, int first, int count, int batch_frames, int io_threads);
/* geom (optional): width, height, bpp, black = black_d, the rest 0; frames_averaged (optional): 0 for a plane given to
 * mlvfs_amd_dark_create.  Host code.                                                                                              */
int  mlvfs_amd_dark_info(const mlvfs_amd_dark_t *dark, mlvfs_amd_geom_t *geom, int *frames_averaged);
/* the plane into h_plane[width * height]; MLVFS_AMD_ERR_ARG when cap_pixels is smaller.  Host code.                              */
int  mlvfs_amd_dark_plane(const mlvfs_amd_dark_t *dark, uint16_t *h_plane, size_t cap_pixels);
void mlvfs_amd_dark_destroy(mlvfs_amd_dark_t *dark);
/* In place on nframes 16-bit device frames `stride` bytes apart (bytes between them are not touched); asynchronous on `stream`.
 * geom's width, height and bpp must be the dark frame's: anything else is MLVFS_AMD_ERR_ARG before any device work.  width * height
 * a multiple of 16 with d_frames and stride 16-byte aligned takes the fast form (16 pixels per lane), anything else down to 2-byte
 * alignment one pixel per lane.                                                                                                   */
int  mlvfs_amd_dark_subtract_dev(const mlvfs_amd_dark_t *dark, const mlvfs_amd_geom_t *geom, void *d_frames, size_t stride,
                                 int nframes, void *stream);
/* The mount subtracts `dark` from every frame it serves, between the read and everything else (mlvfs_amd_mount_dng and
 * mlvfs_amd_mount_dng_lossless alike).  NULL clears.  MLVFS_AMD_ERR_ARG once the handle has served a frame, or when width, height
 * or bpp differ from the clip's.
 * The bad-pixel map is the process's, shared per clip GUID like cs.c's (see mlvfs_amd_mount_open), and is detected from the first
 * frame that reaches the repair -- with a dark frame set, a subtracted one.  Mounts of one clip with different dark frames, or with
 * and without one, in one process share whichever map was detected first: call free_focus_pixel_maps() between them where each is to
 * behave like a fresh process (which is what the byte-for-byte equalities are stated for).                                        */
int  mlvfs_amd_mount_set_dark(void *mount, const mlvfs_amd_dark_t *dark);
/* mlvfs_amd_mlv_transcode with the dark frame subtracted from every frame: the same container rules, refusals, clean-up and stats.
 * With a dark frame, plain output of a plain or LZMA clip goes through the GPU too (upload, unpack and subtract in one pass,
 * mlvfs_amd_pack_dev).  A frame whose width, height or bpp is not the dark frame's: MLVFS_AMD_ERR_ARG before any output file
 * exists.  dark = NULL: mlvfs_amd_mlv_transcode itself, the host-only route included.                                             */
int  mlvfs_amd_mlv_transcode_dark(const void *reader, const char *out_path, int payload, const mlvfs_amd_dark_t *dark,
                                  int batch_frames, int io_threads, long long stats[4]);

/* -- a clip at another bit depth (csrc/mlvwriter.cpp, csrc/k_mlvpack.hip) -- what `mlv_dump -b` does ------------- */
/* For a frame whose RAWI block says bpp bits and a requested out_bpp, d = out_bpp - bpp:
 *     out = px >> -d  (d < 0: truncation; no rounding, no dither)      out = px << d  (d > 0)      out = px  (d = 0)
 * A dark frame, if any, is subtracted first, at the source's depth (stage 0); the shift comes after it.  The reference has no such
 * code: the definition is this project's.
 * mlvfs_amd_rawi_set_bits applies the same rule to a RAWI block in place (host code, no HIP device): raw_info.bits_per_pixel =
 * out_bpp; black_level and white_level shifted like pixels; pitch = raw_info.width * out_bpp / 8; frame_size = xRes * yRes *
 * out_bpp / 8 (integer divisions); every other byte stays.  MLVFS_AMD_ERR_ARG, with the block untouched: a null pointer, out_bpp
 * outside 8..16, a bits_per_pixel outside 1..16.                                                                                 */
int  mlvfs_amd_rawi_set_bits(mlv_rawi_hdr_t *rawi, int out_bpp);
/* Packed payloads of geom->bpp bits (1..16) -> packed payloads of out_bpp bits (8..16) in one pass: unpack, `dark` subtracted
 * (NULL: none; its width, height and bpp must be geom's), shift, pack.  Input as mlvfs_amd_unpack_dev takes it, output as
 * mlvfs_amd_pack_dev writes it: exactly ceil(width * height * out_bpp / 16) words per frame, the unused low bits of the last word
 * zero, nothing behind it touched.  14 / 12 / 10 bits on both sides with width * height a multiple of 16 and 4-byte aligned buffers
 * and strides take the fast form (16 pixels per lane: bpp / 2 dwords in, out_bpp / 2 dwords out), anything else down to 2-byte
 * alignment one output word per lane.  Not in place.  Asynchronous on `stream`; every check happens before any device work.       */
int  mlvfs_amd_repack_dev(const mlvfs_amd_geom_t *geom, int out_bpp, const mlvfs_amd_dark_t *dark, const void *d_packed,
                          size_t packed_stride, void *d_out, size_t out_stride, int nframes, void *stream);
/* mlvfs_amd_mlv_transcode_dark at another bit depth: every frame whose depth is not out_bpp is shifted (after the dark frame) and
 * written at out_bpp -- a plain payload of ceil(w * h * out_bpp / 16) words, an LJ92 payload encoded at out_bpp precision --, and
 * every RAWI block of another depth, in every chunk, is rewritten from its own content as mlvfs_amd_rawi_set_bits does.  The shift
 * rides in a pass the route makes anyway: a plain or LZMA source to plain output is unpacked, subtracted, shifted and packed in one
 * (as in mlvfs_amd_repack_dev), so with a conversion that route goes through the GPU, as it does with a dark frame.  Everything else
 * -- container rules, refusals, clean-up, stats -- is mlvfs_amd_mlv_transcode's.  out_bpp = 0, or the depth every frame has already:
 * mlvfs_amd_mlv_transcode_dark itself, byte for byte and launch for launch, the host-only route included.  out_bpp outside
 * {0, 8..16}: MLVFS_AMD_ERR_ARG before any output file exists.  A frame that cannot be encoded at the new depth fails the call and
 * is named in the error, as before: widening to 16 bits in particular can produce a difference of class 16.                       */
int  mlvfs_amd_mlv_transcode_bits(const void *reader, const char *out_path, int payload, int out_bpp, const mlvfs_amd_dark_t *dark,
                                  int batch_frames, int io_threads, long long stats[4]);

/* -- flat-field correction (csrc/cal.cpp, csrc/k_cal.hip) -- what `mlv_dump -t` does -------------------------- */
/* A flat field: a plane F of width x height 16-bit values with a pedestal black_f, the black level of the clip of an evenly lit
 * target it was averaged from.  Integer arithmetic only.  The gain plane, one uint16 per pixel in Q14 (16384 = 1.0):
 *     s[p]    = max(F[p] - black_f, 1)
 *     c       = (y & 1) * 2 + (x & 1)                                 the channel, by position in the stored frame
 *     M_c     = (sum of s[p] over channel c + n_c / 2) / n_c          n_c pixels of channel c; 64-bit sums
 *     gain[p] = min((M_c * 16384 + s[p] / 2) / s[p], 65535)
 * so a gain stops at 65535 / 16384, just under 4.0: a pixel whose flat value is below a quarter of its channel's mean is corrected
 * by that cap and no more.  A channel without pixels (a width or height of 1) has no M_c and is never read.  The application:
 *     out = clamp(black + floor(((px - black) * gain[p] + 8192) / 16384), 0, 2^bpp - 1)
 * with the frame's own raw_info.black_level and depth; a frame value above 2^bpp - 1, which no valid frame holds but a damaged LJ92
 * stream can decode to, is taken as 2^bpp - 1.  A gain plane has no depth: a flat shot at 14 bits corrects a 12- or 10-bit
 * clip of the same width x height; only the size must match.  A constant flat gives gain = 16384 everywhere and leaves every frame
 * as it is, bit for bit.  The plane is applied by position in the stored frame; panPosX/Y and cropPosX/Y are ignored.  The frame's
 * levels, its RAWI block and its DNG header do not change.  It is stage 0b: directly after the dark frame (stage 0), before every
 * other stage and before a change of bit depth.  The reference has no such stage.
 * A handle keeps the gain plane on the host and uploads it once per device, on that device's first use; afterwards it is read-only: it
 * may be shared between threads and mounts and must outlive the mounts that use it.                                               */
typedef struct mlvfs_amd_flat mlvfs_amd_flat_t;
/* The gain plane of h_plane[width * height], computed on the host.  geom: width, height, bpp (1..16) and black (= black_f,
 * 0..65535) are used.  Needs no HIP device.  NULL on a null argument, a non-positive size (or 2^27 pixels and more), bpp or black
 * out of range (mlvfs_amd_last_error).                                                                                            */
mlvfs_amd_flat_t *mlvfs_amd_flat_create(const mlvfs_amd_geom_t *geom, const uint16_t *h_plane);
/* The gain plane of the rounded mean of frames first .. first + count - 1 of an opened clip (mlvfs_amd_dark_from_clip's mean and
 * limits), computed on the GPU; black_f is the black level of frame `first`.  dark (optional; its width, height and bpp must be the
 * flat clip's) is subtracted from the mean plane first.  The plane equals mlvfs_amd_flat_create's of the same mean.  NULL as for
 * mlvfs_amd_dark_from_clip, and for a dark frame of another geometry.                                                             */
mlvfs_amd_flat_t *mlvfs_amd_flat_from_clip(const void *reader, int first, int count, const mlvfs_amd_dark_t *dark, int batch_frames,
                                           int io_threads);
/* geom (optional): width, height, the flat plane's bpp and black = black_f, the rest 0; frames_averaged (optional): 0 for a plane
 * given to mlvfs_amd_flat_create; means (optional): M_c[4], 0 for a channel without pixels.  Host code.                           */
int  mlvfs_amd_flat_info(const mlvfs_amd_flat_t *flat, mlvfs_amd_geom_t *geom, int *frames_averaged, uint32_t means[4]);
/* the gain plane into h_gain[width * height]; MLVFS_AMD_ERR_ARG when cap_pixels is smaller.  Host code.                           */
int  mlvfs_amd_flat_gain(const mlvfs_amd_flat_t *flat, uint16_t *h_gain, size_t cap_pixels);
void mlvfs_amd_flat_destroy(mlvfs_amd_flat_t *flat);
/* In place on nframes 16-bit device frames `stride` bytes apart (bytes between them are not touched); asynchronous on `stream`.
 * geom: the FRAMES' width, height, bpp (1..16) and black (0..65535).  dark (optional; geom's width, height and bpp) is subtracted
 * first, in the same pass.  A size that is not the flat field's, a dark frame of another geometry, bpp or black out of range:
 * MLVFS_AMD_ERR_ARG before any device work.  Up to 15 bits with black <= 32767, width * height a multiple of 16 and d_frames and
 * stride 16-byte aligned take the fast form (16 pixels per lane, 32-bit products); anything else, 16-bit frames included, one pixel
 * per lane with 64-bit products, down to 2-byte alignment.                                                                        */
int  mlvfs_amd_flat_apply_dev(const mlvfs_amd_flat_t *flat, const mlvfs_amd_dark_t *dark, const mlvfs_amd_geom_t *geom, void *d_frames,
                              size_t stride, int nframes, void *stream);
/* The mount corrects every frame it serves with `flat`, directly after the dark frame if one is set and before everything else
 * (mlvfs_amd_mount_dng and mlvfs_amd_mount_dng_lossless alike).  NULL clears.  MLVFS_AMD_ERR_ARG once the handle has served a
 * frame, or when width or height differ from the clip's.
 * As for mlvfs_amd_mount_set_dark: the bad-pixel map is the process's, shared per clip GUID, and is detected from the first frame
 * that reaches the repair -- with a flat field set, a corrected one.  Mounts of one clip with different flat fields, or with and
 * without one, in one process share whichever map was detected first: call free_focus_pixel_maps() between them where each is to
 * behave like a fresh process (which is what the byte-for-byte equalities are stated for).                                        */
int  mlvfs_amd_mount_set_flat(void *mount, const mlvfs_amd_flat_t *flat);
/* mlvfs_amd_mlv_transcode_bits with the flat field applied to every frame after the dark frame and before the change of depth.
 * flat = NULL: mlvfs_amd_mlv_transcode_bits itself, byte for byte and launch for launch.  With a flat field the load delivers
 * corrected 16-bit frames, and the tiling or packing pass (with the shift, if any) follows: every route goes through the GPU, plain
 * output of a plain clip included, and plain or LZMA to plain pays one pass more than the packed-to-packed repack.  A frame whose
 * width or height is not the flat field's: MLVFS_AMD_ERR_ARG before any output file exists.                                       */
int  mlvfs_amd_mlv_transcode_cal(const void *reader, const char *out_path, int payload, int out_bpp, const mlvfs_amd_dark_t *dark,
                                 const mlvfs_amd_flat_t *flat, int batch_frames, int io_threads, long long stats[4]);

/* -- half-size Bayer proxies (csrc/k_proxy.hip, csrc/mount.cpp) -------------------------------------------------- */
/* A proxy: the frame the mount serves, binned 2x2 within each colour of the CFA, so that a quarter of the pixels remain and the file is
 * still raw.  Integer arithmetic only; the reference has no such stage.  A W x H frame with W >= 4 and H >= 4 becomes W' x H':
 *     W' = 2 * floor(W / 4)        H' = 2 * floor(H / 4)
 * columns 4 * floor(W / 4) .. W - 1 and rows 4 * floor(H / 4) .. H - 1 are never read.  H' is even, so the lossless path always
 * takes its 2W' x H'/2 form.  Output pixel (Y, X) has the CFA parity py = Y & 1, px = X & 1 and is the rounded mean of the four
 * pixels of that parity inside its 4x4 block:
 *     y0 = 4 * (Y >> 1) + py        x0 = 4 * (X >> 1) + px
 *     out(Y, X) = (in(y0, x0) + in(y0, x0 + 2) + in(y0 + 2, x0) + in(y0 + 2, x0 + 2) + 2) >> 2
 * exact for every 16-bit input (the sum takes 18 bits).  CFA pattern, black level, white level and bit depth stay the frame's.
 * It is the LAST stage: after chroma smoothing and stripes, on the frame mlvfs_amd_mount_dng would have served; dark frame, flat
 * field, bad-pixel map, stripe coefficients, dual ISO and deflicker all work at full size, in serve order, as without a proxy.
 * A dual-ISO clip served unconverted (dual_iso = 0) has its two ISOs mixed: rows y0 and y0 + 2 differ in ISO.  Nothing is done
 * about that.
 * The proxy file's first 65536 bytes are the header mlvfs_amd_mount_dng writes for the frame in its final state (levels x4 after a
 * conversion, exposure_bias after deflicker) but for the value fields of these tags -- all of fixed size, so every other byte keeps
 * its offset.  With lo(v) = 2 * ceil(v / 4), hi(v, lim) = min(2 * floor(v / 4), lim) and (x1, y1, x2, y2) = raw_info.active_area as
 * the full-size header uses it (after its own overwrite rule):
 *     256 ImageWidth, 257 ImageLength, 278 RowsPerStrip      W', H', H'
 *     279 StripByteCounts                                    W' * H' * 2, or the stream's length under Compression 7
 *     50719 DefaultCropOrigin                                (lo(ox), lo(oy))
 *     50720 DefaultCropSize                                  (max(hi(x2, W') - lo(x1), 0), max(hi(y2, H') - lo(y1), 0))
 *     50829 ActiveArea (top, left, bottom, right)            lo(top), lo(left), hi(bottom, H'), hi(right, W')
 *     41486 / 41487 FocalPlaneX/YResolution                  the same numerators, denominators x 2
 * DefaultScale, the 5:3 and "x3 below 2000 columns" decisions, the levels and every other tag are the FULL-SIZE frame's.           */
/* W', H' of a width x height frame.  Host code.  MLVFS_AMD_ERR_ARG: a null pointer, factor != 2, a size below 4, 2^27 pixels or more. */
int    mlvfs_amd_proxy_geom(int width, int height, int factor, int *pw, int *ph);
/* nframes frames of width x height 16-bit pixels `stride` bytes apart -> their proxies, W' x H' pixels each (rows W' * 2 bytes apart),
 * out_stride bytes apart.  Bytes between frames and behind W' * H' * 2 are not touched.  Not in place.  Asynchronous on `stream`;
 * every check happens before any device work: a null pointer, a size below 4 or of 2^27 pixels and more, a negative frame count,
 * odd addresses or strides, strides smaller than a frame (with more than one frame), source and destination ranges that overlap are
 * MLVFS_AMD_ERR_ARG.  width a multiple of 16 with both bases and both strides 16-byte aligned takes the fast form (k_bin2_x16: a lane
 * reads 16 pixels of each of a block row's four rows and writes 8 pixels to each of two rows), anything else one output pixel per lane. */
int    mlvfs_amd_bin2_dev(const void *d_frames, size_t stride, int width, int height, void *d_out, size_t out_stride, int nframes,
                          void *stream);
/* The proxy file's header as defined above; stream_bytes = 0: uncompressed (dng_get_header_data's tags 259 and 279 rule), else
 * mlvfs_amd_dng_header_lossless's.  Rewrites raw_info.active_area like dng_get_header_data.  Host code.  Returns 0 and writes
 * nothing for a null pointer, factor != 2 or a frame below 4x4 (mlvfs_amd_last_error).                                           */
size_t mlvfs_amd_dng_header_proxy(struct frame_headers *frame_headers, uint8_t *output_buffer, off_t offset, size_t max_size,
                                  double fps_override, const char *mlv_basename, int factor, uint32_t stream_bytes);
/* factor 2: the handle serves proxies -- mlvfs_amd_mount_dng files of 65536 + W' * H' * 2 bytes, mlvfs_amd_mount_dng_lossless the
 * binned frames as 2W' x H'/2 streams with the sizes, the cap and the fallback of the proxy file; results[], the serve-order state
 * and every stage in front of the binning are untouched.  out_stride of both calls may then be anything from the proxy file's size
 * up.  factor 1: off (the default), byte for byte and launch for launch.  MLVFS_AMD_ERR_ARG: a null handle, another factor, a handle
 * that has served a frame, a clip whose first frame is smaller than 4x4.                                                          */
int    mlvfs_amd_mount_set_proxy(void *mount, int factor);
/* bytes of file `index` as this handle serves it uncompressed (dng_get_size, or the proxy file's size); 0: no such frame */
size_t mlvfs_amd_mount_dng_size(const void *mount, int index);

/* -- rendered half-size sRGB frames (csrc/k_render.hip, csrc/dngheader.cpp, csrc/mount.cpp) --------------------------- */
/* A rendering: the frame the mount serves, developed to 8-bit sRGB at half size, as a TIFF any viewer opens.  The definition is this
 * project's (the reference has no such stage), in integers only, so that it has a byte-exact oracle (mlvfs_amd/render.py).
 * Geometry.  A W x H frame with W, H >= 2 becomes W' x H' RGB pixels, W' = floor(W / 2), H' = floor(H / 2).  An odd last column or
 * row is never read.  The CFA is RGGB, as the header always declares it.  The whole frame is rendered: no crop to the active area.
 * Input.  The frame mlvfs_amd_mount_dng would have served, after every stage, at full size, with the BlackLevel and WhiteLevel of the
 * header written for that frame in its final state (the x4 levels after a dual-ISO conversion).  range = max(white - black, 1).
 * Per output pixel (Y, X):
 *   1. superpixel   c0 = in(2Y, 2X)    c1 = (in(2Y, 2X + 1) + in(2Y + 1, 2X) + 1) >> 1    c2 = in(2Y + 1, 2X + 1)
 *                   c'_j = max(c_j - black, 0)
 *   2. balance, exposure, normalisation to 16 bits
 *                   n_j = min((c'_j * A_j + 2048) >> 12, 65535)            the product in 64 bits; the min keeps clipped highlights
 *                                                                          neutral instead of pink
 *   3. camera to linear sRGB
 *                   acc_i = sum_j K[i][j] * n_j                            64 bits, signed
 *                   t_i = clamp((acc_i + 32768) >> 16, 0, 4095)            the shift is arithmetic: floor
 *   4. tone         out_i = LUT[t_i]                                       bytes in R, G, B order, rows top down, no padding in a row
 * Per-frame parameters, computed on the host in exact integer arithmetic (no floating point takes part):
 *   A_j   from the frame's AsShotNeutral num_j / den_j -- the six integers the header writes in tag 50728 -- and the caller's gain_q8,
 *         1 .. 65535, 256 is unity:    D = 256 * num_j * range    A_j = floor((2 * 65535 * 4096 * gain_q8 * den_j + D) / (2 * D))
 *         capped at 2^31 - 1.  If any num_j <= 0 or any den_j <= 0, all three channels take num = den = 1.
 *   K     from the camera's ForwardMatrix2 FM, nine integers over 10000 (tag 50965; always this matrix, no interpolation between
 *         illuminants), and the D50-XYZ -> linear-sRGB matrix as integers over 10^7
 *             S = [[31338561, -16168667, -4906146], [-9787684, 19161415, 334540], [719453, -2289914, 14052427]]
 *         P[i][j] = sum_k S[i][k] * FM[k][j]      K[i][j] = floor((2 * 4096 * P[i][j] + 10^11) / (2 * 10^11)), floor towards -inf
 *   LUT   the 8-bit sRGB curve on 12 bits, LUT[t] = round(255 * oetf(t / 4095)), oetf(x) = 12.92 x for x <= 0.0031308, else
 *         1.055 x^(1 / 2.4) - 0.055: 4096 constant bytes (csrc/srgb_lut12.h = tests/golden/srgb_lut12.bin), never computed at run time.
 * The deflicker's exposure_bias is NOT applied: gain_q8 is the only exposure control.
 * The file: a baseline little-endian TIFF with one strip -- ImageWidth W', ImageLength H', BitsPerSample 8 8 8, Compression 1,
 * PhotometricInterpretation 2, StripOffsets = the header's size, Orientation 1, SamplesPerPixel 3, RowsPerStrip H', StripByteCounts
 * 3 W' H', PlanarConfiguration 1, Software "MLVFS" -- of mlvfs_amd_rgb_header_size() + 3 W' H' bytes.                              */
/* W', H' of a width x height frame.  Host code.  MLVFS_AMD_ERR_ARG: a null pointer, a size below 2, 2^27 pixels or more. */
int    mlvfs_amd_rgb_geom(int width, int height, int *pw, int *ph);
/* bytes of the file's header: fixed (256), a multiple of 16 */
size_t mlvfs_amd_rgb_header_size(void);
/* the tone table.  Host code. */
int    mlvfs_amd_rgb_lut(uint8_t out[4096]);
/* out = black, A[3], K[9] (K row by row) for a frame with these headers: the levels are raw_info's as passed in, the neutral is what
 * dng_get_header_data writes for them, the matrix the camera's (cameraName; unknown cameras use the first row, as the header does).
 * Host code.  MLVFS_AMD_ERR_ARG (out untouched): a null pointer, gain_q8 outside 1 .. 65535.                                        */
int    mlvfs_amd_rgb_params(const struct frame_headers *frame_headers, int gain_q8, int32_t out[13]);
/* the header of a pw x ph file into out[0 .. cap): returns its size, or 0 and writes nothing for a null pointer, pw or ph below 1,
 * 2^25 pixels or more, cap below the header's size (mlvfs_amd_last_error).  Host code.                                             */
size_t mlvfs_amd_rgb_header(int pw, int ph, uint8_t *out, size_t cap);
/* nframes frames of width x height 16-bit pixels `stride` bytes apart -> their renderings, 3 W' H' bytes each, out_stride bytes apart,
 * frame k with the 13 parameters d_params[13 k ..] (device memory, as mlvfs_amd_rgb_params yields them).  Bytes between frames and
 * behind 3 W' H' are not touched.  Not in place.  Asynchronous on `stream`; every check happens before any device work: a null
 * pointer, a size below 2 or of 2^27 pixels and more, a negative frame count, an odd source address or stride, parameters off a
 * 4-byte boundary, strides smaller than a frame (with more than one frame), a destination that overlaps the source or the parameters
 * are MLVFS_AMD_ERR_ARG.  width a multiple of 16 with source base and stride 16-byte and destination base and stride 8-byte aligned
 * takes the fast form (k_render2_x16: a lane reads 16 pixels of each of a superpixel row's two rows and writes 8 pixels, 24 bytes);
 * anything else one output pixel per lane (k_render2_generic).                                                                     */
int    mlvfs_amd_render2_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                             size_t out_stride, int nframes, void *stream);
/* mlvfs_amd_mount_dng's frames first .. first + count - 1, through the same stages, the same serve-order state and the same
 * results[], as rendered TIFF files out_stride bytes apart in h_out: header + pixels, out_stride anything from the file's size up.
 * Each frame's parameters come from its headers in their final state.  Only the 3 W' H' bytes of a frame cross the link.  May be
 * interleaved with mlvfs_amd_mount_dng and mlvfs_amd_mount_dng_lossless on one handle.  MLVFS_AMD_ERR_ARG besides mlvfs_amd_mount_dng's:
 * gain_q8 outside 1 .. 65535, a handle with mlvfs_amd_mount_set_proxy(2), frames below 2x2.                                         */
int    mlvfs_amd_mount_rgb(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int batch_frames,
                           int io_threads, int *results);
/* bytes of file `index` as mlvfs_amd_mount_rgb serves it; 0: no such frame, or one below 2x2 */
size_t mlvfs_amd_mount_rgb_size(const void *mount, int index);

/* -- rendered frames as baseline JPEG files (csrc/k_jpeg.hip, csrc/jpeg.cpp, csrc/mount.cpp) -------------------------- */
/* A rendering as an ordinary baseline (DCT, Huffman) JFIF file that any decoder opens, a tenth of the TIFF's bytes.  The definition is
 * this project's (the reference has no such stage), in integers only, so that it has a byte-exact oracle (mlvfs_amd/jpeg.py).
 * Input.   W' x H' RGB bytes exactly as mlvfs_amd_render2_dev writes them: rows top down, no padding in a row.  W', H' 1 .. 65535,
 *          W' H' < 2^25.
 * Colour.  JFIF full-range YCbCr per pixel, 32 bits signed, arithmetic (floor) shifts:
 *            Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *            Cb = clamp(((-11058 R - 21710 G + 32768 B + 32768) >> 16) + 128, 0, 255)      (R = G = 0, B = 255 gives 256 before the clamp)
 *            Cr = clamp(((32768 R - 27439 G - 5329 B + 32768) >> 16) + 128, 0, 255)
 * MCUs.    4:2:0 (the default; 4:2:2 and 4:4:4: "the chroma sampling of the JPEG files" below), MCUs of 16 x 16 pixels, mw = ceil(W' / 16),
 *          mh = ceil(H' / 16).  The three planes are extended to 16 mw x 16 mh by repeating the last column and the last row; then Cb
 *          and Cr are halved:
 *            c(y, x) = (p(2y, 2x) + p(2y, 2x + 1) + p(2y + 1, 2x) + p(2y + 1, 2x + 1) + 2) >> 2
 * DCT.     Of each 8 x 8 block of p - 128, with the integer matrix T[u][x] = round(8192 s(u) cos((2x + 1) u pi / 16)), s(0) = sqrt(1 / 8),
 *          s(u > 0) = 1 / 2 -- 64 constants (row 1: 4017 3406 2276 799 -799 -2276 -3406 -4017), never computed by the library:
 *            rows     A[y][u] = (sum_x T[u][x] (p[y][x] - 128) + 128) >> 8          |A| < 2^14
 *            columns  B[v][u] = sum_y T[v][y] A[y][u]                               |B| < 2^29: the coefficient times 2^18
 * Tables.  The IJG rule for quality 1 .. 100: scale = 5000 / quality below 50, else 200 - 2 quality;
 *          Q[k] = clamp((base[k] scale + 50) / 100, 1, 255), integer divisions, base the two example tables of Annex K of the standard.
 * Quantisation.  q = sgn(B) floor((|B| + Q 2^17) / (Q 2^18)) (round half away from zero) = sgn(B) floor(((|B| + (Q << 17)) >> 18) / Q);
 *          the 63 AC values are then clamped to +-1023 (DC lies in -1024 .. 1016).
 * Entropy coding.  Baseline sequential, the zigzag order of the standard, the four "typical" Huffman tables of Annex K.3 - K.6, never
 *          others.  One interleaved scan, blocks of an MCU in the order Y(0,0) Y(0,1) Y(1,0) Y(1,1) Cb Cr.  DC: the difference to the
 *          block of the same component before; category = bit length of |d|; value bits d for d >= 0, else d + 2^cat - 1.  AC: (run,
 *          category) symbols, ZRL (0xF0) for each 16 zeros in front of a non-zero value, EOB (0x00) if and only if the last non-zero
 *          coefficient lies before position 63.
 * Restart intervals.  One MCU row each (DRI = mw): every row starts with the three DC predictors at 0, ends padded with 1-bits to a
 *          byte, and every row but the last is followed by FF D0 + (r mod 8), r from 0.  Every 0xFF byte of entropy-coded data, one
 *          that the padding completes included, is followed by 0x00.
 * The file.  SOI; APP0 FF E0 00 10 'JFIF\0' 01 01 00 00 01 00 01 00 00; two DQT segments (ids 0 and 1, zigzag order); SOF0 (precision 8,
 *          H', W', components 01 22 00, 02 11 01, 03 11 01); four DHT segments (DC0 AC0 DC1 AC1); DRI; SOS (01 00, 02 11, 03 11, 00 3F 00)
 *          -- mlvfs_amd_jpeg_header_size() = 629 bytes --; the rows with their RST markers; EOI.                                      */
size_t mlvfs_amd_jpeg_header_size(void);
/* the file's bytes in front of the entropy-coded data into out[0 .. cap): returns their number, or 0 and writes nothing for a null
 * pointer, a size outside the input's, a quality outside 1 .. 100, cap below 629 (mlvfs_amd_last_error).  Host code.                */
size_t mlvfs_amd_jpeg_header(int pw, int ph, int quality, uint8_t *out, size_t cap);
/* the two quantisation tables of a quality, natural (row-major) order, luminance then chrominance.  Host code.  MLVFS_AMD_ERR_ARG (out
 * untouched): a null pointer, a quality outside 1 .. 100.                                                                            */
int    mlvfs_amd_jpeg_qtables(int quality, uint8_t out[128]);
/* bytes of device scratch mlvfs_amd_jpeg_encode_dev takes for nframes renderings of pw x ph; 0: a size outside the input's.  Host code. */
size_t mlvfs_amd_jpeg_scratch_bytes(int pw, int ph, int nframes);
/* nframes renderings of pw x ph RGB bytes `stride` apart -> per frame the entropy-coded data followed by EOI at d_out + k out_stride.
 * h_lengths[k]: that length, known on return (the call synchronises `stream`).  h_status[k] = 1 where it exceeds `room`: then no byte
 * at or behind `room` is touched and the frame's content is unspecified; otherwise 0, and bytes behind the stream and between frames
 * are not touched.  The streams may begin at any address.  Every check happens before any device work: a null pointer, a size outside
 * the input's, a quality outside 1 .. 100, a frame count outside 0 .. 65535, strides smaller than a rendering or than `room` (with more
 * than one frame), a scratch off a 16-byte boundary or smaller than mlvfs_amd_jpeg_scratch_bytes, renderings, streams and scratch that
 * overlap are MLVFS_AMD_ERR_ARG.                                                                                                     */
int    mlvfs_amd_jpeg_encode_dev(const void *d_rgb, size_t stride, int pw, int ph, int quality, void *d_out, size_t out_stride, size_t room,
                                 void *d_scratch, size_t scratch_bytes, uint32_t *h_lengths, int *h_status, int nframes, void *stream);
/* mlvfs_amd_mount_rgb's frames, through the same stages, the same serve-order state, the same results[] and the same rendering, as
 * JPEG files of `quality`: each rendering is encoded on the device where it lies, the header is written on the host and only the
 * stream crosses the link.  sizes[k]: the bytes of file k.  flags[k] bit 0: the JPEG file would be larger than the TIFF
 * (629 + stream > 256 + 3 W' H'), and the frame is served as mlvfs_amd_mount_rgb's TIFF, byte for byte.  out_stride: anything from
 * mlvfs_amd_mount_rgb_size up.  May be interleaved with the other three serving calls on one handle; a handle that never calls it
 * serves what it served before, launch for launch.  MLVFS_AMD_ERR_ARG besides mlvfs_amd_mount_rgb's: null sizes or flags, a quality
 * outside 1 .. 100.                                                                                                                  */
int    mlvfs_amd_mount_jpeg(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int quality, size_t *sizes,
                            int *flags, int batch_frames, int io_threads, int *results);

/* -- the chroma sampling of the JPEG files (csrc/k_jpeg.hip, csrc/jpeg.cpp, csrc/mount.cpp) ------------------------------ */
/* Everything above describes MLVFS_AMD_JPEG_420, the default.  A sampling s changes four things of the definition and nothing else
 * (colour, DCT, tables, quantisation, Huffman tables, stuffing, EOI are as above; the oracle takes it as `sampling`: mlvfs_amd/jpeg.py):
 * MCUs.    (mcw, mch) = (16, 16) at 4:2:0, (16, 8) at 4:2:2, (8, 8) at 4:4:4; mw = ceil(W' / mcw), mh = ceil(H' / mch); the three planes
 *          are extended to mcw mw x mch mh by repeating the last column and the last row.
 * Chroma.  4:2:0 as above;  4:2:2: c(y, x) = (p(y, 2x) + p(y, 2x + 1) + 1) >> 1;  4:4:4: c = p.
 * Blocks.  Of an MCU: its luminance blocks from left to right (4:2:0: the top row first; 4:2:2: Y0 Y1; 4:4:4: Y), then Cb, Cr.  DC
 *          prediction is per component and starts at 0 in every MCU row: the first Y block of an MCU from the last Y block of the MCU
 *          before, later Y blocks from the block before them, Cb and Cr from the MCU before.
 * Restart intervals.  One MCU row of the sampling each: DRI = mw, RST index = MCU row mod 8.
 * The file.  629 bytes of header at every sampling; three bytes differ: byte 169, the sampling factors of component 1 (22, 21, 11), and
 *          bytes 613 - 614, the DRI count.                                                                                              */
#define MLVFS_AMD_JPEG_420 0     /* H2V2: six blocks per MCU */
#define MLVFS_AMD_JPEG_422 1     /* H2V1: four */
#define MLVFS_AMD_JPEG_444 2     /* H1V1: three */
/* mlvfs_amd_jpeg_header at a sampling: besides its refusals, a sampling that is none of the three returns 0 and writes nothing.  Host code. */
size_t mlvfs_amd_jpeg_header_sampled(int pw, int ph, int quality, int sampling, uint8_t *out, size_t cap);
/* mlvfs_amd_jpeg_scratch_bytes at a sampling (what mlvfs_amd_jpeg_encode_sampled_dev takes); 0 also for a sampling that is none of the
 * three.  4:4:4 has twice the MCU rows and twice the coefficient bytes per pixel of 4:2:0.  Host code.                               */
size_t mlvfs_amd_jpeg_scratch_bytes_sampled(int pw, int ph, int sampling, int nframes);
/* the MCU grid of pw x ph at a sampling into *mw, *mh.  Host code.  MLVFS_AMD_ERR_ARG (nothing written): a null pointer, a sampling that
 * is none of the three, a size outside the input's.                                                                                   */
int    mlvfs_amd_jpeg_mcus(int pw, int ph, int sampling, int *mw, int *mh);
/* mlvfs_amd_jpeg_encode_dev at a sampling: the same contract -- checks before any device work, `room`, h_lengths, h_status, untouched
 * bytes -- and one refusal more, MLVFS_AMD_ERR_ARG for a sampling that is none of the three.  mlvfs_amd_jpeg_encode_dev is this call
 * with MLVFS_AMD_JPEG_420.                                                                                                            */
int    mlvfs_amd_jpeg_encode_sampled_dev(const void *d_rgb, size_t stride, int pw, int ph, int quality, int sampling, void *d_out,
                                         size_t out_stride, size_t room, void *d_scratch, size_t scratch_bytes, uint32_t *h_lengths,
                                         int *h_status, int nframes, void *stream);
/* The sampling of every later mlvfs_amd_mount_jpeg, _full, _scaled and _resampled call of the handle, their AMaZE forms included.  It
 * holds no serve-order state and may change between calls; the rendering, the flag rule (the TIFF where 629 + stream > 256 + 3 W' H'),
 * sizes[] and results[] are unchanged.  A handle that never calls it serves 4:2:0, launch for launch what it served before.
 * MLVFS_AMD_ERR_ARG: a null handle, a sampling that is none of the three.
 * Not built: 4:1:1 and 4:4:0, greyscale files, per-frame Huffman tables, progressive coding, a sampling chosen from the quality
 * (DESIGN.md 3.21).                                                                                                                   */
int    mlvfs_amd_mount_set_jpeg_sampling(void *mount, int sampling);

/* -- rendered full-size sRGB frames (csrc/k_demosaic.hip, csrc/mount.cpp) --------------------------------------------- */
/* The rendering at the size the frame was shot: three channels per sensor pixel.  The definition is this project's, in integers only,
 * so that it has a byte-exact oracle (mlvfs_amd/demosaic.py): a fixed linear demosaic, the Malvar-He-Cutler 5x5 filter, whose
 * coefficients are eighths and sixteenths, between the half-size rendering's balance and its matrix.
 * Geometry.  A W x H frame with W, H >= 4 and W H < 2^25 becomes W x H RGB pixels; odd sizes are allowed.  The CFA is RGGB.  No crop.
 * Input.  The frame mlvfs_amd_mount_dng would have served, and the 13 parameters black, A[3], K[9] exactly as mlvfs_amd_rgb_params
 * yields them for the half-size rendering.
 *   1. balance every sensor pixel at its own site: the site's colour is j(y, x) = (y & 1) + (x & 1) (0 R, 1 G, 2 B) and
 *                   b(y, x) = min((max(in(y, x) - black, 0) * A_j + 2048) >> 12, 65535)        the product in 64 bits
 *      (steps 1's clamp and 2 of the half-size definition per pixel).  Balancing before interpolating keeps clipped highlights
 *      neutral -- every channel stops at 65535 first -- and gives the filter's cross-channel terms channels of equal scale.
 *      Border.  b outside the frame is b reflected about the edge pixel: index i < 0 stands for -i, i >= n for 2 (n - 1) - i
 *      (-1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3).  The reflection keeps the CFA parity and needs n >= 3.
 *   2. interpolate, in sixteenths.  With c = b(y, x),
 *                   h1 = b(y, x - 1) + b(y, x + 1)      v1 = b(y - 1, x) + b(y + 1, x)      d1 = the four diagonal neighbours
 *                   h2 = b(y, x - 2) + b(y, x + 2)      v2 = b(y - 2, x) + b(y + 2, x)
 *                   sG = 8 c + 4 (h1 + v1) - 2 (h2 + v2)                green at an R or B site
 *                   sH = 10 c + 8 h1 - 2 d1 - 2 h2 + v2                 the colour whose samples lie left and right of a green site
 *                   sV = 10 c + 8 v1 - 2 d1 - 2 v2 + h2                 the colour whose samples lie above and below a green site
 *                   sD = 12 c + 4 d1 - 3 (h2 + v2)                      B at an R site, R at a B site
 *                   site                          R     G     B
 *                   R (even row, even column)     c     sG    sD
 *                   G (even row, odd column)      sH    c     sV
 *                   G (odd row, even column)      sV    c     sH
 *                   B (odd row, odd column)       sD    sG    c
 *      An interpolated channel is m = clamp((s + 8) >> 4, 0, 65535), the shift arithmetic (floor); the site's own channel is m = c.
 *      |s| < 2^22: 32 bits signed hold every sum.
 *   3., 4.  the half-size definition's, with n = (m_R, m_G, m_B): t_i = clamp((sum_j K[i][j] n_j + 32768) >> 16, 0, 4095) in 64 bits,
 *      out_i = LUT[t_i]; bytes in R, G, B order, rows top down, no padding in a row.
 * The file: mlvfs_amd_rgb_header(W, H, ...) followed by 3 W H bytes -- the same 256-byte TIFF header at full size.
 * Not built: an adaptive demosaic, a crop to the active area, 16-bit output, highlight recovery, other CFA orders, enlarging (smaller
 * sizes: "rendered frames at any smaller size" and "rendered frames resampled from the full-size rendering" below).               */
/* *pw = width, *ph = height.  Host code.  MLVFS_AMD_ERR_ARG: a null pointer, a size below 4, 2^25 pixels or more. */
int    mlvfs_amd_rgb_full_geom(int width, int height, int *pw, int *ph);
/* mlvfs_amd_render2_dev at full size: nframes frames of width x height 16-bit pixels `stride` bytes apart -> their renderings, 3 W H
 * bytes each, out_stride bytes apart, frame k with the 13 parameters d_params[13 k ..].  Bytes between frames and behind 3 W H are not
 * touched.  Not in place.  Asynchronous on `stream`; every check happens before any device work, and the checks are
 * mlvfs_amd_render2_dev's but for the size: below 4x4 or of 2^25 pixels and more is MLVFS_AMD_ERR_ARG.  width a multiple of 16 with
 * source base and stride 16-byte and destination base and stride 8-byte aligned takes the fast form (k_render1_x16: a workgroup walks
 * down a strip of 512 columns with the balanced rows in a ring in LDS, a lane writes 8 pixels, 24 bytes); anything else one output
 * pixel per lane with its taps from global memory (k_render1_generic).                                                          */
int    mlvfs_amd_render1_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                             size_t out_stride, int nframes, void *stream);
/* mlvfs_amd_mount_rgb and mlvfs_amd_mount_jpeg at full size: the same arguments, the same stages, the same serve-order state and the
 * same results[]; each file is the full-size TIFF (256 + 3 W H bytes) or the JPEG file of that rendering.  flags[k] bit 0: the JPEG
 * file would be larger than the TIFF (629 + stream > 256 + 3 W H), and the frame is served as mlvfs_amd_mount_rgb_full's TIFF.
 * out_stride: anything from mlvfs_amd_mount_rgb_full_size up.  The renderings (and a JPEG call's streams behind them) lie in a device
 * buffer of their own, which the first full-size call allocates for its batch; a handle that never makes a full-size call serves what
 * it served before, byte for byte and launch for launch.  May be interleaved with the other serving calls on one handle.
 * MLVFS_AMD_ERR_ARG besides the half-size calls': frames below 4x4 or of 2^25 pixels and more.                                      */
int    mlvfs_amd_mount_rgb_full(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int batch_frames,
                                int io_threads, int *results);
int    mlvfs_amd_mount_jpeg_full(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int quality, size_t *sizes,
                                 int *flags, int batch_frames, int io_threads, int *results);
/* bytes of file `index` as mlvfs_amd_mount_rgb_full serves it; 0: no such frame, or one below 4x4 or of 2^25 pixels and more */
size_t mlvfs_amd_mount_rgb_full_size(const void *mount, int index);

/* -- rendered frames at any smaller size (csrc/k_scale.hip, csrc/mount.cpp) -------------------------------------------- */
/* The rendering at any size up to half the frame's -- a daily, a thumbnail --, area-averaged in linear light between the half-size
 * rendering's balance and its matrix.  The definition is this project's (the reference has no such stage), in integers only, so that
 * it has a byte-exact oracle (mlvfs_amd/scale.py).
 * Geometry.  W' = floor(W / 2), H' = floor(H / 2) as in the half-size rendering.  The caller names an output size ow x oh with
 *   1 <= ow <= W', 1 <= oh <= H': the scaling never enlarges.  W' <= 65535, H' <= 65535 and W H < 2^27.  Anything else is
 *   MLVFS_AMD_ERR_ARG.
 * Source.  The three balanced superpixel channels n_j(Y, X), j = 0 .. 2, on the W' x H' grid: exactly steps 1 and 2 of the half-size
 *   definition, 16 bits each.
 * Weights.  In units of 1 / ow of a source pixel, source column X covers [X ow, (X + 1) ow) and output column u covers
 *   [u W', (u + 1) W'):
 *                   wx(u, X) = max(0, min((X + 1) ow, (u + 1) W') - max(X ow, u W'))
 *   The weights of one output column sum to W'; the weights of one source column over all outputs sum to ow.  wy(v, Y) is defined
 *   likewise with H' and oh.  The products stay below 2^32.
 * Horizontal pass.
 *                   hm_j(Y, u) = floor((sum_X wx(u, X) n_j(Y, X) + (W' >> 1)) / W')
 *   The sum is at most 65535^2, so it fits in 32 bits unsigned with the rounding term.
 * Vertical pass.
 *                   m_j(v, u) = floor((sum_Y wy(v, Y) hm_j(Y, u) + (H' >> 1)) / H')              the bound is the same
 * Steps 3 and 4 are the half-size definition's with n = m: matrix K, clamp to 12 bits, LUT; bytes in R, G, B order, rows top down,
 *   no padding in a row.
 * Consequences the tests use: ow = W', oh = H' gives the half-size rendering byte for byte; a constant frame renders to the same
 *   constant at every size; two source values a and a + 1 averaged 1 : 1 give a + 1, because a half rounds up.
 * The file: mlvfs_amd_rgb_header(ow, oh, ...) followed by 3 ow oh bytes, or the JPEG file of that rendering; the flag rule is the
 *   half-size JPEG call's: bit 0 is set and the TIFF is served when 629 + stream > 256 + 3 ow oh.
 * Not applied, as before: the deflicker's exposure bias, and any crop.
 * Not built: enlarging, other filters than the area average, contact sheets.  Sizes between half and full size: "rendered frames
 *   resampled from the full-size rendering" below.                                                                                   */
/* the largest size inside a box of box_w x box_h at the frame's aspect.  Host code.  With W', H' as above: box_w >= W' and
 * box_h >= H' gives (W', H'); otherwise, if box_w H' <= box_h W' (in 64 bits), the width limits: ow = min(box_w, W'),
 * oh = max(1, (2 ow H' + W') / (2 W')); otherwise the height limits: oh = min(box_h, H'), ow = max(1, (2 oh W' + H') / (2 H')).
 * MLVFS_AMD_ERR_ARG, with the outputs untouched: a null pointer, a box side below 1, a frame that the scaled rendering does not take. */
int    mlvfs_amd_rgb_fit(int width, int height, int box_w, int box_h, int *ow, int *oh);
/* mlvfs_amd_render2_dev at ow x oh: nframes frames of width x height 16-bit pixels `stride` bytes apart -> their renderings, 3 ow oh
 * bytes each, out_stride bytes apart, frame k with the 13 parameters d_params[13 k ..].  Bytes between renderings and behind 3 ow oh
 * are not touched.  Not in place.  Asynchronous on `stream`; every check happens before any device work, and the checks are
 * mlvfs_amd_render2_dev's plus the geometry above.  width a multiple of 16 with source base and stride 16-byte aligned takes the fast
 * form (k_scale_x16: a workgroup walks the source rows of a band of output rows of one strip of columns, the balanced row in LDS;
 * one pass, nothing in between in device memory); anything else one output pixel per lane with its footprint from global memory
 * (k_scale_generic).                                                                                                               */
int    mlvfs_amd_render_scaled_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                   void *d_out, size_t out_stride, int nframes, void *stream);
/* mlvfs_amd_mount_rgb and mlvfs_amd_mount_jpeg at ow x oh: the same stages, the same serve-order state and the same results[]; each
 * file is the TIFF of 256 + 3 ow oh bytes or the JPEG file of that rendering.  Only 3 ow oh bytes, or the stream, cross the link.
 * out_stride: anything from mlvfs_amd_mount_rgb_scaled_size up.  The renderings are developed into the frames' other slots, as the
 * half-size ones are; a handle that never makes a scaled call serves what it served before, byte for byte and launch for launch.
 * May be interleaved with the other serving calls on one handle.  MLVFS_AMD_ERR_ARG besides the half-size calls' (a handle with
 * mlvfs_amd_mount_set_proxy(2) among them): a size outside the geometry above.                                                      */
int    mlvfs_amd_mount_rgb_scaled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int ow, int oh,
                                  int batch_frames, int io_threads, int *results);
int    mlvfs_amd_mount_jpeg_scaled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int quality, int ow,
                                   int oh, size_t *sizes, int *flags, int batch_frames, int io_threads, int *results);
/* bytes of file `index` as mlvfs_amd_mount_rgb_scaled serves it; 0: no such frame, or a size the frame does not allow */
size_t mlvfs_amd_mount_rgb_scaled_size(const void *mount, int index, int ow, int oh);
/* Test hooks, host only.  mlvfs_amd_test_scale_div: out[k] = floor(in[k] / d) by the multiplication k_scale_x16 divides with, d >= 1.
 * mlvfs_amd_test_scale_plan: how a launch of nframes frames is divided among k_scale_x16's workgroups -- out = { width % 16 == 0, the
 * superpixels a step stages, the most output columns of a strip, the output columns of a strip, the strips, the output rows of a
 * band, the bands, the source rows a band covers at least }.                                                                       */
int    mlvfs_amd_test_scale_div(uint32_t d, int n, const uint32_t *in, uint32_t *out);
int    mlvfs_amd_test_scale_plan(int width, int height, int ow, int oh, int nframes, int32_t out[8]);

/* -- a look for the rendered frames (csrc/k_tone_dev.h, csrc/look.cpp, csrc/mount.cpp) --------------------------------- */
/* Step 4 of the three renderings is one fixed sRGB curve.  A look replaces that step, and only that step, by a per-channel shaper table
 * followed by a 3D table with tetrahedral interpolation -- "with our LUT on it": a .cube file from the grade, a log curve for the editor.
 * The definition is this project's, in integers only, so that it has a byte-exact oracle (mlvfs_amd/look.py).
 * A look is (S, N, T):
 *   S   4096 unsigned 16-bit values, any values (it need not be monotone)
 *   N   2 .. 65
 *   T   N^3 entries of three unsigned 16-bit values (R, G, B out), indexed T[(b N + g) N + r]: red fastest, the order of a .cube file
 * Steps 1 - 3 of the half-size, the full-size and the scaled definition are unchanged: three 12-bit linear-sRGB indices t_r, t_g, t_b per
 * output pixel.  With a look, step 4 is
 *   4a. u_c = S[t_c]                                               c = r, g, b
 *   4b. p_c = u_c (N - 1)     i_c = p_c >> 16     f_c = p_c & 65535
 *       u_c <= 65535, so i_c <= N - 2 always: the cell i .. i + 1 exists on every axis.
 *   4c. tetrahedral interpolation.  Let a, b, c be the three axes ordered so that f_a >= f_b >= f_c.
 *         V0 = T[i]     V1 = T[i + e_a]     V2 = T[i + e_a + e_b]     V3 = T[i + (1, 1, 1)]
 *         w0 = 65536 - f_a     w1 = f_a - f_b     w2 = f_b - f_c     w3 = f_c                        they sum to 65536
 *         v_k = (sum_j w_j V_j[k] + 32768) >> 16                                                     per output channel k
 *       The sum with its rounding term is below 2^32 (65536 * 65535 + 32768): 32 bits unsigned suffice, and v_k <= 65535.  The order
 *       among equal fractions does not matter -- the vertex two orders disagree on has weight 0 --, so there is no tie rule.
 *   4d. out_k = floor((v_k + 128) / 257), 0 .. 255: v_k / 257 rounded, a half up.
 * Bytes, rows and files are as before.
 * Consequences the tests use: with S[t] = 257 LUT[t] and the identity table T[g] = floor((2 * 65535 g + (N - 1)) / (2 (N - 1))) per axis
 *   the output is the plain rendering's, byte for byte, at every N (v differs from u by at most 1); a table of 65535 throughout behind
 *   S = 65535 throughout gives v = 65535.
 * Limits.  The table is fed from the 12-bit linear t, so a log shaper has coarse steps in the deepest shadows; for 8-bit output that is
 *   accepted, and "rendered frames at 16 bits" below feeds a deep look from a 16-bit t.  No floating point takes part: S and T arrive
 *   as integers (mlvfs_amd/look.py converts a .cube file's decimals in exact rational arithmetic).
 * Not built: vendor log curves by name, 1D-only .cube files and domains other than 0 .. 1, more than one
 *   look per launch, a table kept in LDS, a look on the .dng or proxy routes.                                                          */
/* bytes of the device image of a look with a table of n a side: 8192 + 8 n^3; 0 for n outside 2 .. 65.  Host code. */
size_t mlvfs_amd_look_image_size(int n);
/* the device image into image[0 .. cap): S as it is, then the N^3 entries in the table's order as four uint16 each, R, G, B, 0 (with the
 * image 16-byte aligned every entry is one aligned 64-bit load).  Host code.  MLVFS_AMD_ERR_ARG, with the image untouched: a null
 * pointer, n outside 2 .. 65, cap below mlvfs_amd_look_image_size(n).                                                                  */
int    mlvfs_amd_look_pack(const uint16_t shaper[4096], int n, const uint16_t *table, void *image, size_t cap);
/* a look on the calling thread's device: packed, uploaded once, independent of any mount.  NULL (mlvfs_amd_last_error): a null pointer,
 * n outside 2 .. 65, no device, no memory (nothing is held then).  Calls that run on another device refuse the handle.                 */
mlvfs_amd_look_t *mlvfs_amd_look_create(const uint16_t shaper[4096], int n, const uint16_t *table);
void   mlvfs_amd_look_destroy(mlvfs_amd_look_t *look);
/* mlvfs_amd_render2_dev, mlvfs_amd_render1_dev and mlvfs_amd_render_scaled_dev with the look as step 4: the same arguments, the same
 * checks before any device work (a null look is MLVFS_AMD_ERR_ARG too), the same rule for the fast form; the kernels are
 * k_render2_look_x16 / _generic, k_render1_look_x16 / _generic and k_scale_look_x16 / _generic.  One look per launch.                  */
int    mlvfs_amd_render2_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                                  size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream);
int    mlvfs_amd_render1_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                                  size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream);
int    mlvfs_amd_render_scaled_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                        void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream);
/* step 4 alone: n triples t_r, t_g, t_b of 16-bit values at d_t (each is masked to 12 bits) -> n triples of bytes at d_out, device
 * memory both.  Asynchronous on `stream`.  MLVFS_AMD_ERR_ARG: a null pointer, indices at an odd address, more than 2^40 triples, a
 * destination that overlaps the indices.                                                                                               */
int    mlvfs_amd_look_apply_dev(const mlvfs_amd_look_t *look, const uint16_t *d_t, size_t n, uint8_t *d_out, void *stream);
/* every later mlvfs_amd_mount_rgb* and mlvfs_amd_mount_jpeg* call of the handle, at all three sizes, renders with the look (the
 * mlvfs_amd_mount_rgb16* calls below do not: they take a deep look of their own per call); NULL clears.  Allowed at any time between
 * serving calls: it touches no serve-order state, so unlike mlvfs_amd_mount_set_dark it is not refused after the first frame.  The
 * .dng, lossless and proxy routes never see it; the JPEG routes encode the rendering where it lies, so flags, sizes and results[] keep
 * their rules.  The look must outlive its use.  A handle that never sets a look serves byte for byte and launch for launch what it
 * served before.  MLVFS_AMD_ERR_ARG: a null handle.                                                                                    */
int    mlvfs_amd_mount_set_look(void *mount, const mlvfs_amd_look_t *look);

/* -- rendered frames at 16 bits (csrc/k_tone_dev.h, csrc/look.cpp, csrc/mount.cpp) ------------------------------------- */
/* The routes above end in 8 bits and quantise linear light to a 12-bit index before the tone step: enough for a daily, not for a grade.
 * The 16-bit routes serve the same three renderings as 16-bit TIFF files, toned from a 16-bit linear index.  Integers only; the numpy
 * restatement is mlvfs_amd/look.py (stages16, apply16) with render.py, demosaic.py and scale.py (look16=).
 * A deep look is (S16, N, T):
 *   S16 65536 unsigned 16-bit values, any values (it need not be monotone)
 *   N   0, or 2 .. 65; 0: there is no table
 *   T   N^3 entries of three unsigned 16-bit values, T[(b N + g) N + r], exactly as in the 8-bit look; absent when N = 0
 * Steps 1 and 2 of the half-size definition, the demosaic of the full-size definition and the two averaging passes of the scaled
 * definition are unchanged: three 16-bit channels n_j (m_j) per output pixel and the 13 parameters of mlvfs_amd_rgb_params.  Then
 *   3d. acc_i = sum_j K[i][j] n_j as before     t_i = clamp((acc_i + 2048) >> 12, 0, 65535)           (signed; an arithmetic shift)
 *       K is Q12 and n has 16 bits: the same sum read four bits further down.  Where the matrix fits 32 bits for the 8-bit routes
 *       (sum_j |K[i][j]| * 65535 + 32768 < 2^31) it does here, the rounding term being the smaller one.
 *   4a. u_c = S16[t_c]
 *   N = 0:  out_c = u_c
 *   N >= 2: 4b and 4c of the 8-bit look, word for word: the cell, the fractions, the tetrahedron, v_k = (sum_j w_j V_j[k] + 32768) >> 16;
 *           out_k = v_k.  There is no step 4d.
 *   Samples: unsigned 16 bits, little-endian, R, G, B; a pixel is 6 bytes; rows top down, no padding.
 * The file: the 256 bytes of mlvfs_amd_rgb_header with BitsPerSample 16 16 16 and StripByteCounts 6 pw ph -- the same tags, order and
 * offsets otherwise --, then 6 pw ph bytes.
 * Consequences the tests use: S16[t] = t and N = 0 give a file of t itself, a linear 16-bit TIFF; a constant S16 with N = 0 gives a
 *   constant file; the scaled route at W' x H' gives the half-size route's bytes; t >> 4 is not always the 8-bit routes' t (the
 *   roundings differ).
 * The library ships no default curve (a 16-bit sRGB curve would be 128 KiB of constant, and the library computes nothing in floating
 *   point): every 16-bit call takes a deep look; mlvfs_amd/look.py gives shaper16_linear, shaper16_srgb and shaper16_log2.
 * Not built: 16-bit JPEG files, more than one deep look per launch, S16 or the table kept in LDS.                                       */
/* bytes of the device image of a deep look: 131072 + 8 n^3; 0 for n outside {0, 2 .. 65}.  Host code. */
size_t mlvfs_amd_look16_image_size(int n);
/* the device image into image[0 .. cap): S16 as it is, then the N^3 entries as four uint16 each, R, G, B, 0 (16-byte aligned, every entry
 * is one aligned 64-bit load; every gather is in bounds whatever S16 and a frame hold, t and u being at most 65535).  Host code.
 * MLVFS_AMD_ERR_ARG, with the image untouched: a null shaper or image, a null table with n != 0, n outside {0, 2 .. 65}, a short cap. */
int    mlvfs_amd_look16_pack(const uint16_t shaper[65536], int n, const uint16_t *table, void *image, size_t cap);
/* a deep look on the calling thread's device, with the lifetime rules of mlvfs_amd_look_create.  table may be NULL only when n = 0.     */
mlvfs_amd_look16_t *mlvfs_amd_look16_create(const uint16_t shaper[65536], int n, const uint16_t *table);
void   mlvfs_amd_look16_destroy(mlvfs_amd_look16_t *look);
/* the 256-byte header of a 16-bit file; everything else as mlvfs_amd_rgb_header.  Host code. */
size_t mlvfs_amd_rgb16_header(int pw, int ph, uint8_t *out, size_t cap);
/* mlvfs_amd_render2_look_dev, mlvfs_amd_render1_look_dev and mlvfs_amd_render_scaled_look_dev at 16 bits: the same arguments with a deep
 * look, 6 bytes per pixel written, all checks before any device work, the stride checks with 6 bytes per pixel.  The fast forms
 * (k_render2_deep_x16, k_render1_deep_x16) write a lane's 8 pixels as three 16-byte stores and need the destination base and stride
 * 16-byte aligned -- a destination that is only 8-byte aligned takes the generic kernel --; k_scale_deep_x16 needs them 2-byte aligned;
 * the rules for the source are the 8-bit calls'.  One deep look per launch.                                                            */
int    mlvfs_amd_render2_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                                  size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream);
int    mlvfs_amd_render1_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                                  size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream);
int    mlvfs_amd_render_scaled_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                        void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream);
/* step 4 alone: n triples of raw 16-bit t at d_t -> n triples of 16-bit samples at d_out, device memory both, 2-byte aligned.
 * Asynchronous on `stream`.  MLVFS_AMD_ERR_ARG: a null pointer, an odd address, more than 2^40 triples, an overlap.                   */
int    mlvfs_amd_look16_apply_dev(const mlvfs_amd_look16_t *look, const uint16_t *d_t, size_t n, uint16_t *d_out, void *stream);
/* mlvfs_amd_mount_rgb, mlvfs_amd_mount_rgb_full and mlvfs_amd_mount_rgb_scaled as 16-bit TIFF files: the same arguments plus a non-null
 * deep look, passed per call.  The same stages, the same serve-order state, the same results[]; they may be interleaved with every other
 * serving call.  They refuse a handle with mlvfs_amd_mount_set_proxy(2) and ignore mlvfs_amd_mount_set_look, which belongs to the 8-bit
 * routes.  A handle that never makes such a call serves byte for byte and launch for launch what it served before.                     */
int    mlvfs_amd_mount_rgb16(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, const mlvfs_amd_look16_t *look,
                             int batch_frames, int io_threads, int *results);
int    mlvfs_amd_mount_rgb16_full(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8,
                                  const mlvfs_amd_look16_t *look, int batch_frames, int io_threads, int *results);
int    mlvfs_amd_mount_rgb16_scaled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int ow, int oh,
                                    const mlvfs_amd_look16_t *look, int batch_frames, int io_threads, int *results);
/* bytes of file `index` as those calls serve it: 256 + 6 pw ph; 0 where the 8-bit size call gives 0 */
size_t mlvfs_amd_mount_rgb16_size(const void *mount, int index);
size_t mlvfs_amd_mount_rgb16_full_size(const void *mount, int index);
size_t mlvfs_amd_mount_rgb16_scaled_size(const void *mount, int index, int ow, int oh);

/* -- rendered frames resampled from the full-size rendering (csrc/k_resample.hip, csrc/mount.cpp) ---------------------- */
/* The rendering at any size up to the frame's own -- a 1920 x 1080 delivery of a 3.5K clip, a 1 x 3 binning mode squeezed back --,
 * area-averaged in linear light between the full-size rendering's demosaic and its matrix.  The definition is this project's, in
 * integers only, so that it has a byte-exact oracle (mlvfs_amd/resample.py).
 * Geometry.  W, H >= 4, W <= 65535, H <= 65535 and W H < 2^25: the full-size rendering's rule and a limit on the sides.  The caller
 *   names an output size ow x oh with 1 <= ow <= W, 1 <= oh <= H: the resampling never enlarges, and the two factors are independent
 *   (ow = W, oh = H / 3 is allowed).  Anything else is MLVFS_AMD_ERR_ARG before any device work.
 * Source.  The three demosaiced 16-bit channels d_c(y, x), c = R, G, B, of the full-size definition after its steps 1 and 2: the pixel
 *   balanced at its own site, the border reflected about the edge pixel, the Malvar-He-Cutler sums in sixteenths, an interpolated
 *   channel clamp((s + 8) >> 4, 0, 65535), the site's own channel untouched.
 * Weights.  The scaled definition's with W and H in the place of W' and H':
 *                   wx(u, x) = max(0, min((x + 1) ow, (u + 1) W) - max(x ow, u W))              wy(v, y) likewise with H and oh
 * Horizontal pass.
 *                   hd_c(y, u) = floor((sum_x wx(u, x) d_c(y, x) + (W >> 1)) / W)
 * Vertical pass.
 *                   m_c(v, u) = floor((sum_y wy(v, y) hd_c(y, u) + (H >> 1)) / H)
 *   Every sum is at most 65535^2 and fits 32 bits unsigned with its rounding term.
 * Steps 3 and 4 are the half-size definition's with n = m, in each of the three tone forms: the sRGB table, a look, a deep look with
 *   16-bit samples.
 * Consequences the tests use: ow = W, oh = H is the full-size rendering byte for byte, in all three tone forms; a frame that is flat per
 *   CFA colour renders to the half-size definition's pixel at every size.
 * This is NOT the scaled route at the sizes both accept (1x1 up to W' x H'): this one averages interpolated samples, that one
 *   averages superpixels, and their bytes differ.  Neither chooses the other by itself.
 * The file: mlvfs_amd_rgb_header(ow, oh, ...) followed by 3 ow oh bytes; at 16 bits mlvfs_amd_rgb16_header and 6 ow oh bytes; or the
 *   JPEG file of the 8-bit rendering with the half-size JPEG call's flag rule.
 * Not applied, as before: the deflicker's exposure bias, and any crop.
 * Not built: enlarging, other filters than the area average, an adaptive demosaic as the source.                                      */
/* mlvfs_amd_rgb_fit's rule on the W x H grid: if box_w H <= box_h W (in 64 bits) the width limits: ow = min(box_w, W),
 * oh = max(1, (2 ow H + W) / (2 W)); otherwise the height limits: oh = min(box_h, H), ow = max(1, (2 oh W + H) / (2 H)).  3584 x 1320
 * in 1920 x 1080 gives 1920 x 707.  Host code.  MLVFS_AMD_ERR_ARG, with the outputs untouched: a null pointer, a box side below 1, a
 * frame that the resampled rendering does not take.                                                                                  */
int    mlvfs_amd_rgb_fit_full(int width, int height, int box_w, int box_h, int *ow, int *oh);
/* mlvfs_amd_render1_dev at ow x oh: nframes frames of width x height 16-bit pixels `stride` bytes apart -> their renderings, 3 ow oh
 * bytes each (6 ow oh in the deep form), out_stride bytes apart, frame k with the 13 parameters d_params[13 k ..].  Bytes between
 * renderings and behind a rendering are not touched.  Not in place.  Asynchronous on `stream`; every check happens before any device
 * work, and the checks are mlvfs_amd_render1_dev's plus the geometry above; the look and deep forms take what their render1
 * counterparts take.  width a multiple of 16 with source base and stride 16-byte aligned and 2 ow >= width takes the fast form
 * (k_resample_x16: a workgroup walks the source rows of a band of output rows of one strip of columns, the balanced rows in
 * k_render1_x16's ring, the demosaiced row in LDS; one pass, nothing in between in device memory; the deep form needs a 2-byte aligned
 * destination); anything else one output pixel per lane with its footprint demosaiced from global memory (k_resample_generic).     */
int    mlvfs_amd_render_resampled_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                      void *d_out, size_t out_stride, int nframes, void *stream);
int    mlvfs_amd_render_resampled_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                           void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream);
int    mlvfs_amd_render_resampled_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                           void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream);
/* mlvfs_amd_mount_rgb_full, mlvfs_amd_mount_jpeg_full and mlvfs_amd_mount_rgb16_full at ow x oh: the same stages, the same serve-order
 * state, the same results[], the handle's look on the 8-bit calls.  A resampled rendering can exceed a frame's other slot, so the
 * renderings (and a JPEG call's streams behind them) lie in the full-size calls' device buffer, sized for ow x oh; it grows and fails
 * as it does for them.  out_stride: anything from the size call's answer up.  A handle that never makes a resampled call serves byte
 * for byte and launch for launch what it served before.  May be interleaved with the other serving calls on one handle.
 * MLVFS_AMD_ERR_ARG besides the full-size calls' (a handle with mlvfs_amd_mount_set_proxy(2) among them): a size outside the geometry. */
int    mlvfs_amd_mount_rgb_resampled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int ow, int oh,
                                     int batch_frames, int io_threads, int *results);
int    mlvfs_amd_mount_jpeg_resampled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int quality, int ow,
                                      int oh, size_t *sizes, int *flags, int batch_frames, int io_threads, int *results);
int    mlvfs_amd_mount_rgb16_resampled(void *mount, int first, int count, void *h_out, size_t out_stride, int gain_q8, int ow, int oh,
                                       const mlvfs_amd_look16_t *look, int batch_frames, int io_threads, int *results);
/* bytes of file `index` as those calls serve it (256 + 3 ow oh, 256 + 6 ow oh); 0: no such frame, or a size the frame does not allow */
size_t mlvfs_amd_mount_rgb_resampled_size(const void *mount, int index, int ow, int oh);
size_t mlvfs_amd_mount_rgb16_resampled_size(const void *mount, int index, int ow, int oh);
/* Test hook, host only: how a launch of nframes frames is divided among k_resample_x16's workgroups -- out = { 1 where the sizes allow
 * the fast form (width % 16 == 0 and 2 ow >= width; the alignment is the caller's), the most source columns of a strip, the output
 * columns of a strip, the strips, the output rows of a band, the bands, the source rows a band covers at least, the source rows of
 * a step }; the four numbers of the plan are 0 where the first is.  A strip's source columns run from floor(us0 W / ow) rounded down
 * to 8 up to ceil(us1 W / ow) rounded up to 8; a band's source rows from floor(v0 H / oh) up to ceil(v1 H / oh).                  */
int    mlvfs_amd_test_resample_plan(int width, int height, int ow, int oh, int nframes, int32_t out[8]);

/* -- rendered full-size frames demosaiced by AMaZE (csrc/k_amaze_render.hip, csrc/amaze_render.cpp) -------------------- */
/* The full-size rendering with the library's AMaZE (csrc/k_amaze.hip, csrc/k_amaze_rows.hip: amaze_demosaic_RT.c bit for bit) in the
 * place of the Malvar-He-Cutler filter.  The definition is this project's, integers but for AMaZE itself (mlvfs_amd/amaze_render.py):
 * Geometry.  W a multiple of 4, W >= 36, H >= 36 (what mlvfs_amd_amaze_demosaic_dev takes) and W H < 2^25.  Anything else is
 *   MLVFS_AMD_ERR_ARG before any device work; no such frame is ever served by the linear filter instead.
 * 1. b(y, x) = min((max(in(y, x) - black, 0) A_j + 2048) >> 12, 65535), j = (y & 1) + (x & 1): the full-size definition's step 1.
 *    raw(y, x) = b(y, x) as binary32, which is exact.
 * 2. (R, G, B) = AMaZE(raw): amaze_demosaic_RT.c:113 as hdr.c calls it, winx = winy = 0, the 65535 scale, output planes zero beforehand.
 * 3. n_c = (int)floor(clampf(v_c) + 0.5f) in binary32, c = R, G, B; clampf(v) = 0 for NaN and v <= 0, 65535 for v >= 65535, v otherwise.
 * 4. The half-size definition's steps 3 and 4 on n, in each of the three tone forms: the sRGB table, a look, a deep look with 16-bit
 *    samples; both forms of the matrix give the same result.
 * The file: the full-size routes', byte for byte in its header.  Not applied, as before: the deflicker's exposure bias, and any crop.
 * Not built: AMaZE behind the half-size or scaled routes, other CFA orders, highlight recovery.  AMaZE behind the resampled route is
 * the next section's.                                                                                                              */
/* *pw = width, *ph = height for a frame the route takes.  Host code.  MLVFS_AMD_ERR_ARG, with the outputs untouched: a null pointer,
 * a frame outside the geometry above.                                                                                              */
int    mlvfs_amd_rgb_amaze_geom(int width, int height, int *pw, int *ph);
/* Step 1: nframes frames of width x height 16-bit pixels `stride` bytes apart -> their float planes, plane_stride floats apart, frame k
 * with the 13 parameters d_params[13 k ..] (of which black and A are read).  Floats between planes are not touched.  Asynchronous on
 * `stream`; every check happens before any device work: null pointers, the geometry, an odd source address or stride, parameters or
 * planes off a 4-byte boundary, strides smaller than a frame or a plane, planes that overlap the source or the parameters.  width a
 * multiple of 16 with source base and stride and plane base and stride 16-byte aligned takes the fast form (k_amz_balance_x16: 8
 * pixels per lane, one 16-byte load, two 16-byte stores), anything else one pixel per lane (k_amz_balance_generic).                    */
int    mlvfs_amd_amaze_balance_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, float *d_planes,
                                   size_t plane_stride, int nframes, void *stream);
/* Steps 3 and 4: three batches of nframes float planes, plane_stride floats apart -> interleaved RGB, 3 W H bytes per frame, out_stride
 * bytes apart; with look16 set 6 W H bytes of 16-bit samples.  look and look16 may each be null (both null: the sRGB table), never both
 * set.  Bytes between renderings and behind a rendering are not touched.  Asynchronous on `stream`; every check happens before any
 * device work: null planes, parameters or destination, the geometry, planes or parameters off a 4-byte boundary, strides too small, a
 * destination that overlaps a plane or the parameters.  width a multiple of 16 with plane bases and stride 16-byte aligned and the
 * destination base and stride 8-byte aligned (16-byte with look16) takes the fast form (k_amz_tone_x16 and its look and deep forms:
 * 8 pixels per lane, 24 bytes as three 8-byte stores or 48 as three 16-byte stores), anything else one pixel per lane.               */
int    mlvfs_amd_amaze_tone_dev(const float *d_red, const float *d_green, const float *d_blue, size_t plane_stride, int width, int height,
                                const int32_t *d_params, void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look_t *look,
                                const mlvfs_amd_look16_t *look16, void *stream);
/* mlvfs_amd_render1_dev, mlvfs_amd_render1_look_dev and mlvfs_amd_render1_deep_dev with AMaZE as the demosaic: the same arguments and
 * the same checks with this route's geometry.  Each runs step 1, the library's AMaZE for the batch, then steps 3 and 4.  Work memory:
 * four float planes and AMaZE's tile planes per frame, 0.71 GB per frame at 3584 x 1320, held per host thread and device, grown on
 * demand, given back by mlvfs_amd_dualiso_trim.  A batch that would need more than 6 GiB, or more than can be allocated, runs in
 * sub-batches; a call fails with MLVFS_AMD_ERR_HIP only where one frame's work memory cannot be had.  The tile planes are this
 * route's own and are zeroed when they are allocated anew or serve another geometry: a dual-ISO conversion and an AMaZE rendering on
 * one thread never see each other's.  Calls of one thread on different streams are the caller's to order: they share that memory.   */
int    mlvfs_amd_render1_amaze_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                                   size_t out_stride, int nframes, void *stream);
int    mlvfs_amd_render1_amaze_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                                        size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream);
int    mlvfs_amd_render1_amaze_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, void *d_out,
                                        size_t out_stride, int nframes, const mlvfs_amd_look16_t *look, void *stream);
/* Which demosaic mlvfs_amd_mount_rgb_full, mlvfs_amd_mount_jpeg_full and mlvfs_amd_mount_rgb16_full use: 0 the linear filter (the
 * default), 1 AMaZE.  No serve-order state: it may change between serving calls, as the look may.  The same stages, results[], flags and
 * look handling; the renderings lie where the linear ones lie and the JPEG encoder takes them there.  With 1 set:
 * mlvfs_amd_mount_rgb_full_size is 0 for a frame outside the geometry above and the three calls refuse it; the _resampled calls are
 * refused with MLVFS_AMD_ERR_ARG unless mlvfs_amd_mount_set_resample_demosaic(mount, 1) has given them AMaZE of their own (the next
 * section); every other call serves what it served.  A handle that never calls this serves byte for byte and
 * launch for launch what it served before.  MLVFS_AMD_ERR_ARG: a null handle, another value.                                          */
int    mlvfs_amd_mount_set_demosaic(void *mount, int which);
/* Test hook, host only: how a batch of nframes frames is cut to fit cap_bytes of work memory (0: the library's 6 GiB) -- out = { floats
 * from one plane to the next, floats of a frame's tile planes, bytes of work memory per frame, frames of a sub-batch (at least 1, at
 * most nframes) }.  MLVFS_AMD_ERR_ARG: null, nframes below 1, a frame outside the geometry.                                          */
int    mlvfs_amd_test_amaze_render_plan(int width, int height, int nframes, size_t cap_bytes, int64_t out[4]);

/* -- resampled rendered frames demosaiced by AMaZE (csrc/k_amaze_resample.hip, csrc/amaze_render.cpp) ----------------- */
/* The resampled rendering with AMaZE as its source: the two definitions above composed, with no arithmetic of its own
 * (mlvfs_amd/amaze_resample.py):
 * Geometry.  W a multiple of 4, W >= 36, H >= 36, W H < 2^25 (the AMaZE rendering's) and W, H <= 65535; 1 <= ow <= W, 1 <= oh <= H, the
 *   two factors independent, never larger than the frame.  Anything else is MLVFS_AMD_ERR_ARG before any device work; no such frame is
 *   ever served by the linear filter instead.
 * 1. - 3. The AMaZE rendering's: every site balanced, raw = float32(b), (R, G, B) = AMaZE(raw), n_c = (int)floor(clampf(v_c) + 0.5f).
 * 4. The resampled rendering's average on n in the place of d, horizontally first, each pass rounded on its own:
 *    hd_c(y, u) = floor((sum_x wx(u, x) n_c(y, x) + (W >> 1)) / W), m_c(v, u) = floor((sum_y wy(v, y) hd_c(y, u) + (H >> 1)) / H).
 * 5. The half-size definition's steps 3 and 4 on m, in each of the three tone forms.
 * The file: mlvfs_amd_rgb_header(ow, oh) or its 16-bit form.  ow = W, oh = H is the AMaZE full-size rendering byte for byte.
 * Not built: AMaZE behind the half-size and scaled routes (they average superpixels and have no demosaic), enlarging.              */
/* MLVFS_AMD_OK for a frame and a size the route takes, MLVFS_AMD_ERR_ARG otherwise.  Host code.  mlvfs_amd_rgb_fit_full gives the
 * fitted size.                                                                                                                     */
int    mlvfs_amd_rgb_amaze_resample_geom(int width, int height, int ow, int oh);
/* Steps 3 to 5 alone, on a caller's planes: mlvfs_amd_amaze_tone_dev's arguments and checks plus the size, 3 ow oh bytes per frame (6
 * with look16).  Every check happens before any device work and follows no pointer.  width a multiple of 8 with 2 ow >= width, plane
 * bases and stride 16-byte aligned and, with look16, a 2-byte aligned destination base and stride takes the fast form
 * (k_amz_resample_x16 and its look and deep forms: strips and bands as mlvfs_amd_test_amz_resample_plan reports them), anything else
 * one output pixel per lane (k_amz_resample_generic and its forms).                                                                 */
int    mlvfs_amd_amaze_resample_dev(const float *d_red, const float *d_green, const float *d_blue, size_t plane_stride, int width, int height,
                                    const int32_t *d_params, int ow, int oh, void *d_out, size_t out_stride, int nframes,
                                    const mlvfs_amd_look_t *look, const mlvfs_amd_look16_t *look16, void *stream);
/* mlvfs_amd_render_resampled_dev, _look_dev and _deep_dev with AMaZE as the demosaic: the same arguments, mlvfs_amd_render1_amaze_dev's
 * checks with this route's geometry, its work memory with its zeroing rule, its sub-batches and its halving on a failed reservation.
 * Each runs step 1, the library's AMaZE for the batch, then steps 3 to 5 in one pass.                                               */
int    mlvfs_amd_render_resampled_amaze_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow, int oh,
                                            void *d_out, size_t out_stride, int nframes, void *stream);
int    mlvfs_amd_render_resampled_amaze_look_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow,
                                                 int oh, void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look_t *look, void *stream);
int    mlvfs_amd_render_resampled_amaze_deep_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_params, int ow,
                                                 int oh, void *d_out, size_t out_stride, int nframes, const mlvfs_amd_look16_t *look,
                                                 void *stream);
/* Which demosaic mlvfs_amd_mount_rgb_resampled, mlvfs_amd_mount_jpeg_resampled and mlvfs_amd_mount_rgb16_resampled use: 0 the linear
 * filter (the default), 1 AMaZE.  No serve-order state: it may change between serving calls.  With 1 set, whatever
 * mlvfs_amd_mount_set_demosaic says: the three calls render through this section's route, with the resampled route's placement,
 * growth, JPEG encoding, fallback flag, results[], sizes[] and look handling; mlvfs_amd_mount_rgb_resampled_size and
 * mlvfs_amd_mount_rgb16_resampled_size are 0 for a frame AMaZE does not take and the three calls refuse it.  With 0 nothing changes,
 * the refusal of the three calls under mlvfs_amd_mount_set_demosaic(mount, 1) included.  A handle that never calls this serves byte
 * for byte and launch for launch what it served before.  MLVFS_AMD_ERR_ARG: a null handle, another value.                            */
int    mlvfs_amd_mount_set_resample_demosaic(void *mount, int which);
/* Test hook, host only: how a launch of nframes frames is divided among k_amz_resample_x16's workgroups -- out = { 1 where the sizes
 * allow the fast form (width % 8 == 0 and 2 ow >= width; the alignment is the caller's), the most source columns of a strip, uo: the
 * output columns of a strip, the strips, bo: the output rows of a band, the bands, the source rows a band covers at least, the source
 * rows of a step }; the four numbers of the plan are 0 where the first is.  Strip k begins at output column k uo, band k at output row
 * k bo: those are the seams.  A strip's source columns run from floor(us0 W / ow) rounded down to 8 up to ceil(us1 W / ow) rounded up
 * to 8; a band's source rows from floor(v0 H / oh) up to ceil(v1 H / oh), walked a step at a time from the first.                   */
int    mlvfs_amd_test_amz_resample_plan(int width, int height, int ow, int oh, int nframes, int32_t out[8]);

/* -- a clip's frames as device-resident tensors (csrc/k_tensor.hip, csrc/tensor.cpp, csrc/mount.cpp) ------------------ */
/* The frame the mount would have served, written into the caller's device memory as a tensor: nothing crosses the link.  The definition
 * is this project's (mlvfs_amd/tensor.py restates it in numpy).  Two kinds:
 * RGB.    The source is a rendering exactly as a file route produces it: ph x pw pixels, interleaved R, G, B; 8-bit samples behind the
 *         mlvfs_amd_mount_rgb* routes (with the handle's look if one is set), 16-bit samples behind the mlvfs_amd_mount_rgb16* routes
 *         through the deep look of the call (an identity shaper and n = 0: linear light).  C = 3.  v = the sample;
 *         unit = fl32(1 / 255) or fl32(1 / 65535), the double quotient rounded once to binary32.
 * Bayer.  The source is the frame mlvfs_amd_mount_dng would have served: after every stage, 16-bit mosaic, RGGB.  C = 4 planes of
 *         floor(H / 2) x floor(W / 2): R (2Y, 2X), G1 (2Y, 2X + 1), G2 (2Y + 1, 2X), B (2Y + 1, 2X + 1); an odd last row or column is
 *         never read.  black and range = max(white - black, 1) from the header written for that frame in its final state (after a
 *         dual-ISO conversion the x4 levels, so they differ from frame to frame in a mixed clip).  v = px - black as a signed integer,
 *         clamped at neither end.  unit = fl32(1.0 / range), divided in double.  |black| > 2^30 is refused.
 * The element of channel c:
 *   F32   y = fl32(fl32(fl32(v) unit) scale_c), out = fl32(y + bias_c): three operations, each rounded to binary32 on its own, never fused
 *   F16   that value converted by round-to-nearest-even: results below 2^-14 become subnormal halves, overflow gives infinity
 *   BF16  that value converted by round-to-nearest-even
 *   U8    8-bit RGB sources only: the sample itself, re-laid out         U16   16-bit RGB sources: the sample; Bayer: the raw px
 *   For U8 and U16 scale and bias are not read; any other pair of source and integer dtype is refused.
 * scale_c, bias_c: binary32 from the caller, each finite and either zero or of magnitude within [2^-64, 2^64]; anything else is refused.
 *   Inside that range no intermediate binary32 is subnormal: the only gradual underflow of the definition is the conversion to half.
 * Layout.  NCHW: C planes of ph x pw per frame; NHWC: C interleaved.  Frames lie out_stride bytes apart, a multiple of the element's size
 *   and at least C ph pw elements; bytes between frames are never touched.
 * Not built: the tensor written from inside the tone kernels, a proxy handle, JPEG, other CFA orders, the drop-in symbols.          */
#define MLVFS_AMD_TENSOR_RGB       0
#define MLVFS_AMD_TENSOR_BAYER     1
#define MLVFS_AMD_TENSOR_HALF      0     /* the rendering of mlvfs_amd_mount_rgb / _rgb16 */
#define MLVFS_AMD_TENSOR_FULL      1     /* of mlvfs_amd_mount_rgb_full / _rgb16_full */
#define MLVFS_AMD_TENSOR_SCALED    2     /* of mlvfs_amd_mount_rgb_scaled / _rgb16_scaled, ow x oh */
#define MLVFS_AMD_TENSOR_RESAMPLED 3     /* of mlvfs_amd_mount_rgb_resampled / _rgb16_resampled, ow x oh */
#define MLVFS_AMD_TENSOR_F32       0
#define MLVFS_AMD_TENSOR_F16       1
#define MLVFS_AMD_TENSOR_BF16      2
#define MLVFS_AMD_TENSOR_U8        3
#define MLVFS_AMD_TENSOR_U16       4
#define MLVFS_AMD_TENSOR_NCHW      0
#define MLVFS_AMD_TENSOR_NHWC      1
/* What a tensor call asks for.  For Bayer only kind, dtype, layout, scale and bias are read.  The device calls below read dtype, layout,
 * scale and bias.                                                                                                                   */
typedef struct {
    int32_t kind;                        /* MLVFS_AMD_TENSOR_RGB, _BAYER */
    int32_t size;                        /* MLVFS_AMD_TENSOR_HALF .. _RESAMPLED */
    int32_t ow, oh;                      /* _SCALED, _RESAMPLED */
    int32_t gain_q8;                     /* 1 .. 65535, 256 is unity */
    int32_t dtype;                       /* MLVFS_AMD_TENSOR_F32 .. _U16 */
    int32_t layout;                      /* MLVFS_AMD_TENSOR_NCHW, _NHWC */
    int32_t reserved;                    /* 0 */
    const mlvfs_amd_look16_t *look16;    /* the deep look of a 16-bit rendering, or NULL: the 8-bit rendering */
    float scale[4], bias[4];
} mlvfs_amd_tensor_spec_t;
/* The pass alone, on a caller's renderings: nframes renderings of pw x ph pixels of three src_bits-bit samples (8 or 16), src_stride
 * bytes apart -> their tensors, out_stride bytes apart.  Never in place; the source is not written.  Asynchronous on `stream`; every
 * check happens before any device work and follows no pointer: nulls, pw, ph >= 1 and pw ph < 2^28, a negative count, src_bits, a dtype
 * or layout that does not exist or is illegal for the source, scale or bias outside the range above (float dtypes), a source or a
 * destination off its element's boundary, strides too small or no multiple of the element, a destination that overlaps the source.
 * pw a multiple of 8 with both bases and strides 16-byte aligned takes the fast form (k_tensor_rgb_x8: 8 pixels per lane, 24 or 48
 * source bytes as 64- and 128-bit loads, three runs of 8 elements or one of 24), anything else one pixel per lane (k_tensor_rgb_generic). */
int    mlvfs_amd_tensor_rgb_dev(const void *d_src, size_t src_stride, int pw, int ph, int src_bits, const mlvfs_amd_tensor_spec_t *spec,
                                void *d_out, size_t out_stride, int nframes, void *stream);
/* What the Bayer pass reads per frame, from the frame's headers as they are: out = { black, range (reported as at most 2^31 - 1; unit
 * is of the range itself), the bits of unit, 0 }.  Host code.  MLVFS_AMD_ERR_ARG, with out untouched: a null pointer, |black| > 2^30. */
int    mlvfs_amd_tensor_bayer_params(const struct frame_headers *frame_headers, int32_t out[4]);
/* The pass alone, on a caller's frames: nframes frames of width x height 16-bit pixels `stride` bytes apart -> their tensors of 4 planes
 * of (height / 2) x (width / 2), frame k with the four parameters d_levels[4 k ..] (device memory, as mlvfs_amd_tensor_bayer_params
 * yields them; the pass reads black and unit).  The checks are mlvfs_amd_tensor_rgb_dev's, with width, height >= 2, width height
 * < 2^28, an odd source address or stride and levels off a 4-byte boundary or overlapped by the destination.  width a multiple of 16
 * with both bases and strides 16-byte aligned takes the fast form (k_tensor_bayer_x8: 16 pixels of each of the two rows of a superpixel
 * row per lane, 8 elements to each of four planes or 32 interleaved), anything else one superpixel per lane (k_tensor_bayer_generic). */
int    mlvfs_amd_tensor_bayer_dev(const void *d_frames, size_t stride, int width, int height, const int32_t *d_levels,
                                  const mlvfs_amd_tensor_spec_t *spec, void *d_out, size_t out_stride, int nframes, void *stream);
/* Frames first .. first + count - 1 as tensors in the caller's device memory, out_stride bytes apart: the stages, the serve-order state
 * and results[] of every other serving call; only the last step differs.  The rendering lies where the file routes leave it, and one
 * launch of the pass per run of frames writes d_out in the place of the downloads; a Bayer tensor is read from the final frames.  The
 * handle's look, demosaic settings, dark frame and flat field apply as they do to the file routes.  The call synchronises the library's
 * stream before it returns.  May be interleaved with the other serving calls on one handle; a handle that never makes a tensor call
 * serves byte for byte and launch for launch what it served before.  MLVFS_AMD_ERR_ARG before anything is launched: nulls, a spec
 * outside the definition, a handle with mlvfs_amd_mount_set_proxy(2), a shape the route does not take, an out_stride below
 * mlvfs_amd_mount_tensor_bytes or no multiple of the element, d_out that is not device memory on the handle's device (a host pointer,
 * another device's) or off the element's boundary.                                                                                  */
int    mlvfs_amd_mount_tensor(void *mount, int first, int count, void *d_out, size_t out_stride, const mlvfs_amd_tensor_spec_t *spec,
                              int batch_frames, int io_threads, int *results);
/* bytes of the tensor of frame `index`; 0 with the error set: no such frame, a spec outside the definition, a shape the route refuses */
size_t mlvfs_amd_mount_tensor_bytes(const void *mount, int index, const mlvfs_amd_tensor_spec_t *spec);

/* self tests that need no GPU (selection networks, LUT identities): 0 = pass */
int mlvfs_amd_selftest_host(void);
/* Test hook, host only: the two selection networks of k_frame_p5's pair step (csrc/median_nets.h) on the caller's values, n sets at a
 * time.  net 4: mlv_sort4, in[4] -> out[4] per set; net 5: mlv_insert4, in[0..3] (sorted) and in[4] -> the sorted five, out[5] per set. */
int mlvfs_amd_test_median_net(int net, int n, const int32_t *in, int32_t *out);
/* the library's host EV tables against raw2ev_lin[16384] (index = pixel - black) and ev2raw[24 * 32768] (index 0 = EV -10 * 32768):
 * 0 = identical (main.c:128-196; no GPU needed) */
int mlvfs_amd_selftest_tables(const int32_t *raw2ev_lin, const int32_t *ev2raw);

#ifdef __cplusplus
}
#endif
#endif

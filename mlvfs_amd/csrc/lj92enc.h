// lj92enc.h -- shared between csrc/lj92enc.cpp (host: Huffman tables, marker segments, the batch call) and csrc/k_lj92enc.hip
// (kernels); the mount (csrc/mount.cpp) encodes its batches through lje_encode_batch.
#pragma once
#include "common.h"

namespace mlv {

constexpr int LJE_PER_THREAD = 16;                      // pixels (or stream bytes) per thread
constexpr int LJE_BLOCK = 256 * LJE_PER_THREAD;         // pixels per workgroup
constexpr int LJE_SCAN_THREADS = 1024;                  // threads of the one workgroup per frame that scans its blocks' offsets
constexpr int LJE_HIST = 20;                            // counters per frame: 17 classes, 17-bit differences, a value beyond the
                                                        // delinearisation table, one spare

enum { LJE_OK = 0, LJE_DIFF17 = 1, LJE_TABLE = 2, LJE_NOFIT = 3, LJE_DELIN = 4 };   // 0..3: MLVFS_AMD_LJ92ENC_* of the header

// what the pack kernels know of a frame: its table, its marker segments, where its bits go (device memory, one upload per batch)
struct LjeFrame {
    uint8_t len[17];           // per class: length of its Huffman code
    uint8_t head_len;
    uint16_t code[17];
    uint8_t head[64];          // SOI, SOF3, DHT, SOS
    uint32_t status;           // not LJE_OK: the kernels leave the frame alone
    uint32_t bits_at;          // first dword of the frame's unstuffed bit stream in the batch's bit buffer
};

// what comes back in one copy
struct LjeOut {
    uint32_t length;           // the whole stream, SOI .. EOI
    uint32_t status;           // LJE_OK or LJE_NOFIT
    uint32_t bits, stuffed;    // bits of the entropy-coded segment, 0xFF bytes in it
};

struct LjeResult {
    uint32_t length = 0;
    int status = LJE_OK;
    int max_class = 0;         // highest SSSS in use (17: a 17-bit difference)
    const char *why = nullptr; // LJE_TABLE: what the reference's table construction runs into
};

inline uint32_t lje_blocks(uint64_t npix) { return (uint32_t)((npix + LJE_BLOCK - 1) / LJE_BLOCK); }
// blocks a thread of the scan kernels sums before the workgroup's scan (k_lje_scan_bits, k_lje_scan_ff and the test hook)
__host__ __device__ inline uint32_t lje_scan_per(uint32_t nb) { return (nb + LJE_SCAN_THREADS - 1) / LJE_SCAN_THREADS; }
// the batch's fixed scratch: frame pointers, histograms, per-block class counts, bit and 0xFF offsets, frame records, results
size_t lje_fixed_bytes(uint32_t npix, int nframes);

// After the histograms are known: room for the batch's bit streams (bits_bytes) and, where the caller has none yet, for the
// streams themselves (a frame needs at most stream_bytes).  *d_out / *out_stride hold the caller's buffer if it has one.
struct LjeRoom {
    virtual int get(size_t bits_bytes, size_t stream_bytes, void **d_bits, uint8_t **d_out, size_t *out_stride) = 0;
    virtual ~LjeRoom() {}
};

// n frames of width x height values (device pointers in h_src[]) -> n complete JPEG streams.  One host round trip for the
// tables, one copy for lengths and states; synchronises s.  Returns an MLVFS_AMD_* code; per-frame refusals are in res[].
int lje_encode_batch(const uint16_t *const *h_src, int n, int width, int height, int bitdepth, const uint16_t *d_delin, int delin_len,
                     void *d_fixed, LjeRoom &room, uint8_t **d_out_used, size_t *out_stride_used, LjeResult *res, hipStream_t s);

// kernels (k_lj92enc.hip)
int lje_launch_hist(const uint16_t *const *d_src, const uint16_t *d_delin, int delin_len, int width, uint32_t npix, int bitdepth, int n,
                    uint32_t *d_hist, uint32_t *d_blockhist, hipStream_t s);
int lje_launch_pack(const uint16_t *const *d_src, const uint16_t *d_delin, int delin_len, int width, uint32_t npix, int bitdepth, int n,
                    const LjeFrame *d_tabs, const uint32_t *d_blockhist, uint32_t *d_off, uint32_t *d_ffoff, uint32_t *d_bits, uint8_t *d_out,
                    size_t out_stride, LjeOut *d_res, hipStream_t s);

}  // namespace mlv

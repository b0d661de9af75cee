// lj92.h -- shared between csrc/lj92.cpp (host: stream parsing, tables, buffers) and csrc/k_lj92.hip (kernels)
#pragma once
#include "common.h"

namespace mlv {

constexpr uint32_t LJ_TAIL = 128;          // zero bytes kept behind the unstuffed data (look-ahead of the last symbols)
constexpr int LJ_ERR_CODE = 1;             // a bit pattern that is no Huffman code / a pixel decoded from bits behind the data
constexpr int LJ_ERR_SHORT = 2;            // fewer symbols than pixels
constexpr int LJ_L1_BITS = 11;             // first-level Huffman look-up: 2048 entries
constexpr int LJ_LUT_MAX = 3584;           // both levels together (7 KiB of LDS): 48 second-level tables of 32 entries

// one frame's view of the work buffers (all pointers are device memory)
struct LjFrame {
    const uint8_t *raw;        // entropy-coded segment as stored (0xFF 0x00 stuffing inside)
    uint32_t raw_len;
    uint8_t *ust;              // unstuffed bytes, 16-byte aligned, followed by LJ_TAIL zero bytes
    uint32_t *ust_len;
    uint32_t *blk_drop;        // stuffed zeros per 4 KiB block, then their exclusive prefix sums
    const uint16_t *lut;       // two-level table, see lut_entry() in k_lj92.hip
    int huffbits, lut_entries;
    uint16_t *cmap;            // [nwg * 256][32] chunk maps: exit offset | symbols << 5
    uint2 *wmap, *gmap;        // [nwg][32], [ngrp][32]: {exit offset, symbols}
    uint2 *smap;               // [nwg][16][32]: the same for the 16 segments of 16 chunks inside each workgroup
    uint2 *wstart, *gstart;    // [nwg], [ngrp]: {true entry offset, index of the first symbol}
    int32_t *diff;             // [W * H] differences, then the per-row recurrence values
    int32_t *colsum;           // [16][W] sums of e over segments of rows
    uint16_t *out;             // xres x yres pixels, untiled
    int W, H, bits, pred;      // the JPEG's own dimensions, sample precision, predictor (0..7)
    int xres, yres;            // the video frame the decoded values are re-read as (main.c:646-667)
    uint32_t nwg, ngrp;        // 8 KiB workgroup windows over raw_len bytes, groups of 32 of them
    int *err;
};

constexpr int LJ_WAVE_MAX_H = 8192;        // predictor 7 keeps two anti-diagonals (indexed by row) in LDS

// k_lj_rows' dynamic LDS, ONE rule for the launcher (how many bytes) and the kernel (where a frame's row goes): the carries of the
// widest frame's blocks of 32 columns (+ 2), then room for the widest row of the batch that can be staged at all -- min(max_w,
// LJ_ROW_LDS) values, one spare word per 32 (+ 2).  A row of w <= LJ_ROW_LDS values is staged there whatever else is in its batch;
// a longer one is worked on in place in global memory.  65535 values at most: 2050 carries + 8450 ints = 50 200 bytes.
constexpr int LJ_ROW_LDS = 8192;
struct LjRowPlan {
    bool staged;                 // the row of w values goes through LDS
    uint32_t stage_off;          // bytes from the start of the launch's LDS to the staged row (behind the carries)
    uint32_t stage_end;          // bytes up to which a staged row of w values reaches (== stage_off when it is not staged)
    uint32_t lds_bytes;          // what a launch for rows of up to max_w values asks for
};
__host__ __device__ inline LjRowPlan lj_row_plan(int w, int max_w)
{
    const int cap = max_w < LJ_ROW_LDS ? max_w : LJ_ROW_LDS;
    LjRowPlan p;
    p.staged = w <= cap;
    p.stage_off = (uint32_t)((max_w + 31) / 32 + 2) * (uint32_t)sizeof(long long);
    p.lds_bytes = p.stage_off + (uint32_t)(cap + cap / 32 + 2) * (uint32_t)sizeof(int);
    p.stage_end = p.stage_off + (p.staged && w > 0 ? (uint32_t)(w + ((w - 1) >> 5)) * (uint32_t)sizeof(int) : 0u);      // value i lies at i + (i >> 5)
    return p;
}

// preds: bit p set when some frame of the batch uses predictor p (the rarely used ones have kernels of their own)
int lj92_launch(const LjFrame *d_frames, int nframes, uint32_t max_raw, uint32_t max_nwg, uint32_t max_ngrp, int max_w, int max_h,
                unsigned preds, hipStream_t s);

}  // namespace mlv

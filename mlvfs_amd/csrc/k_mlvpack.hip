// k_mlvpack.hip -- the two passes that turn 16-bit frames in HBM back into what an MLV file stores (csrc/mlvwriter.cpp):
//
//   k_mlv_tile_*   the four Bayer channels of a frame as the four quadrants of one image, what an MLV writer hands to lj92_encode.
//                  The inverse of the untiling loop of get_image_data (mlvfs/main.c:656-667): tiled row y, column x holds source
//                  pixel (ty, tx) with ty = (2y) % H + (2y) / H, tx = (2x) % W + (2x) / W.  For even W and H that is a bijection:
//                  source pixel (sy, sx) goes to row sy / 2 + (sy & 1) * H / 2, column sx / 2 + (sx & 1) * W / 2.  (For an odd size
//                  the reference's map writes some rows twice and others never; the launcher refuses those.)
//   k_mlv_pack_*   16-bit pixels -> packed payload, the inverse of k_unpack.hip: pixel i is bits [i*bpp, (i+1)*bpp) of an MSB-first
//                  bit stream stored as little-endian 16-bit words (mlvfs/raw.h:41-79).  Exactly ceil(npix * bpp / 16) words are
//                  written; pixels are masked to bpp bits.
//
// Both are HBM-bound (tile: 2 B read + 2 B written per pixel; pack at 14 bits: 2 B + 1.75 B, k_unpack_x16<14>'s traffic the other
// way round).  One lane moves 16 bytes per load; the lanes of a wave are contiguous in the source and in the destination; frames
// are batched in grid.y.
//   k_mlv_tile_x<16 | 8, SHIFT> : one lane = 16 (8) consecutive pixels of one source row = two (one) 128-bit loads; their even and
//                  their odd pixels leave as two runs of 16 (8) bytes, one into the left half of the destination row, one into the right.
//   k_mlv_tile_generic<SHIFT> : any even width and height; one lane = one destination pixel.
//   k_mlv_pack_x16<14 | 12 | 10, SHIFT> : one lane = 16 pixels = two 128-bit loads and 7 / 6 / 5 coalesced dword stores.
//   k_mlv_pack_generic<SHIFT> : any bpp in 1..16, any length; one lane = one output word (the pixels that touch it: 2 at 14 bits, 16 at 1).
//
// A clip rewritten at another bit depth (mlvfs_amd_mlv_transcode_bits, `mlv_dump -b`).  For a frame of bpp bits and a
// requested out_bpp, d = out_bpp - bpp:
//     out = px >> -d   (d < 0: truncation, no rounding, no dither)        out = px << d   (d > 0)        out = px   (d = 0)
// after the dark frame, if any, was subtracted at the source's depth (stage 0, k_cal.hip).  The shift rides inside the pass a route
// makes anyway.  In the passes above it is the compile-time SHIFT with d as the last kernel argument: every pixel read is shifted
// first (tile: LJ92 source to LJ92 output; pack: LJ92 source to plain output, in front of the mask).  Without SHIFT no instruction
// depends on d: a call without conversion runs the code it ran before there was a conversion.  The passes that read a packed stream:
//   k_mlv_repack_x16<IN, OUT>, IN, OUT in {14, 12, 10} : packed stream in, packed stream out; one lane = 16 pixels = IN / 2 coalesced
//                  dword loads, unpack, the dark plane (optional: two 128-bit loads), shift, OUT / 2 coalesced dword stores.
//                  3.25 B per pixel at 14 -> 12 where unpack + pack move 7.25.  IN == OUT is for a dark frame alone.
//   k_mlv_repack_generic : any depths in 1..16, any length, 2-byte alignment; one lane = one output word.
//   k_mlv_unpack_shift_x16<IN> : k_cal_unpack_x16<IN, true, false> with the shift (plain / LZMA source to the encoder); the plane is optional.
//   k_mlv_shift_generic : in place, one pixel per lane -- the extra pass behind the generic unpack, for the shapes
//                  k_mlv_unpack_shift_x16 does not take.
// Pad bytes between frames are never touched.
#include "clip.h"
#include "k_cal_dev.h"
#include "k_unpack_dev.h"

namespace mlv {

// the even (low) and the odd (high) halves of two dwords of pixel pairs
__device__ __forceinline__ uint32_t evens(uint32_t a, uint32_t b) { return (a & 0xFFFFu) | (b << 16); }
__device__ __forceinline__ uint32_t odds(uint32_t a, uint32_t b) { return (a >> 16) | (b & 0xFFFF0000u); }

// d > 0: << d, d < 0: >> -d; the result is kept to 16 bits (a decoded value above its depth must not reach the neighbouring pixel)
__device__ __forceinline__ uint32_t shift_px(uint32_t v, int d) { return (d >= 0 ? v << d : v >> -d) & 0xFFFFu; }

// two pixels in a dword
__device__ __forceinline__ uint32_t shift_px2(uint32_t two, int d)
{
    return d >= 0 ? (two << d) & (((0xFFFFu << d) & 0xFFFFu) * 0x10001u) : (two >> -d) & ((0xFFFFu >> -d) * 0x10001u);
}

// what a pass with the compile-time SHIFT does to a pixel (a pair) it has read: without SHIFT d is not looked at
template <bool SHIFT>
__device__ __forceinline__ uint32_t shifted(uint32_t v, int d) { if constexpr (SHIFT) return shift_px(v, d); else return v; }
template <bool SHIFT>
__device__ __forceinline__ uint32_t shifted2(uint32_t two, int d) { if constexpr (SHIFT) return shift_px2(two, d); else return two; }

// PX = 16: W % 16 == 0; PX = 8: W % 8 == 0.  groups = W / PX * H per frame, in source order.
template <int PX, bool SHIFT>
__global__ __launch_bounds__(256) void k_mlv_tile_x(const uint8_t *__restrict__ frames, size_t stride, uint8_t *__restrict__ out,
                                                    size_t out_stride, uint32_t groups, uint32_t groups_per_row, uint32_t w, uint32_t h, int d)
{
    const uint4 *src = (const uint4 *)(frames + (size_t)blockIdx.y * stride);
    uint16_t *dst = (uint16_t *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        const uint32_t sy = g / groups_per_row, gx = g - sy * groups_per_row;
        const uint32_t dy = (sy >> 1) + (sy & 1u) * (h >> 1);
        uint16_t *row = dst + (size_t)dy * w + (size_t)gx * (PX / 2);
        if (PX == 16) {
            const uint4 a = src[(size_t)g * 2], b = src[(size_t)g * 2 + 1];
            uint4 e, o;
            e.x = evens(a.x, a.y); e.y = evens(a.z, a.w); e.z = evens(b.x, b.y); e.w = evens(b.z, b.w);
            o.x = odds(a.x, a.y);  o.y = odds(a.z, a.w);  o.z = odds(b.x, b.y);  o.w = odds(b.z, b.w);
            e.x = shifted2<SHIFT>(e.x, d); e.y = shifted2<SHIFT>(e.y, d); e.z = shifted2<SHIFT>(e.z, d); e.w = shifted2<SHIFT>(e.w, d);
            o.x = shifted2<SHIFT>(o.x, d); o.y = shifted2<SHIFT>(o.y, d); o.z = shifted2<SHIFT>(o.z, d); o.w = shifted2<SHIFT>(o.w, d);
            *(uint4 *)row = e;
            *(uint4 *)(row + (w >> 1)) = o;
        } else {
            const uint4 a = src[g];
            uint2 e, o;
            e.x = shifted2<SHIFT>(evens(a.x, a.y), d); e.y = shifted2<SHIFT>(evens(a.z, a.w), d);
            o.x = shifted2<SHIFT>(odds(a.x, a.y), d);  o.y = shifted2<SHIFT>(odds(a.z, a.w), d);
            *(uint2 *)row = e;
            *(uint2 *)(row + (w >> 1)) = o;
        }
    }
}

template <bool SHIFT>
__global__ __launch_bounds__(256) void k_mlv_tile_generic(const uint8_t *__restrict__ frames, size_t stride, uint8_t *__restrict__ out,
                                                          size_t out_stride, uint32_t npix, uint32_t w, uint32_t h, int d)
{
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint16_t *dst = (uint16_t *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x) {
        const uint32_t y = k / w, x = k - y * w;
        const uint32_t ty = y < (h >> 1) ? 2 * y : 2 * y - h + 1, tx = x < (w >> 1) ? 2 * x : 2 * x - w + 1;
        dst[k] = (uint16_t)shifted<SHIFT>(src[(size_t)ty * w + tx], d);
    }
}

// 16 pixels of BPP bits (BPP even) -> BPP / 2 little-endian dwords of the MSB-first stream
template <int BPP>
__device__ __forceinline__ void pack_x16(const uint32_t (&px)[16], uint32_t (&le)[BPP / 2])
{
    constexpr uint32_t mask = (1u << BPP) - 1u;
    uint32_t s[BPP / 2];
#pragma unroll
    for (int i = 0; i < BPP / 2; i++) s[i] = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int bit = BPP * k, wi = bit >> 5, sh = bit & 31;
        const uint32_t v = px[k] & mask;
        if (sh + BPP <= 32) {
            s[wi] |= v << (32 - BPP - sh);
        } else {
            s[wi] |= v >> (sh + BPP - 32);
            s[wi + 1] |= v << (64 - BPP - sh);
        }
    }
#pragma unroll
    for (int i = 0; i < BPP / 2; i++) le[i] = (s[i] << 16) | (s[i] >> 16);      // 32 stream bits -> two little-endian words
}

// BPP: the depth written
template <int BPP, bool SHIFT>
__global__ __launch_bounds__(256) void k_mlv_pack_x16(const uint8_t *__restrict__ frames, size_t stride, uint8_t *__restrict__ packed,
                                                      size_t packed_stride, uint32_t groups, int d)
{
    constexpr int NW = BPP / 2;
    const uint4 *src = (const uint4 *)(frames + (size_t)blockIdx.y * stride);
    uint32_t *dst = (uint32_t *)(packed + (size_t)blockIdx.y * packed_stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint32_t px[16], le[NW];
        split_x16(src[(size_t)g * 2], src[(size_t)g * 2 + 1], px);
#pragma unroll
        for (int k = 0; k < 16; k++) px[k] = shifted<SHIFT>(px[k], d);
        pack_x16<BPP>(px, le);
#pragma unroll
        for (int i = 0; i < NW; i++) dst[(size_t)g * NW + i] = le[i];
    }
}

// word j holds stream bits [16j, 16j + 16): the pixels floor(16j / bpp) .. floor((16j + 15) / bpp), as far as the frame has them
// (bpp: the depth written)
template <bool SHIFT>
__global__ __launch_bounds__(256) void k_mlv_pack_generic(const uint8_t *__restrict__ frames, size_t stride, uint8_t *__restrict__ packed,
                                                          size_t packed_stride, uint32_t npix, uint32_t nwords, int bpp, int d)
{
    const uint16_t *src = (const uint16_t *)(frames + (size_t)blockIdx.y * stride);
    uint16_t *dst = (uint16_t *)(packed + (size_t)blockIdx.y * packed_stride);
    const uint32_t mask = (1u << bpp) - 1u;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < nwords; j += gridDim.x * blockDim.x) {
        const uint32_t bit0 = j * 16u;
        const uint32_t first = bit0 / (uint32_t)bpp;
        uint32_t last = (bit0 + 15u) / (uint32_t)bpp;
        if (last > npix - 1) last = npix - 1;
        uint32_t word = 0;
        for (uint32_t i = first; i <= last; i++) {
            const uint32_t v = shifted<SHIFT>(src[i], d) & mask;
            // the pixel's lowest bit is stream bit i * bpp + bpp - 1; stream bit b of this word is bit 15 - (b - bit0)
            const int sh = 15 - (int)(i * (uint32_t)bpp + (uint32_t)bpp - 1u - bit0);
            word |= sh >= 0 ? v << sh : v >> -sh;
        }
        dst[j] = (uint16_t)word;
    }
}

// ---- the passes that read a packed stream at one depth and deliver another --------------------------------------
// the lane's 16 pixels less the dark plane's (k_cal_dev.h's rule: clamp(px - dark + black_d, 0, 2^IN - 1))
__device__ __forceinline__ void dark_x16(uint32_t (&px)[16], const uint4 *__restrict__ dark, size_t g, int black_d, int top)
{
    uint32_t dk[16];
    split_x16(dark[g * 2], dark[g * 2 + 1], dk);
#pragma unroll
    for (int k = 0; k < 16; k++) px[k] = cal_px<true, false>(px[k], dk[k], 0, black_d, 0, top);
}

// dark: nullptr or the plane, 16-byte aligned; a frame is `groups` runs of 16 pixels
template <int IN, int OUT>
__global__ __launch_bounds__(256) void k_mlv_repack_x16(const uint8_t *__restrict__ packed, size_t packed_stride, uint8_t *__restrict__ out,
                                                        size_t out_stride, const uint4 *__restrict__ dark, uint32_t groups, int black_d)
{
    constexpr int NI = IN / 2, NO = OUT / 2, D = OUT - IN;
    const uint32_t *src = (const uint32_t *)(packed + (size_t)blockIdx.y * packed_stride);
    uint32_t *dst = (uint32_t *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint32_t s[NI], px[16], le[NO];
#pragma unroll
        for (int i = 0; i < NI; i++) s[i] = stream_word(src[(size_t)g * NI + i]);
        unpack_x16<IN>(s, px);
        if (dark) dark_x16(px, dark, g, black_d, (1 << IN) - 1);
#pragma unroll
        for (int k = 0; k < 16; k++) {                                                        // IN bits at most: OUT bits at most
            if constexpr (D >= 0) px[k] <<= D; else px[k] >>= -D;
        }
        pack_x16<OUT>(px, le);
#pragma unroll
        for (int i = 0; i < NO; i++) dst[(size_t)g * NO + i] = le[i];
    }
}

// output word j holds output stream bits [16j, 16j + 16): every pixel that touches it is read from the input stream (its two words,
// the second one only where the frame has it), subtracted, shifted and masked
__global__ __launch_bounds__(256) void k_mlv_repack_generic(const uint8_t *__restrict__ packed, size_t packed_stride, uint8_t *__restrict__ out,
                                                            size_t out_stride, const uint16_t *__restrict__ dark, uint32_t npix, uint32_t in_words,
                                                            uint32_t out_words, int bpp, int out_bpp, int black_d)
{
    const uint16_t *src = (const uint16_t *)(packed + (size_t)blockIdx.y * packed_stride);
    uint16_t *dst = (uint16_t *)(out + (size_t)blockIdx.y * out_stride);
    const uint32_t in_mask = (1u << bpp) - 1u, out_mask = (1u << out_bpp) - 1u;
    const int d = out_bpp - bpp;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < out_words; j += gridDim.x * blockDim.x) {
        const uint32_t bit0 = j * 16u;
        const uint32_t first = bit0 / (uint32_t)out_bpp;
        uint32_t last = (bit0 + 15u) / (uint32_t)out_bpp;
        if (last > npix - 1) last = npix - 1;
        uint32_t word = 0;
        for (uint32_t i = first; i <= last; i++) {
            const uint32_t bit = i * (uint32_t)bpp, wi = bit >> 4, sh = bit & 15u;
            const uint32_t two = ((uint32_t)src[wi] << 16) | (wi + 1 < in_words ? (uint32_t)src[wi + 1] : 0u);
            uint32_t v = (two >> (32 - bpp - (int)sh)) & in_mask;
            if (dark) v = cal_px<true, false>(v, dark[i], 0, black_d, 0, (int)in_mask);
            v = shift_px(v, d) & out_mask;
            const int pos = 15 - (int)(i * (uint32_t)out_bpp + (uint32_t)out_bpp - 1u - bit0);
            word |= pos >= 0 ? v << pos : v >> -pos;
        }
        dst[j] = (uint16_t)word;
    }
}

template <int IN>
__global__ __launch_bounds__(256) void k_mlv_unpack_shift_x16(const uint8_t *__restrict__ packed, size_t packed_stride, uint8_t *__restrict__ out,
                                                              size_t out_stride, const uint4 *__restrict__ dark, uint32_t groups, int black_d, int d)
{
    constexpr int NW = IN / 2;
    const uint32_t *src = (const uint32_t *)(packed + (size_t)blockIdx.y * packed_stride);
    uint4 *dst = (uint4 *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint32_t s[NW], px[16];
#pragma unroll
        for (int i = 0; i < NW; i++) s[i] = stream_word(src[(size_t)g * NW + i]);
        unpack_x16<IN>(s, px);
        if (dark) dark_x16(px, dark, g, black_d, (1 << IN) - 1);
#pragma unroll
        for (int k = 0; k < 16; k++) px[k] = shift_px(px[k], d);
        uint4 lo, hi;
        join_x16(px, lo, hi);
        dst[(size_t)g * 2] = lo;
        dst[(size_t)g * 2 + 1] = hi;
    }
}

__global__ __launch_bounds__(256) void k_mlv_shift_generic(uint8_t *__restrict__ frames, size_t stride, uint32_t npix, int d)
{
    uint16_t *f = (uint16_t *)(frames + (size_t)blockIdx.y * stride);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x) f[k] = (uint16_t)shift_px(f[k], d);
}

// ---- the launchers ----------------------------------------------------------------------------------------------------------
// d_out != d_frames; w and h even (the callers check); every pixel shifted by d bits on the way (d > 0: left; 0: as it is)
int launch_mlv_tile(const void *d_frames, size_t stride, void *d_out, size_t out_stride, int w, int h, int d, int nframes, hipStream_t stream)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1)) { set_error("quadrant tiling takes even sizes, not %dx%d", w, h); return MLVFS_AMD_ERR_ARG; }
    if (d < -15 || d > 15) { set_error("a shift of %d bits", d); return MLVFS_AMD_ERR_ARG; }
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    // (h is even: a width of 8k pixels is whole groups of 16 as well)
    const int px = !fits_x16(npix, nframes, d_frames, stride, 16, d_out, out_stride, 16) ? 0 : (w % 16 == 0 ? 16 : (w % 8 == 0 ? 8 : 0));
    if (px) {
        const uint32_t gpr = (uint32_t)w / px, groups = gpr * (uint32_t)h;
        auto kern = px == 16 ? (d ? k_mlv_tile_x<16, true> : k_mlv_tile_x<16, false>) : (d ? k_mlv_tile_x<8, true> : k_mlv_tile_x<8, false>);
        hipLaunchKernelGGL(kern, dim3(grid_x(groups, 8192), nframes), dim3(256), 0, stream, (const uint8_t *)d_frames, stride, (uint8_t *)d_out,
                           out_stride, groups, gpr, (uint32_t)w, (uint32_t)h, d);
    } else {
        hipLaunchKernelGGL(d ? k_mlv_tile_generic<true> : k_mlv_tile_generic<false>, dim3(grid_x(npix, 16384), nframes), dim3(256), 0, stream,
                           (const uint8_t *)d_frames, stride, (uint8_t *)d_out, out_stride, npix, (uint32_t)w, (uint32_t)h, d);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

template <int BPP>
static auto pack_kernel(bool shift) { return shift ? k_mlv_pack_x16<BPP, true> : k_mlv_pack_x16<BPP, false>; }

// 16-bit frames of bpp bits -> packed payloads of out_bpp bits (out_bpp == bpp: masked, not shifted)
int launch_mlv_pack(const void *d_frames, size_t stride, void *d_packed, size_t packed_stride, uint32_t npix, int bpp, int out_bpp, int nframes,
                    hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    const int d = out_bpp - bpp;
    if (bpp < 1 || bpp > 16 || out_bpp < 1 || out_bpp > 16) {
        if (d) set_error("unsupported bits_per_pixel %d -> %d", bpp, out_bpp); else set_error("unsupported bits_per_pixel %d", bpp);
        return MLVFS_AMD_ERR_ARG;
    }
    if (npix >= (1u << 27)) { set_error("more than 2^27 pixels"); return MLVFS_AMD_ERR_ARG; }       // bit positions are 32-bit
    if (fast_depth(out_bpp) && fits_x16(npix, nframes, d_frames, stride, 16, d_packed, packed_stride, 4)) {
        const uint32_t groups = npix / 16;
        auto kern = out_bpp == 14 ? pack_kernel<14>(d != 0) : (out_bpp == 12 ? pack_kernel<12>(d != 0) : pack_kernel<10>(d != 0));
        hipLaunchKernelGGL(kern, dim3(grid_x(groups, 8192), nframes), dim3(256), 0, stream, (const uint8_t *)d_frames, stride, (uint8_t *)d_packed,
                           packed_stride, groups, d);
    } else {
        const uint32_t nwords = (uint32_t)(((uint64_t)npix * out_bpp + 15) / 16);
        hipLaunchKernelGGL(d ? k_mlv_pack_generic<true> : k_mlv_pack_generic<false>, dim3(grid_x(nwords, 16384), nframes), dim3(256), 0, stream,
                           (const uint8_t *)d_frames, stride, (uint8_t *)d_packed, packed_stride, npix, nwords, out_bpp, d);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// the dark plane as an x16 form takes it: none, or of the frames' depth and 16-byte aligned
static bool dark_x16_ok(const Calib *cal, int bpp) { return !cal || !cal->d_dark || (cal->top == (1 << bpp) - 1 && (uintptr_t)cal->d_dark % 16 == 0); }

// packed payloads of bpp bits -> packed payloads of out_bpp bits, the dark frame (optional) subtracted in between
int launch_mlv_repack(const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride, uint32_t npix, int bpp, int out_bpp, int nframes,
                      const Calib *cal, hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    const uint16_t *dark = cal ? cal->d_dark : nullptr;
    if (bpp < 1 || bpp > 16 || out_bpp < 1 || out_bpp > 16) { set_error("unsupported bits_per_pixel %d -> %d", bpp, out_bpp); return MLVFS_AMD_ERR_ARG; }
    if (npix >= (1u << 27)) { set_error("more than 2^27 pixels"); return MLVFS_AMD_ERR_ARG; }       // bit positions are 32-bit
    if (fast_depth(bpp) && fast_depth(out_bpp) && dark_x16_ok(cal, bpp) && fits_x16(npix, nframes, d_packed, packed_stride, 4, d_out, out_stride, 4)) {
        using Kern = void (*)(const uint8_t *, size_t, uint8_t *, size_t, const uint4 *, uint32_t, int);
        static const Kern table[3][3] = {
            { k_mlv_repack_x16<14, 14>, k_mlv_repack_x16<14, 12>, k_mlv_repack_x16<14, 10> },
            { k_mlv_repack_x16<12, 14>, k_mlv_repack_x16<12, 12>, k_mlv_repack_x16<12, 10> },
            { k_mlv_repack_x16<10, 14>, k_mlv_repack_x16<10, 12>, k_mlv_repack_x16<10, 10> },
        };
        const uint32_t groups = npix / 16;
        hipLaunchKernelGGL(table[(14 - bpp) / 2][(14 - out_bpp) / 2], dim3(grid_x(groups, 8192), nframes), dim3(256), 0, stream,
                           (const uint8_t *)d_packed, packed_stride, (uint8_t *)d_out, out_stride, (const uint4 *)dark, groups,
                           dark ? cal->black_d : 0);
    } else {
        const uint32_t in_words = (uint32_t)(((uint64_t)npix * bpp + 15) / 16), out_words = (uint32_t)(((uint64_t)npix * out_bpp + 15) / 16);
        hipLaunchKernelGGL(k_mlv_repack_generic, dim3(grid_x(out_words, 16384), nframes), dim3(256), 0, stream, (const uint8_t *)d_packed,
                           packed_stride, (uint8_t *)d_out, out_stride, dark, npix, in_words, out_words, bpp, out_bpp, dark ? cal->black_d : 0);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// in place: the pass more of launch_mlv_unpack_shift's fallback
static int launch_mlv_shift(void *d_frames, size_t stride, uint32_t npix, int d, int nframes, hipStream_t stream)
{
    if (d == 0) return MLVFS_AMD_OK;
    hipLaunchKernelGGL(k_mlv_shift_generic, dim3(grid_x(npix, 16384), nframes), dim3(256), 0, stream, (uint8_t *)d_frames, stride, npix, d);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// packed payloads of bpp bits -> 16-bit frames of out_bpp bits, the dark frame (optional) subtracted in between: one pass where
// k_unpack_x16 would run, else the generic unpack (and subtraction) and one in-place pass more
int launch_mlv_unpack_shift(const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride, uint32_t npix, int bpp, int out_bpp,
                            int nframes, const Calib *cal, hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    const uint16_t *dark = cal ? cal->d_dark : nullptr;
    if (bpp < 1 || bpp > 16 || out_bpp < 1 || out_bpp > 16) { set_error("unsupported bits_per_pixel %d -> %d", bpp, out_bpp); return MLVFS_AMD_ERR_ARG; }
    const bool fast = fast_depth(bpp) && dark_x16_ok(cal, bpp) && fits_x16(npix, nframes, d_packed, packed_stride, 4, d_out, out_stride, 16);
    if (!fast) {
        if (int rc = dark ? launch_cal_unpack(d_packed, packed_stride, d_out, out_stride, npix, bpp, nframes, *cal, stream)
                          : launch_unpack(d_packed, packed_stride, d_out, out_stride, 0, npix, bpp, nframes, stream)) return rc;
        return launch_mlv_shift(d_out, out_stride, npix, out_bpp - bpp, nframes, stream);
    }
    const uint32_t groups = npix / 16;
    auto kern = bpp == 14 ? k_mlv_unpack_shift_x16<14> : (bpp == 12 ? k_mlv_unpack_shift_x16<12> : k_mlv_unpack_shift_x16<10>);
    hipLaunchKernelGGL(kern, dim3(grid_x(groups, 8192), nframes), dim3(256), 0, stream, (const uint8_t *)d_packed, packed_stride, (uint8_t *)d_out,
                       out_stride, (const uint4 *)dark, groups, dark ? cal->black_d : 0, out_bpp - bpp);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// (see preload_k_unpack: the transcoder asks before its first batch, so that the first batch's timing is the others')
void preload_k_mlvpack() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)k_mlv_tile_x<16, false>); (void)hipGetLastError(); }

}  // namespace mlv

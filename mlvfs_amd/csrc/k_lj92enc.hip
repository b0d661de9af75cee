// k_lj92enc.hip -- the lossless-JPEG ENCODER of the reference's lj92.o (lj92.h:65-68, lj92.c:711-1144) on the GPU, for batches of
// frames that lie in HBM (the mount's lossless .dng files, csrc/mount.cpp) and, as a batch of one, for the lj92_encode drop-in.
//
// The reference encodes sequentially: one scan for the SSSS histogram (lj92.c:733-786), a Huffman table from it (lj92.c:788-937,
// host: lj92enc.cpp), a second scan that writes code + value bits and stuffs a zero behind every 0xFF byte (lj92.c:986-1099).
// Predictor 6 needs only the ORIGINAL neighbours (the encoder predicts from the pixels themselves, not from a recurrence), so
// every pixel is independent and its class and value bits are recomputed from the pixels wherever they are needed -- no plane of
// code words goes through HBM.  Every kernel takes its frame from blockIdx.y (the scans: blockIdx.x):
//
//   k_lje_hist     a workgroup's 4096 pixels -> their class counts (LDS) -> the frame's histogram and the block's 17 counts
//   -- host: the batch's tables, marker segments and bit-buffer offsets (lj92enc.cpp), one download and one upload --
//   k_lje_scan_bits  block bit lengths = counts x (code length + class), exclusive scan; zeroes the dwords two blocks share
//   k_lje_emit     a thread packs its 16 pixels into a 64-bit window, the workgroup's bits are assembled in LDS and stored as
//                  whole dwords (only the first and last one can be shared with a neighbour: atomicOr); 0xFF bytes counted there
//   k_lje_scan_ff  adds the bytes that straddle two blocks, exclusive scan; stream length, marker segments, EOI
//   k_lje_stuff    a block's bytes to their final places, a zero behind each 0xFF (lj92.c:1046-1048, 1063-1065, 1085-1088),
//                  assembled in LDS and stored as whole dwords
#include "k_bits_dev.h"

namespace mlv {

// pixel i of the tile (lj92.c:748-776: target coordinates row = i / width, col = i % width; the tile is contiguous)
template <bool DELIN>
__device__ __forceinline__ int lje_value(const uint16_t *__restrict__ img, const uint16_t *__restrict__ delin, int delin_len, uint32_t i, int *bad)
{
    int p = img[i];
    if (DELIN) {
        if (p >= delin_len) { *bad = 1; return 0; }     // the reference reads behind its table here
        p = delin[p];
    }
    return p;
}

__device__ __forceinline__ void lje_unpack8(const uint4 v, int *o)
{
    o[0] = v.x & 0xFFFF; o[1] = v.x >> 16; o[2] = v.y & 0xFFFF; o[3] = v.y >> 16;
    o[4] = v.z & 0xFFFF; o[5] = v.z >> 16; o[6] = v.w & 0xFFFF; o[7] = v.w >> 16;
}

// pixels i0 .. i0 + cnt - 1 (cnt <= 16) -> code[k] = SSSS << 24 | value bits (17 at most)
template <bool DELIN>
__device__ __forceinline__ void lje_codes(const uint16_t *__restrict__ img, const uint16_t *__restrict__ delin, int delin_len, int width,
                                          int bitdepth, uint32_t i0, int cnt, uint32_t *code, int *bad)
{
    if (cnt <= 0) return;
    uint32_t row = i0 / (uint32_t)width, col = i0 - row * (uint32_t)width;
    int cur[LJE_PER_THREAD], up[LJE_PER_THREAD];
    const bool full = cnt == LJE_PER_THREAD;
    if (!DELIN && full && (((uintptr_t)(img + i0)) & 15) == 0) {
        lje_unpack8(*(const uint4 *)(img + i0), cur);
        lje_unpack8(*(const uint4 *)(img + i0 + 8), cur + 8);
    } else {
#pragma unroll
        for (int k = 0; k < LJE_PER_THREAD; k++) cur[k] = k < cnt ? lje_value<DELIN>(img, delin, delin_len, i0 + k, bad) : 0;
    }
    if (!DELIN && full && row >= 1 && (((uintptr_t)(img + i0 - width)) & 15) == 0) {
        lje_unpack8(*(const uint4 *)(img + i0 - width), up);
        lje_unpack8(*(const uint4 *)(img + i0 - width + 8), up + 8);
    } else {
#pragma unroll
        for (int k = 0; k < LJE_PER_THREAD; k++) up[k] = (k < cnt && i0 + k >= (uint32_t)width) ? lje_value<DELIN>(img, delin, delin_len, i0 + k - width, bad) : 0;
    }
    int a = i0 ? lje_value<DELIN>(img, delin, delin_len, i0 - 1, bad) : 0;
    int c = (row >= 1 && col >= 1) ? lje_value<DELIN>(img, delin, delin_len, i0 - width - 1, bad) : 0;
#pragma unroll
    for (int k = 0; k < LJE_PER_THREAD; k++) {
        if (k < cnt) {
            const int p = cur[k], b = up[k];
            int px;
            if (row == 0 && col == 0) px = 1 << (bitdepth - 1);
            else if (row == 0) px = a;
            else if (col == 0) px = b;
            else px = b + ((a - c) >> 1);
            int d = p - px;
            const int ssss = d ? 32 - __clz(abs(d)) : 0;
            if (ssss > 0 && d < (1 << (ssss - 1))) d += (1 << ssss) - 1;         // negative differences: one's complement, lj92.c:1030-1035
            code[k] = ((uint32_t)ssss << 24) | ((uint32_t)d & 0x1FFFFu);
            a = p;
            c = b;
            if (++col == (uint32_t)width) { col = 0; row++; }
        }
    }
}

template <bool DELIN>
__global__ __launch_bounds__(256) void k_lje_hist(const uint16_t *const *__restrict__ src, const uint16_t *__restrict__ delin, int delin_len,
                                                  int width, uint32_t npix, int bitdepth, uint32_t *__restrict__ hist,
                                                  uint32_t *__restrict__ blockhist)
{
    __shared__ uint32_t h[LJE_HIST];
    if (threadIdx.x < LJE_HIST) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t f = blockIdx.y;
    const uint16_t *img = src[f];
    const uint32_t i0 = blockIdx.x * (uint32_t)LJE_BLOCK + threadIdx.x * LJE_PER_THREAD;
    const int cnt = i0 < npix ? (int)min((uint32_t)LJE_PER_THREAD, npix - i0) : 0;
    uint32_t code[LJE_PER_THREAD];
    int bad = 0;
    lje_codes<DELIN>(img, delin, delin_len, width, bitdepth, i0, cnt, code, &bad);
#pragma unroll
    for (int k = 0; k < LJE_PER_THREAD; k++)
        if (k < cnt) atomicAdd(&h[min(code[k] >> 24, 17u)], 1u);
    if (bad) h[18] = 1;
    __syncthreads();
    if (threadIdx.x < 17) blockhist[((size_t)f * gridDim.x + blockIdx.x) * 17 + threadIdx.x] = h[threadIdx.x];
    if (threadIdx.x < 19 && h[threadIdx.x]) atomicAdd(&hist[f * LJE_HIST + threadIdx.x], h[threadIdx.x]);
}

// off[0 .. nb]: where each block's bits begin, off[nb] = the frame's bits
__global__ __launch_bounds__(LJE_SCAN_THREADS) void k_lje_scan_bits(const LjeFrame *__restrict__ tabs, const uint32_t *__restrict__ blockhist, uint32_t nb,
                                                        uint32_t *__restrict__ off, uint32_t *__restrict__ bits, LjeOut *__restrict__ res)
{
    __shared__ uint32_t ws[16], cost[17];
    const uint32_t f = blockIdx.x;
    const LjeFrame &t = tabs[f];
    if (t.status != LJE_OK) return;
    if (threadIdx.x < 17) cost[threadIdx.x] = t.len[threadIdx.x] + threadIdx.x;
    __syncthreads();
    const uint32_t per = lje_scan_per(nb), b0 = min(nb, threadIdx.x * per), b1 = min(nb, b0 + per);
    uint32_t *o = off + (size_t)f * (nb + 1);
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t *bh = blockhist + ((size_t)f * nb + b) * 17;
        uint32_t v = 0;
        for (int s = 0; s < 17; s++) v += bh[s] * cost[s];
        o[b] = v;
        sum += v;
    }
    uint32_t total;
    uint32_t run = lje_scan1024(sum, ws, &total);
    uint32_t *fb = bits + t.bits_at;
    for (uint32_t b = b0; b < b1; b++) { const uint32_t v = o[b]; o[b] = run; fb[run >> 5] = 0; run += v; }
    if (threadIdx.x == 0) { o[nb] = total; fb[total >> 5] = 0; res[f].bits = total; }
}

template <bool DELIN>
__global__ __launch_bounds__(256) void k_lje_emit(const uint16_t *const *__restrict__ src, const uint16_t *__restrict__ delin, int delin_len,
                                                  int width, uint32_t npix, int bitdepth, const LjeFrame *__restrict__ tabs,
                                                  const uint32_t *__restrict__ off, uint32_t *__restrict__ bits, uint32_t *__restrict__ blockff)
{
    __shared__ uint32_t lds[LJE_BLOCK + 4];              // 32 bits per pixel at most, and the bits before the first in its dword
    __shared__ uint32_t wave_sum[4], ffs;
    __shared__ uint8_t tl[17];
    __shared__ uint16_t tc[17];
    const uint32_t f = blockIdx.y, nb = gridDim.x;
    const LjeFrame &t = tabs[f];
    if (t.status != LJE_OK) return;
    for (int j = threadIdx.x; j < LJE_BLOCK + 4; j += 256) lds[j] = 0;
    if (threadIdx.x < 17) { tl[threadIdx.x] = t.len[threadIdx.x]; tc[threadIdx.x] = t.code[threadIdx.x]; }
    if (threadIdx.x == 0) ffs = 0;
    const uint32_t i0 = blockIdx.x * (uint32_t)LJE_BLOCK + threadIdx.x * LJE_PER_THREAD;
    const int cnt = i0 < npix ? (int)min((uint32_t)LJE_PER_THREAD, npix - i0) : 0;
    uint32_t code[LJE_PER_THREAD];
    int bad = 0;
    lje_codes<DELIN>(src[f], delin, delin_len, width, bitdepth, i0, cnt, code, &bad);
    __syncthreads();
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < LJE_PER_THREAD; k++)
        if (k < cnt) { const uint32_t s = min(code[k] >> 24, 16u); n += tl[s] + s; }
    // exclusive scan over the workgroup's 256 threads
    uint32_t inc = n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    const uint32_t begin = off[(size_t)f * (nb + 1) + blockIdx.x], end = off[(size_t)f * (nb + 1) + blockIdx.x + 1];
    uint32_t at = (begin & 31) + inc - n;
    for (int k = 0; k < wave; k++) at += wave_sum[k];
    // a 64-bit window whose top bit is bit (at & ~31) of the workgroup's dwords
    uint32_t word = at >> 5;
    int fill = at & 31;                                  // bits of the window in use
    uint64_t win = 0;
#pragma unroll
    for (int k = 0; k < LJE_PER_THREAD; k++) {
        if (k < cnt) {
            const uint32_t c = code[k], s = min(c >> 24, 16u);
            const int hl = tl[s];
            // code then value: hl + s <= 32 bits, appended in two steps so that neither shift reaches 64
            if (hl) { win |= (uint64_t)tc[s] << (64 - fill - hl); fill += hl; }
            if (fill >= 32) { atomicOr(&lds[word++], (uint32_t)(win >> 32)); win <<= 32; fill -= 32; }
            if (s) { win |= (uint64_t)(c & ((1u << s) - 1u)) << (64 - fill - (int)s); fill += (int)s; }
            if (fill >= 32) { atomicOr(&lds[word++], (uint32_t)(win >> 32)); win <<= 32; fill -= 32; }
        }
    }
    if (fill) atomicOr(&lds[word], (uint32_t)(win >> 32));
    __syncthreads();
    // the workgroup's dwords: whole ones stored, the two it may share with its neighbours ORed into zeroed memory
    const uint32_t lead = begin & 31, ndw = (lead + (end - begin) + 31) >> 5, w0 = begin >> 5;
    uint32_t *g = bits + t.bits_at + w0;
    uint32_t ff = 0;
    for (uint32_t j = threadIdx.x; j < ndw; j += 256) {
        const uint32_t v = lds[j];
        if ((j == 0 && lead) || (j == ndw - 1 && (end & 31))) atomicOr(&g[j], v);
        else g[j] = v;
        // 0xFF bytes that lie wholly inside the block (a byte two blocks share is counted by k_lje_scan_ff)
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t bit = ((w0 + j) << 5) + 8 * q;
            if (bit >= begin && bit + 8 <= end && ((v >> (24 - 8 * q)) & 0xFFu) == 0xFFu) ff++;
        }
    }
    for (int o = 32; o; o >>= 1) ff += __shfl_down(ff, o);
    if (lane == 0 && ff) atomicAdd(&ffs, ff);
    __syncthreads();
    if (threadIdx.x == 0) blockff[(size_t)f * (nb + 1) + blockIdx.x] = ffs;
}

// ffoff[b]: 0xFF bytes before block b's bytes -- a block's bytes are those whose first bit is its own
__global__ __launch_bounds__(LJE_SCAN_THREADS) void k_lje_scan_ff(const LjeFrame *__restrict__ tabs, const uint32_t *__restrict__ off, uint32_t nb,
                                                      uint32_t *__restrict__ ffoff, const uint32_t *__restrict__ bits, uint8_t *__restrict__ out,
                                                      size_t out_stride, LjeOut *__restrict__ res)
{
    __shared__ uint32_t ws[16];
    const uint32_t f = blockIdx.x;
    const LjeFrame &t = tabs[f];
    if (t.status != LJE_OK) return;
    const uint32_t per = lje_scan_per(nb), b0 = min(nb, threadIdx.x * per), b1 = min(nb, b0 + per);
    const uint32_t *o = off + (size_t)f * (nb + 1);
    uint32_t *fo = ffoff + (size_t)f * (nb + 1);
    const uint32_t *fb = bits + t.bits_at;
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; b++) {
        uint32_t v = fo[b];
        const uint32_t e = o[b + 1];
        if ((e & 7) && (e & ~7u) >= o[b] && lje_byte(fb, e >> 3) == 0xFFu) v++;                 // the byte this block begins and the next one ends
        fo[b] = v;
        sum += v;
    }
    uint32_t total;
    uint32_t run = lje_scan1024(sum, ws, &total);
    for (uint32_t b = b0; b < b1; b++) { const uint32_t v = fo[b]; fo[b] = run; run += v; }
    const uint32_t nbytes = (o[nb] + 7) >> 3, hl = t.head_len;
    const uint64_t length = (uint64_t)hl + nbytes + total + 2;
    const bool fits = length <= out_stride;
    uint8_t *e = out + (size_t)f * out_stride;
    if (fits) {
        if (threadIdx.x < hl) e[threadIdx.x] = t.head[threadIdx.x];
        if (threadIdx.x == 64) e[length - 2] = 0xFF;
        if (threadIdx.x == 65) e[length - 1] = 0xD9;
    }
    if (threadIdx.x == 0) {
        res[f].length = fits ? (uint32_t)length : 0;
        res[f].status = fits ? LJE_OK : LJE_NOFIT;
        res[f].stuffed = total;
    }
}

__global__ __launch_bounds__(256) void k_lje_stuff(const LjeFrame *__restrict__ tabs, const uint32_t *__restrict__ off, const uint32_t *__restrict__ ffoff,
                                                   const uint32_t *__restrict__ bits, uint8_t *__restrict__ out, size_t out_stride,
                                                   const LjeOut *__restrict__ res)
{
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t ldw[2 * LJE_BLOCK / 4 + 2];      // a chunk's stuffed bytes behind the up to three bytes before them in their dword
    const uint32_t f = blockIdx.y, nb = gridDim.x;
    const LjeFrame &t = tabs[f];
    if (t.status != LJE_OK || res[f].status != LJE_OK) return;
    const uint32_t *fb = bits + t.bits_at;
    uint8_t *e = out + (size_t)f * out_stride;           // 4-byte aligned (checked by the host)
    const uint32_t begin = off[(size_t)f * (nb + 1) + blockIdx.x], end = off[(size_t)f * (nb + 1) + blockIdx.x + 1];
    const uint32_t B0 = (begin + 7) >> 3, B1 = (end + 7) >> 3;
    const uint32_t P = t.head_len + B0 + ffoff[(size_t)f * (nb + 1) + blockIdx.x];      // where byte B0 goes
    lje_stuff_span(fb, e, B0, B1, P, ldw, wave_sum);
}

int lje_launch_hist(const uint16_t *const *d_src, const uint16_t *d_delin, int delin_len, int width, uint32_t npix, int bitdepth, int n,
                    uint32_t *d_hist, uint32_t *d_blockhist, hipStream_t s)
{
    const dim3 grid(lje_blocks(npix), n);
    if (d_delin) hipLaunchKernelGGL(k_lje_hist<true>, grid, dim3(256), 0, s, d_src, d_delin, delin_len, width, npix, bitdepth, d_hist, d_blockhist);
    else hipLaunchKernelGGL(k_lje_hist<false>, grid, dim3(256), 0, s, d_src, d_delin, delin_len, width, npix, bitdepth, d_hist, d_blockhist);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

int lje_launch_pack(const uint16_t *const *d_src, const uint16_t *d_delin, int delin_len, int width, uint32_t npix, int bitdepth, int n,
                    const LjeFrame *d_tabs, const uint32_t *d_blockhist, uint32_t *d_off, uint32_t *d_ffoff, uint32_t *d_bits, uint8_t *d_out,
                    size_t out_stride, LjeOut *d_res, hipStream_t s)
{
    const uint32_t nb = lje_blocks(npix);
    const dim3 grid(nb, n);
    hipLaunchKernelGGL(k_lje_scan_bits, dim3(n), dim3(LJE_SCAN_THREADS), 0, s, d_tabs, d_blockhist, nb, d_off, d_bits, d_res);
    if (d_delin) hipLaunchKernelGGL(k_lje_emit<true>, grid, dim3(256), 0, s, d_src, d_delin, delin_len, width, npix, bitdepth, d_tabs, (const uint32_t *)d_off, d_bits, d_ffoff);
    else hipLaunchKernelGGL(k_lje_emit<false>, grid, dim3(256), 0, s, d_src, d_delin, delin_len, width, npix, bitdepth, d_tabs, (const uint32_t *)d_off, d_bits, d_ffoff);
    hipLaunchKernelGGL(k_lje_scan_ff, dim3(n), dim3(LJE_SCAN_THREADS), 0, s, d_tabs, (const uint32_t *)d_off, nb, d_ffoff, (const uint32_t *)d_bits, d_out, out_stride, d_res);
    hipLaunchKernelGGL(k_lje_stuff, grid, dim3(256), 0, s, d_tabs, (const uint32_t *)d_off, (const uint32_t *)d_ffoff, (const uint32_t *)d_bits, d_out, out_stride, (const LjeOut *)d_res);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

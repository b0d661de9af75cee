// k_bits_dev.h -- what the two entropy coders (k_lj92enc.hip: lossless JPEG of the served frames; k_jpeg.hip: baseline JPEG of the
// renderings) share on the device: the scan over a frame's blocks or rows, a byte of an MSB-first bit stream, and the pass that moves
// a span of stream bytes to its final place with a zero behind every 0xFF.
#pragma once
#include "lj92enc.h"

namespace mlv {

// exclusive scan over the 1024 threads of a workgroup; *total = the sum
static_assert(LJE_SCAN_THREADS == 16 * 64, "lje_scan1024 scans 16 waves of 64");
__device__ __forceinline__ uint32_t lje_scan1024(uint32_t x, uint32_t *ws /* [16], shared */, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = x;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    __syncthreads();                                     // ws may still be read from the scan before
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int k = 0; k < 16; k++) { const uint32_t u = ws[k]; if (k < wave) base += u; tot += u; }
    *total = tot;
    return base + inc - x;
}

// stream byte b of a frame's unstuffed bits (MSB first: bit k of the stream is bit 31 - k % 32 of dword k / 32)
__device__ __forceinline__ uint32_t lje_byte(const uint32_t *__restrict__ bits, uint32_t b) { return (bits[b >> 2] >> (24 - 8 * (b & 3))) & 0xFFu; }

// Bytes B0 .. B1 - 1 of the unstuffed stream fb go to e + P and behind, a zero behind each 0xFF (lj92.c:1046-1048, 1063-1065,
// 1085-1088; JPEG B.1.1.5), by the 256 threads of a workgroup in chunks of LJE_BLOCK bytes: assembled in LDS and stored as whole
// dwords.  e is 4-byte aligned; ldw: 2 * LJE_BLOCK / 4 + 2 dwords, wave_sum: 4, both shared.  Returns where the next byte would go.
__device__ __forceinline__ uint32_t lje_stuff_span(const uint32_t *__restrict__ fb, uint8_t *__restrict__ e, uint32_t B0, uint32_t B1, uint32_t P,
                                                   uint32_t *ldw, uint32_t *wave_sum)
{
    uint8_t *ldb = (uint8_t *)ldw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t Bc = B0; Bc < B1; Bc += LJE_BLOCK) {
        const uint32_t i0 = Bc + threadIdx.x * LJE_PER_THREAD;
        const int cnt = i0 < B1 ? (int)min((uint32_t)LJE_PER_THREAD, B1 - i0) : 0;
        uint32_t a[4] = { 0, 0, 0, 0 };                  // the thread's 16 bytes, first byte on top
        if (cnt) {
            uint32_t w[5];
            const uint32_t last = (B1 - 1) >> 2;
            for (int q = 0; q < 5; q++) w[q] = fb[min((i0 >> 2) + q, last)];
            const int sh = 8 * (i0 & 3);
            for (int q = 0; q < 4; q++) a[q] = sh ? (w[q] << sh) | (w[q + 1] >> (32 - sh)) : w[q];
        }
        uint32_t n = 0;
#pragma unroll
        for (int k = 0; k < LJE_PER_THREAD; k++)
            if (k < cnt) n += ((a[k >> 2] >> (24 - 8 * (k & 3))) & 0xFFu) == 0xFFu;
        uint32_t inc = n;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= o) inc += u; }
        __syncthreads();                                 // the chunk before has left LDS
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        uint32_t before = inc - n, chunk_ff = 0;
        for (int k = 0; k < 4; k++) { const uint32_t u = wave_sum[k]; if (k < wave) before += u; chunk_ff += u; }
        const uint32_t lead = P & 3, chunk_len = min((uint32_t)LJE_BLOCK, B1 - Bc) + chunk_ff;
        uint32_t lp = lead + threadIdx.x * LJE_PER_THREAD + before;
#pragma unroll
        for (int k = 0; k < LJE_PER_THREAD; k++)
            if (k < cnt) {
                const uint8_t v = (uint8_t)(a[k >> 2] >> (24 - 8 * (k & 3)));
                ldb[lp++] = v;
                if (v == 0xFF) ldb[lp++] = 0;
            }
        __syncthreads();
        uint8_t *g = e + (P - lead);
        const uint32_t span = (lead + chunk_len + 3) >> 2;
        for (uint32_t j = threadIdx.x; j < span; j += 256) {
            if (4 * j >= lead && 4 * j + 4 <= lead + chunk_len) ((uint32_t *)g)[j] = ldw[j];
            else
                for (uint32_t q = 4 * j; q < 4 * j + 4; q++)
                    if (q >= lead && q < lead + chunk_len) g[q] = ldb[q];
        }
        P += chunk_len;
    }
    return P;
}

}  // namespace mlv

// k_jpeg.hip -- the renderings (k_render.hip) as baseline JPEG streams: include/mlvfs_amd.h, "rendered frames as baseline JPEG files";
// DESIGN.md 3.13; the definition in numpy: mlvfs_amd/jpeg.py.  4:2:0, MCUs of 16 x 16 pixels, the Annex K Huffman tables, one restart
// interval per MCU row -- so MCU rows are independent and byte-aligned, and only byte offsets are scanned across rows.
// Every kernel takes its frame from blockIdx.y (the two scans across rows: blockIdx.x):
//
//   k_jpg_transform   4 MCUs side by side per workgroup: RGB (whole dwords) -> YCbCr -> 4:2:0 (LDS) -> 8 x 8 DCT, rows then columns with
//                     the transposition in LDS (rows of 9 dwords) -> quantised (one multiply by a reciprocal) -> scan order; the int16
//                     coefficients go to HBM, with each block's DC value and the bits of its AC symbols (a wave = a block's 64
//                     coefficients: runs from one ballot)
//   k_jpg_scan_bits   bits per MCU (AC bits + DC differences along the row), exclusive scan inside each MCU row
//   k_jpg_rows        row lengths -> where each row begins in the row buffer; zeroes the dwords two workgroups of a row share
//   k_jpg_emit        16 MCUs per workgroup: a wave packs a block -- every lane its coefficient's ZRLs, code and value bits, up to 59
//                     bits, placed by a wave scan -- into LDS, stored as whole dwords (only the first one can be shared with the
//                     workgroup before: atomicOr); the row's last workgroup pads with 1-bits
//   k_jpg_count_ff    0xFF bytes per padded row
//   k_jpg_place       bytes + stuffing + 2 per row, exclusive scan across the frame; the stream's length, and whether it fits
//   k_jpg_stuff       each row to its final place with a zero behind each 0xFF (lje_stuff_span, shared with k_lj92enc.hip), then its
//                     RST marker or, after the last row, EOI
// Coefficients go through HBM (1.5 x 256 int16 per MCU, written once, read once by k_jpg_emit): recomputing them in the emit pass
// would run the transform twice to save 1.5 bytes per pixel each way of a stage that is far from the machine's bandwidth.
//
// The chroma sampling is a constant S of the three kernels that see blocks (k_jpg_transform, k_jpg_scan_bits,
// k_jpg_emit), S indexing kJpgModes (jpeg.h): 4:2:0 as above; 4:2:2, MCUs of 16 x 8 pixels and 4 blocks; 4:4:4, MCUs of 8 x 8 pixels
// and 3 blocks.  Their text (k_jpeg_blocks.inc) is compiled once per sampling: k_jpg_transform (4:2:0, the kernel as it was),
// k_jpg_transform_422, k_jpg_transform_444, and so on.  At the two new samplings a workgroup of k_jpg_transform_* takes a tile of
// 64 x 8 pixels (16 or 24 blocks), one of k_jpg_emit_* 96 blocks as at 4:2:0.  The other four kernels see MCU rows only and take
// everything from the layout; k_jpg_rows is told how many MCUs a workgroup of the emit kernel takes.
#include "jpeg.h"
#include "k_bits_dev.h"

namespace mlv {

namespace {

// natural index -> position in scan order
__device__ const uint8_t kIzig[64] = { 0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
                                       10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63 };

// sum_x T[u][x] * s[x] for the eight u, T the integer DCT matrix of the definition: T[u][7 - x] = (-1)^u T[u][x], so the even rows
// take the sums and the odd rows the differences of mirrored samples -- the same integers as the 64 products, in 32 bits
__device__ __forceinline__ void jpg_dct8(const int *s, int *o)
{
    const int e0 = s[0] + s[7], e1 = s[1] + s[6], e2 = s[2] + s[5], e3 = s[3] + s[4];
    const int d0 = s[0] - s[7], d1 = s[1] - s[6], d2 = s[2] - s[5], d3 = s[3] - s[4];
    o[0] = 2896 * (e0 + e1 + e2 + e3);
    o[4] = 2896 * (e0 - e1 - e2 + e3);
    o[2] = 3784 * (e0 - e3) + 1567 * (e1 - e2);
    o[6] = 1567 * (e0 - e3) - 3784 * (e1 - e2);
    o[1] = 4017 * d0 + 3406 * d1 + 2276 * d2 + 799 * d3;
    o[3] = 3406 * d0 - 799 * d1 - 4017 * d2 - 2276 * d3;
    o[5] = 2276 * d0 - 4017 * d1 + 799 * d2 + 3406 * d3;
    o[7] = 799 * d0 - 2276 * d1 + 3406 * d2 - 4017 * d3;
}

// one pixel, R G B in bits 0 .. 23 -> Y, Cb, Cr
__device__ __forceinline__ void jpg_ycc(uint32_t p, uint32_t *y, uint32_t *cb, uint32_t *cr)
{
    const int r = p & 0xFF, g = (p >> 8) & 0xFF, b = (p >> 16) & 0xFF;
    *y = (uint32_t)((19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
    *cb = (uint32_t)min(max(((-11058 * r - 21710 * g + 32768 * b + 32768) >> 16) + 128, 0), 255);
    *cr = (uint32_t)min(max(((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128, 0), 255);
}

__device__ __forceinline__ int jpg_category(int v) { return v ? 32 - __clz(abs(v)) : 0; }

// exclusive scan over the 256 threads of a workgroup; *total = the sum
__device__ __forceinline__ uint32_t jpg_scan256(uint32_t x, uint32_t *ws /* [4], shared */, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = x;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    __syncthreads();                                     // ws may still be read from the scan before
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (int k = 0; k < 4; k++) { const uint32_t u = ws[k]; if (k < wave) base += u; tot += u; }
    *total = tot;
    return base + inc - x;
}

// the DC value block bj of MCU m (mx-th of its row) is predicted from: the block of the same component before it in the row
template <int S> __device__ __forceinline__ int jpg_pred(const int16_t *__restrict__ dcv, uint32_t m, uint32_t mx, int bj)
{
    constexpr int NB = kJpgModes[S].nb, NY = kJpgModes[S].ny;
    if (bj >= 1 && bj <= NY - 1) return dcv[(size_t)m * NB + bj - 1];
    if (mx == 0) return 0;
    return dcv[(size_t)(m - 1) * NB + (bj == 0 ? NY - 1 : bj)];
}

struct JpgFrame {
    int16_t *coef, *dcv;
    uint16_t *bbits;
    uint32_t *off, *rowbits, *rowat, *rowff, *rowdst, *rowbuf;
    __device__ JpgFrame(const JpgLayout &l, uint8_t *scratch, uint32_t nframes, uint32_t f)
    {
        uint8_t *b = scratch + ((sizeof(JpgOut) * (size_t)nframes + 255) / 256 * 256) + l.frame_bytes * f;
        coef = (int16_t *)(b + l.coef);
        dcv = (int16_t *)(b + l.dcv);
        bbits = (uint16_t *)(b + l.bbits);
        off = (uint32_t *)(b + l.off);
        rowbits = (uint32_t *)(b + l.rowbits);
        rowat = (uint32_t *)(b + l.rowat);
        rowff = (uint32_t *)(b + l.rowff);
        rowdst = (uint32_t *)(b + l.rowdst);
        rowbuf = (uint32_t *)(b + l.rowbuf);
    }
};

__device__ __forceinline__ uint32_t jpg_row_dwords(uint32_t bits) { return (((bits + 7) >> 3) + 3) >> 2; }

}  // namespace

// `len` bits (1 .. 64) of v, the first one at bit `pos` of the MSB-first stream in LDS
__device__ __forceinline__ void jpg_put(uint32_t *lds, uint32_t pos, uint64_t v, uint32_t len)
{
    const uint64_t x = v << (64 - len);
    const uint32_t i = pos >> 5, s = pos & 31;
    const uint32_t p0 = (uint32_t)(x >> (32 + s)), p1 = (uint32_t)(x >> s), p2 = s ? (uint32_t)x << (32 - s) : 0u;
    if (p0) atomicOr(&lds[i], p0);
    if (p1) atomicOr(&lds[i + 1], p1);
    if (p2) atomicOr(&lds[i + 2], p2);
}

// grid.x = frames; chunk: the MCUs a workgroup of the sampling's emit kernel takes, nch = ceil(mw / chunk) of them a row
__global__ __launch_bounds__(LJE_SCAN_THREADS) void k_jpg_rows(const JpgLayout l, uint8_t *__restrict__ scratch, uint32_t nframes, uint32_t chunk, uint32_t nch)
{
    __shared__ uint32_t ws[16];
    const uint32_t f = blockIdx.x;
    const JpgFrame fr(l, scratch, nframes, f);
    JpgOut *res = (JpgOut *)scratch + f;
    const uint32_t per = lje_scan_per(l.mh), r0 = min(l.mh, threadIdx.x * per), r1 = min(l.mh, r0 + per);
    uint32_t sum = 0;
    for (uint32_t r = r0; r < r1; r++) sum += jpg_row_dwords(fr.rowbits[r]);
    uint32_t total;
    uint32_t run = lje_scan1024(sum, ws, &total);
    for (uint32_t r = r0; r < r1; r++) { fr.rowat[r] = run; run += jpg_row_dwords(fr.rowbits[r]); }
    const bool fits = total <= l.rowcap_dw;
    if (threadIdx.x == 0) { res->length = 0; res->status = fits ? 0 : 1; }
    if (!fits) return;
    __syncthreads();
    // the dword in which a workgroup of k_jpg_emit begins is the one the workgroup before it ends in
    for (uint32_t k = threadIdx.x; k < l.mh * nch; k += LJE_SCAN_THREADS) {
        const uint32_t r = k / nch, ch = k - r * nch;
        if (ch) fr.rowbuf[fr.rowat[r] + (fr.off[r * l.mw + ch * chunk] >> 5)] = 0;
    }
}

// the three kernels that see blocks, once per sampling
#define JPG_S MLVFS_AMD_JPEG_420
#define JPG_K(name) name
#include "k_jpeg_blocks.inc"
#undef JPG_S
#undef JPG_K
#define JPG_S MLVFS_AMD_JPEG_422
#define JPG_K(name) name##_422
#include "k_jpeg_blocks.inc"
#undef JPG_S
#undef JPG_K
#define JPG_S MLVFS_AMD_JPEG_444
#define JPG_K(name) name##_444
#include "k_jpeg_blocks.inc"
#undef JPG_S
#undef JPG_K

// grid.x = mh
__global__ __launch_bounds__(256) void k_jpg_count_ff(const JpgLayout l, uint8_t *__restrict__ scratch)
{
    __shared__ uint32_t count;
    const uint32_t t = threadIdx.x, f = blockIdx.y, r = blockIdx.x;
    if (((const JpgOut *)scratch)[f].status) return;
    const JpgFrame fr(l, scratch, gridDim.y, f);
    if (t == 0) count = 0;
    __syncthreads();
    const uint32_t nbytes = (fr.rowbits[r] + 7) >> 3;
    const uint32_t *row = fr.rowbuf + fr.rowat[r];
    uint32_t n = 0;
    for (uint32_t k = t; 4 * k < nbytes; k += 256) {
        const uint32_t w = row[k];
        for (uint32_t q = 0; q < 4; q++)
            if (4 * k + q < nbytes && ((w >> (24 - 8 * q)) & 0xFFu) == 0xFFu) n++;
    }
    for (int o = 32; o; o >>= 1) n += __shfl_down(n, o);
    if ((t & 63) == 0 && n) atomicAdd(&count, n);
    __syncthreads();
    if (t == 0) fr.rowff[r] = count;
}

// grid.x = frames
__global__ __launch_bounds__(LJE_SCAN_THREADS) void k_jpg_place(const JpgLayout l, uint8_t *__restrict__ scratch, uint32_t nframes, uint32_t room)
{
    __shared__ uint32_t ws[16];
    const uint32_t f = blockIdx.x;
    JpgOut *res = (JpgOut *)scratch + f;
    if (res->status) return;
    const JpgFrame fr(l, scratch, nframes, f);
    const uint32_t per = lje_scan_per(l.mh), r0 = min(l.mh, threadIdx.x * per), r1 = min(l.mh, r0 + per);
    uint32_t sum = 0;
    for (uint32_t r = r0; r < r1; r++) sum += ((fr.rowbits[r] + 7) >> 3) + fr.rowff[r] + 2;
    uint32_t total;
    uint32_t run = lje_scan1024(sum, ws, &total);
    for (uint32_t r = r0; r < r1; r++) { fr.rowdst[r] = run; run += ((fr.rowbits[r] + 7) >> 3) + fr.rowff[r] + 2; }
    if (threadIdx.x == 0) { res->length = total; res->status = total > room ? 1 : 0; }
}

// grid.x = mh
__global__ __launch_bounds__(256) void k_jpg_stuff(const JpgLayout l, uint8_t *__restrict__ scratch, uint8_t *__restrict__ out, size_t out_stride)
{
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t ldw[2 * LJE_BLOCK / 4 + 2];
    const uint32_t f = blockIdx.y, r = blockIdx.x;
    if (((const JpgOut *)scratch)[f].status) return;
    const JpgFrame fr(l, scratch, gridDim.y, f);
    uint8_t *e = out + (size_t)f * out_stride;
    const uint32_t mis = (uint32_t)((uintptr_t)e & 3);   // the stream may begin anywhere: the dwords are those of the memory
    e -= mis;
    const uint32_t end = lje_stuff_span(fr.rowbuf + fr.rowat[r], e, 0, (fr.rowbits[r] + 7) >> 3, mis + fr.rowdst[r], ldw, wave_sum);
    if (threadIdx.x == 0) {
        e[end] = 0xFF;
        e[end + 1] = r + 1 == l.mh ? 0xD9 : (uint8_t)(0xD0 + (r & 7));
    }
}

// l: jpg_layout() of `sampling`
int jpg_launch(const uint8_t *d_rgb, size_t stride, const JpgLayout &l, const JpgQuant &q, const JpgHuff &h, uint8_t *d_out, size_t out_stride,
               uint32_t room, uint8_t *d_scratch, int nframes, hipStream_t s, int sampling)
{
    if (!jpg_sampling_ok(sampling)) { set_error("jpeg: a sampling of %d", sampling); return MLVFS_AMD_ERR_ARG; }
    if (nframes <= 0) return MLVFS_AMD_OK;
    const uint32_t n = (uint32_t)nframes;
    const uint32_t gx = (l.mw + kJpgModes[sampling].group - 1) / kJpgModes[sampling].group, nch = (l.mw + kJpgModes[sampling].chunk - 1) / kJpgModes[sampling].chunk;
    // the three kernels that see blocks, per sampling
    static constexpr decltype(&k_jpg_transform) transform[3] = { k_jpg_transform, k_jpg_transform_422, k_jpg_transform_444 };
    static constexpr decltype(&k_jpg_scan_bits) scan_bits[3] = { k_jpg_scan_bits, k_jpg_scan_bits_422, k_jpg_scan_bits_444 };
    static constexpr decltype(&k_jpg_emit) emit[3] = { k_jpg_emit, k_jpg_emit_422, k_jpg_emit_444 };
    hipLaunchKernelGGL(transform[sampling], dim3(gx * l.mh, n), dim3(256), 0, s, d_rgb, stride, l, q, h, d_scratch);
    hipLaunchKernelGGL(scan_bits[sampling], dim3(l.mh, n), dim3(256), 0, s, l, h, d_scratch);
    hipLaunchKernelGGL(k_jpg_rows, dim3(n), dim3(LJE_SCAN_THREADS), 0, s, l, d_scratch, n, (uint32_t)kJpgModes[sampling].chunk, nch);
    hipLaunchKernelGGL(emit[sampling], dim3(nch * l.mh, n), dim3(256), 0, s, l, h, d_scratch);
    hipLaunchKernelGGL(k_jpg_count_ff, dim3(l.mh, n), dim3(256), 0, s, l, d_scratch);
    hipLaunchKernelGGL(k_jpg_place, dim3(n), dim3(LJE_SCAN_THREADS), 0, s, l, d_scratch, n, room);
    hipLaunchKernelGGL(k_jpg_stuff, dim3(l.mh, n), dim3(256), 0, s, l, d_scratch, d_out, out_stride);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

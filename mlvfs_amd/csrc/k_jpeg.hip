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
__device__ __forceinline__ int jpg_pred(const int16_t *__restrict__ dcv, uint32_t m, uint32_t mx, int bj)
{
    if (bj >= 1 && bj <= 3) return dcv[(size_t)m * 6 + bj - 1];
    if (mx == 0) return 0;
    return dcv[(size_t)(m - 1) * 6 + (bj == 0 ? 3 : bj)];
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

// grid.x = ceil(mw / 4) * mh
__global__ __launch_bounds__(256) void k_jpg_transform(const uint8_t *__restrict__ rgb, size_t stride, const JpgLayout l, const JpgQuant qt, const JpgHuff hf,
                                                       uint8_t *__restrict__ scratch)
{
    __shared__ uint32_t ys[16][18];                      // a row: 64 samples in 16 dwords, 2 dwords of padding
    __shared__ uint32_t cbs[16][17], crs[16][17];        // a row: 32 sums of two neighbours, 16 bits each, 1 dword of padding
    __shared__ int ab[JPG_GROUP * 6][8][9];              // after the row pass; a row of 8 in 9 dwords: the column pass reads down
    __shared__ __attribute__((aligned(16))) int16_t zz[JPG_GROUP * 6][64];
    __shared__ uint32_t s_recip[128], sb[JPG_GROUP * 6];
    __shared__ uint8_t s_q[128], s_izig[64], s_aclen[512];
    const uint32_t t = threadIdx.x, f = blockIdx.y;
    const uint32_t gx = (l.mw + JPG_GROUP - 1) / JPG_GROUP, r = blockIdx.x / gx, g = blockIdx.x - r * gx;
    if (t < 128) { s_recip[t] = (&qt.recip[0][0])[t]; s_q[t] = (&qt.q[0][0])[t]; }
    if (t < 64) s_izig[t] = kIzig[t];
    s_aclen[t] = (&hf.ac_len[0][0])[t];
    s_aclen[t + 256] = (&hf.ac_len[0][0])[t + 256];
    // 1. colour: a thread takes 4 pixels of one of the 16 rows
    {
        const uint32_t y = t >> 4, xg = t & 15, X = 64 * g + 4 * xg, Y = min(16 * r + y, l.ph - 1);
        const uint8_t *row = rgb + (size_t)f * stride + (size_t)Y * l.pw * 3;
        uint32_t px[4];
        if (X + 3 < l.pw) {
            const uintptr_t p = (uintptr_t)(row + (size_t)X * 3);
            const uint32_t *a = (const uint32_t *)(p & ~(uintptr_t)3);
            const uint32_t sh = 8 * (uint32_t)(p & 3);
            uint32_t w0 = a[0], w1 = a[1], w2 = a[2];
            if (sh) {                                    // the twelve bytes lie in four dwords
                const uint32_t w3 = a[3];
                w0 = (w0 >> sh) | (w1 << (32 - sh));
                w1 = (w1 >> sh) | (w2 << (32 - sh));
                w2 = (w2 >> sh) | (w3 << (32 - sh));
            }
            px[0] = w0 & 0xFFFFFFu;
            px[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
            px[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
            px[3] = w2 >> 8;
        } else {                                         // the last column repeats
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint8_t *q = row + (size_t)min(X + k, l.pw - 1) * 3;
                px[k] = q[0] | (q[1] << 8) | (q[2] << 16);
            }
        }
        uint32_t yy[4], cb[4], cr[4];
#pragma unroll
        for (int k = 0; k < 4; k++) jpg_ycc(px[k], &yy[k], &cb[k], &cr[k]);
        ys[y][xg] = yy[0] | (yy[1] << 8) | (yy[2] << 16) | (yy[3] << 24);
        cbs[y][xg] = (cb[0] + cb[1]) | ((cb[2] + cb[3]) << 16);
        crs[y][xg] = (cr[0] + cr[1]) | ((cr[2] + cr[3]) << 16);
    }
    __syncthreads();
    // 2. rows: a thread takes one row of one of the 24 blocks
    if (t < JPG_GROUP * 48) {
        const uint32_t i = t / 48, rem = t - i * 48, blk = rem >> 3, y = rem & 7;
        int s[8], o[8];
        if (blk < 4) {
            const uint32_t yr = (blk >> 1) * 8 + y, c = i * 4 + (blk & 1) * 2;
            const uint32_t a = ys[yr][c], b = ys[yr][c + 1];
#pragma unroll
            for (int k = 0; k < 4; k++) { s[k] = (int)((a >> (8 * k)) & 0xFF) - 128; s[4 + k] = (int)((b >> (8 * k)) & 0xFF) - 128; }
        } else {
            const uint32_t(*cs)[17] = blk == 4 ? cbs : crs;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t a = cs[2 * y][i * 4 + k], b = cs[2 * y + 1][i * 4 + k];
                s[2 * k] = (int)(((a & 0xFFFF) + (b & 0xFFFF) + 2) >> 2) - 128;
                s[2 * k + 1] = (int)(((a >> 16) + (b >> 16) + 2) >> 2) - 128;
            }
        }
        jpg_dct8(s, o);
#pragma unroll
        for (int u = 0; u < 8; u++) ab[i * 6 + blk][y][u] = (o[u] + 128) >> 8;
    }
    __syncthreads();
    // 3. columns, quantisation, scan order: a thread takes one column of one block
    if (t < JPG_GROUP * 48) {
        const uint32_t b = t >> 3, u = t & 7, tab = (b % 6) >= 4 ? 64 : 0;
        int s[8], o[8];
#pragma unroll
        for (int y = 0; y < 8; y++) s[y] = ab[b][y][u];
        jpg_dct8(s, o);
#pragma unroll
        for (int v = 0; v < 8; v++) {
            const uint32_t n = v * 8 + u, Q = s_q[tab + n];
            const uint32_t dividend = ((uint32_t)abs(o[v]) + (Q << 17)) >> 18;            // below 2^12
            int q = (int)((dividend * s_recip[tab + n]) >> 20);
            if (n) q = min(q, 1023);
            zz[b][s_izig[n]] = (int16_t)(o[v] < 0 ? -q : q);
        }
    }
    __syncthreads();
    // 4. the bits of each block's AC symbols: a wave takes a block, a lane a coefficient
    {
        const uint32_t lane = t & 63, wave = t >> 6;
        for (uint32_t b = wave; b < JPG_GROUP * 6; b += 4) {
            const int v = zz[b][lane];
            const uint8_t *al = s_aclen + ((b % 6) >= 4 ? 256 : 0);
            const unsigned long long mask = __ballot(v != 0);
            uint32_t bits = 0;
            if (lane && v) {
                const unsigned long long below = mask & ((1ull << lane) - 1ull) & ~1ull;
                const uint32_t prev = below ? 63u - (uint32_t)__clzll((long long)below) : 0u, run = lane - prev - 1u;
                const uint32_t cat = (uint32_t)jpg_category(v);
                bits = (run >> 4) * al[0xF0] + al[((run & 15) << 4) | cat] + cat;
            } else if (lane == 63) bits = al[0];
            for (int o = 32; o; o >>= 1) bits += __shfl_xor(bits, o);
            if (lane == 0) sb[b] = bits;
        }
    }
    __syncthreads();
    // 5. out: the group's MCUs lie side by side in HBM as well
    const JpgFrame fr(l, scratch, gridDim.y, f);
    const uint32_t m0 = r * l.mw + g * JPG_GROUP, nm = min((uint32_t)JPG_GROUP, l.mw - g * JPG_GROUP);
    uint32_t *dst = (uint32_t *)(fr.coef + (size_t)m0 * 384);
    for (uint32_t k = t; k < nm * 192; k += 256) dst[k] = ((const uint32_t *)&zz[0][0])[k];
    if (t < nm * 6) {
        fr.dcv[(size_t)m0 * 6 + t] = zz[t][0];
        fr.bbits[(size_t)m0 * 6 + t] = (uint16_t)sb[t];
    }
}

// grid.x = mh
__global__ __launch_bounds__(256) void k_jpg_scan_bits(const JpgLayout l, const JpgHuff hf, uint8_t *__restrict__ scratch)
{
    __shared__ uint32_t ws[4];
    __shared__ uint8_t s_dclen[24];
    const uint32_t t = threadIdx.x, f = blockIdx.y, r = blockIdx.x;
    if (t < 24) s_dclen[t] = (&hf.dc_len[0][0])[t];
    __syncthreads();
    const JpgFrame fr(l, scratch, gridDim.y, f);
    uint32_t carry = 0;
    for (uint32_t x0 = 0; x0 < l.mw; x0 += 256) {
        const uint32_t mx = x0 + t, m = r * l.mw + mx;
        uint32_t bits = 0;
        if (mx < l.mw) {
#pragma unroll
            for (int bj = 0; bj < 6; bj++) {
                const int cat = jpg_category(fr.dcv[(size_t)m * 6 + bj] - jpg_pred(fr.dcv, m, mx, bj));
                bits += fr.bbits[(size_t)m * 6 + bj] + s_dclen[(bj >= 4 ? 12 : 0) + cat] + cat;
            }
        }
        uint32_t total;
        const uint32_t at = jpg_scan256(bits, ws, &total);
        if (mx < l.mw) fr.off[m] = carry + at;
        carry += total;
    }
    if (t == 0) fr.rowbits[r] = carry;
}

// grid.x = frames
__global__ __launch_bounds__(LJE_SCAN_THREADS) void k_jpg_rows(const JpgLayout l, uint8_t *__restrict__ scratch, uint32_t nframes)
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
    const uint32_t nch = (l.mw + JPG_CHUNK - 1) / JPG_CHUNK;
    for (uint32_t k = threadIdx.x; k < l.mh * nch; k += LJE_SCAN_THREADS) {
        const uint32_t r = k / nch, ch = k - r * nch;
        if (ch) fr.rowbuf[fr.rowat[r] + (fr.off[r * l.mw + ch * JPG_CHUNK] >> 5)] = 0;
    }
}

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

// grid.x = ceil(mw / 16) * mh
__global__ __launch_bounds__(256) void k_jpg_emit(const JpgLayout l, const JpgHuff hf, uint8_t *__restrict__ scratch)
{
    constexpr int NB = JPG_CHUNK * 6;
    __shared__ uint32_t lbits[(NB * JPG_BLOCK_BITS + 31) / 32 + 3];
    __shared__ __attribute__((aligned(16))) int16_t lc[NB * 64];
    __shared__ uint16_t s_accode[512], s_dccode[24];
    __shared__ uint8_t s_aclen[512], s_dclen[24];
    __shared__ uint32_t boff[NB], ws[4];
    __shared__ int16_t sd[NB];
    const uint32_t t = threadIdx.x, f = blockIdx.y;
    if (((const JpgOut *)scratch)[f].status) return;
    const JpgFrame fr(l, scratch, gridDim.y, f);
    const uint32_t nch = (l.mw + JPG_CHUNK - 1) / JPG_CHUNK, r = blockIdx.x / nch, ch = blockIdx.x - r * nch;
    const uint32_t mx0 = ch * JPG_CHUNK, nm = min((uint32_t)JPG_CHUNK, l.mw - mx0), nblk = nm * 6, m0 = r * l.mw + mx0;
    s_accode[t] = (&hf.ac_code[0][0])[t];
    s_accode[t + 256] = (&hf.ac_code[0][0])[t + 256];
    s_aclen[t] = (&hf.ac_len[0][0])[t];
    s_aclen[t + 256] = (&hf.ac_len[0][0])[t + 256];
    if (t < 24) { s_dccode[t] = (&hf.dc_code[0][0])[t]; s_dclen[t] = (&hf.dc_len[0][0])[t]; }
    {
        const uint32_t *src = (const uint32_t *)(fr.coef + (size_t)m0 * 384);
        for (uint32_t k = t; k < nm * 192; k += 256) ((uint32_t *)lc)[k] = src[k];
    }
    __syncthreads();
    uint32_t x = 0;
    if (t < nblk) {
        const uint32_t mi = t / 6, bj = t - mi * 6;
        const int d = fr.dcv[(size_t)m0 * 6 + t] - jpg_pred(fr.dcv, m0 + mi, mx0 + mi, (int)bj), cat = jpg_category(d);
        sd[t] = (int16_t)d;
        x = fr.bbits[(size_t)m0 * 6 + t] + s_dclen[(bj >= 4 ? 12 : 0) + cat] + cat;
    }
    uint32_t nb;
    const uint32_t at = jpg_scan256(x, ws, &nb);
    if (t < nblk) boff[t] = at;
    const uint32_t begin = fr.off[m0], lead = begin & 31;
    const bool last = ch == nch - 1;
    const uint32_t pad = last ? (0u - (begin + nb)) & 7u : 0u, ndw = (lead + nb + pad + 31) >> 5;
    for (uint32_t k = t; k < ndw + 2; k += 256) lbits[k] = 0;
    __syncthreads();
    const uint32_t lane = t & 63, wave = t >> 6;
    for (uint32_t j = wave; j < nblk; j += 4) {
        const int v = lc[j * 64 + lane];
        const uint32_t tab = (j % 6) >= 4 ? 1 : 0;
        const uint8_t *al = s_aclen + 256 * tab;
        const uint16_t *ac = s_accode + 256 * tab;
        const unsigned long long mask = __ballot(v != 0);
        uint64_t V = 0;
        uint32_t L = 0;
        if (lane == 0) {
            const int d = sd[j];
            const uint32_t cat = (uint32_t)jpg_category(d);
            const uint32_t vb = (uint32_t)(d >= 0 ? d : d + (1 << cat) - 1) & ((1u << cat) - 1u);
            L = s_dclen[12 * tab + cat] + cat;
            V = ((uint64_t)s_dccode[12 * tab + cat] << cat) | vb;
        } else if (v) {
            const unsigned long long below = mask & ((1ull << lane) - 1ull) & ~1ull;
            const uint32_t prev = below ? 63u - (uint32_t)__clzll((long long)below) : 0u, run = lane - prev - 1u;
            const uint32_t cat = (uint32_t)jpg_category(v);
            const uint32_t vb = (uint32_t)(v >= 0 ? v : v + (1 << cat) - 1) & ((1u << cat) - 1u);
            for (uint32_t z = 0; z < (run >> 4); z++) { V = (V << al[0xF0]) | ac[0xF0]; L += al[0xF0]; }
            const uint32_t sym = ((run & 15) << 4) | cat, sl = al[sym];
            V = (V << (sl + cat)) | ((uint64_t)ac[sym] << cat) | vb;
            L += sl + cat;
        } else if (lane == 63) {
            L = al[0];
            V = ac[0];
        }
        uint32_t inc = L;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += u; }
        if (L) jpg_put(lbits, lead + boff[j] + inc - L, V, L);
    }
    if (t == 0 && pad) jpg_put(lbits, lead + nb, (1u << pad) - 1u, pad);
    __syncthreads();
    // the workgroup's dwords: whole ones stored, the two it may share with its neighbours in the row ORed into the zero that
    // k_jpg_rows put there
    uint32_t *g = fr.rowbuf + fr.rowat[r] + (begin >> 5);
    const bool shared_end = !last && ((lead + nb) & 31);
    for (uint32_t k = t; k < ndw; k += 256) {
        const uint32_t w = lbits[k];
        if ((k == 0 && lead) || (k == ndw - 1 && shared_end)) atomicOr(&g[k], w);
        else g[k] = w;
    }
}

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

int jpg_launch(const uint8_t *d_rgb, size_t stride, const JpgLayout &l, const JpgQuant &q, const JpgHuff &h, uint8_t *d_out, size_t out_stride,
               uint32_t room, uint8_t *d_scratch, int nframes, hipStream_t s)
{
    if (nframes <= 0) return MLVFS_AMD_OK;
    const uint32_t n = (uint32_t)nframes, gx = (l.mw + JPG_GROUP - 1) / JPG_GROUP, nch = (l.mw + JPG_CHUNK - 1) / JPG_CHUNK;
    hipLaunchKernelGGL(k_jpg_transform, dim3(gx * l.mh, n), dim3(256), 0, s, d_rgb, stride, l, q, h, d_scratch);
    hipLaunchKernelGGL(k_jpg_scan_bits, dim3(l.mh, n), dim3(256), 0, s, l, h, d_scratch);
    hipLaunchKernelGGL(k_jpg_rows, dim3(n), dim3(LJE_SCAN_THREADS), 0, s, l, d_scratch, n);
    hipLaunchKernelGGL(k_jpg_emit, dim3(nch * l.mh, n), dim3(256), 0, s, l, h, d_scratch);
    hipLaunchKernelGGL(k_jpg_count_ff, dim3(l.mh, n), dim3(256), 0, s, l, d_scratch);
    hipLaunchKernelGGL(k_jpg_place, dim3(n), dim3(LJE_SCAN_THREADS), 0, s, l, d_scratch, n, room);
    hipLaunchKernelGGL(k_jpg_stuff, dim3(l.mh, n), dim3(256), 0, s, l, d_scratch, d_out, out_stride);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

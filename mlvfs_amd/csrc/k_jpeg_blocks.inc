// k_jpeg_blocks.inc -- the three kernels of k_jpeg.hip that see blocks, which k_jpeg.hip includes once per chroma sampling (DESIGN.md
// 3.21) with JPG_S, the sampling (an index of kJpgModes, jpeg.h), and JPG_K(name), the kernel's name at that sampling: k_jpg_transform,
// k_jpg_transform_422, k_jpg_transform_444, and so on.  At 4:2:0 the text is the kernels as they were before there was a choice.

// grid.x = ceil(mw / GROUP) * mh
__global__ __launch_bounds__(256) void JPG_K(k_jpg_transform)(const uint8_t *__restrict__ rgb, size_t stride, const JpgLayout l, const JpgQuant qt, const JpgHuff hf,
                                                              uint8_t *__restrict__ scratch)
{
    constexpr int S = JPG_S;
    constexpr int NB = kJpgModes[S].nb, NY = kJpgModes[S].ny, GROUP = kJpgModes[S].group, NBLK = GROUP * NB;
    constexpr int ROWS = kJpgModes[S].mch;               // of the workgroup's tile, which is 64 pixels wide at every sampling
    constexpr int CW = S == MLVFS_AMD_JPEG_444 ? 18 : 17;
    static_assert(GROUP * kJpgModes[S].mcw == 64 && NBLK * 8 <= 256, "a tile of 64 pixels; a thread per row of a block");
    __shared__ uint32_t ys[ROWS][18];                    // a row: 64 samples in 16 dwords, 2 dwords of padding
    // a row at 4:2:0: 32 sums of two neighbours, 16 bits each, 1 dword of padding; at 4:2:2: their 32 rounded means, likewise; at 4:4:4:
    // 64 samples as in ys
    __shared__ uint32_t cbs[ROWS][CW], crs[ROWS][CW];
    __shared__ int ab[NBLK][8][9];                       // after the row pass; a row of 8 in 9 dwords: the column pass reads down
    __shared__ __attribute__((aligned(16))) int16_t zz[NBLK][64];
    __shared__ uint32_t s_recip[128], sb[NBLK];
    __shared__ uint8_t s_q[128], s_izig[64], s_aclen[512];
    const uint32_t t = threadIdx.x, f = blockIdx.y;
    const uint32_t gx = (l.mw + GROUP - 1) / GROUP, r = blockIdx.x / gx, g = blockIdx.x - r * gx;
    if (t < 128) { s_recip[t] = (&qt.recip[0][0])[t]; s_q[t] = (&qt.q[0][0])[t]; }
    if (t < 64) s_izig[t] = kIzig[t];
    s_aclen[t] = (&hf.ac_len[0][0])[t];
    s_aclen[t + 256] = (&hf.ac_len[0][0])[t + 256];
    // 1. colour: a thread takes 4 pixels of one of the tile's rows (16, or 8: then half of the threads)
    if (ROWS == 16 || t < ROWS * 16) {
        const uint32_t y = t >> 4, xg = t & 15, X = 64 * g + 4 * xg, Y = min(ROWS * r + y, l.ph - 1);
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
        if constexpr (S == MLVFS_AMD_JPEG_420) {
            cbs[y][xg] = (cb[0] + cb[1]) | ((cb[2] + cb[3]) << 16);
            crs[y][xg] = (cr[0] + cr[1]) | ((cr[2] + cr[3]) << 16);
        } else if constexpr (S == MLVFS_AMD_JPEG_422) {
            cbs[y][xg] = ((cb[0] + cb[1] + 1) >> 1) | (((cb[2] + cb[3] + 1) >> 1) << 16);
            crs[y][xg] = ((cr[0] + cr[1] + 1) >> 1) | (((cr[2] + cr[3] + 1) >> 1) << 16);
        } else {
            cbs[y][xg] = cb[0] | (cb[1] << 8) | (cb[2] << 16) | (cb[3] << 24);
            crs[y][xg] = cr[0] | (cr[1] << 8) | (cr[2] << 16) | (cr[3] << 24);
        }
    }
    __syncthreads();
    // 2. rows: a thread takes one row of one of the blocks
    if (t < NBLK * 8) {
        const uint32_t i = t / (NB * 8), rem = t - i * (NB * 8), blk = rem >> 3, y = rem & 7;
        int s[8], o[8];
        if (blk < NY) {
            // the block's row in the tile and the first of its two dwords there: an MCU is 4 dwords wide, at 4:4:4 two
            const uint32_t yr = S == MLVFS_AMD_JPEG_420 ? (blk >> 1) * 8 + y : y;
            const uint32_t c = S == MLVFS_AMD_JPEG_420 ? i * 4 + (blk & 1) * 2 : S == MLVFS_AMD_JPEG_422 ? i * 4 + blk * 2 : i * 2;
            const uint32_t a = ys[yr][c], b = ys[yr][c + 1];
#pragma unroll
            for (int k = 0; k < 4; k++) { s[k] = (int)((a >> (8 * k)) & 0xFF) - 128; s[4 + k] = (int)((b >> (8 * k)) & 0xFF) - 128; }
        } else {
            const uint32_t(*cs)[CW] = blk == NY ? cbs : crs;
            if constexpr (S == MLVFS_AMD_JPEG_420) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t a = cs[2 * y][i * 4 + k], b = cs[2 * y + 1][i * 4 + k];
                    s[2 * k] = (int)(((a & 0xFFFF) + (b & 0xFFFF) + 2) >> 2) - 128;
                    s[2 * k + 1] = (int)(((a >> 16) + (b >> 16) + 2) >> 2) - 128;
                }
            } else if constexpr (S == MLVFS_AMD_JPEG_422) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t a = cs[y][i * 4 + k];
                    s[2 * k] = (int)(a & 0xFFFF) - 128;
                    s[2 * k + 1] = (int)(a >> 16) - 128;
                }
            } else {
                const uint32_t a = cs[y][i * 2], b = cs[y][i * 2 + 1];
#pragma unroll
                for (int k = 0; k < 4; k++) { s[k] = (int)((a >> (8 * k)) & 0xFF) - 128; s[4 + k] = (int)((b >> (8 * k)) & 0xFF) - 128; }
            }
        }
        jpg_dct8(s, o);
#pragma unroll
        for (int u = 0; u < 8; u++) ab[i * NB + blk][y][u] = (o[u] + 128) >> 8;
    }
    __syncthreads();
    // 3. columns, quantisation, scan order: a thread takes one column of one block
    if (t < NBLK * 8) {
        const uint32_t b = t >> 3, u = t & 7, tab = (b % NB) >= NY ? 64 : 0;
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
        for (uint32_t b = wave; b < NBLK; b += 4) {
            const int v = zz[b][lane];
            const uint8_t *al = s_aclen + ((b % NB) >= NY ? 256 : 0);
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
    const uint32_t m0 = r * l.mw + g * GROUP, nm = min((uint32_t)GROUP, l.mw - g * GROUP);
    uint32_t *dst = (uint32_t *)(fr.coef + (size_t)m0 * (NB * 64));
    for (uint32_t k = t; k < nm * (NB * 32); k += 256) dst[k] = ((const uint32_t *)&zz[0][0])[k];
    if (t < nm * NB) {
        fr.dcv[(size_t)m0 * NB + t] = zz[t][0];
        fr.bbits[(size_t)m0 * NB + t] = (uint16_t)sb[t];
    }
}

// grid.x = mh
__global__ __launch_bounds__(256) void JPG_K(k_jpg_scan_bits)(const JpgLayout l, const JpgHuff hf, uint8_t *__restrict__ scratch)
{
    constexpr int S = JPG_S;
    __shared__ uint32_t ws[4];
    __shared__ uint8_t s_dclen[24];
    const uint32_t t = threadIdx.x, f = blockIdx.y, r = blockIdx.x;
    if (t < 24) s_dclen[t] = (&hf.dc_len[0][0])[t];
    __syncthreads();
    const JpgFrame fr(l, scratch, gridDim.y, f);
    constexpr int NB = kJpgModes[S].nb, NY = kJpgModes[S].ny;
    uint32_t carry = 0;
    for (uint32_t x0 = 0; x0 < l.mw; x0 += 256) {
        const uint32_t mx = x0 + t, m = r * l.mw + mx;
        uint32_t bits = 0;
        if (mx < l.mw) {
#pragma unroll
            for (int bj = 0; bj < NB; bj++) {
                const int cat = jpg_category(fr.dcv[(size_t)m * NB + bj] - jpg_pred<S>(fr.dcv, m, mx, bj));
                bits += fr.bbits[(size_t)m * NB + bj] + s_dclen[(bj >= NY ? 12 : 0) + cat] + cat;
            }
        }
        uint32_t total;
        const uint32_t at = jpg_scan256(bits, ws, &total);
        if (mx < l.mw) fr.off[m] = carry + at;
        carry += total;
    }
    if (t == 0) fr.rowbits[r] = carry;
}

// grid.x = ceil(mw / CHUNK) * mh
__global__ __launch_bounds__(256) void JPG_K(k_jpg_emit)(const JpgLayout l, const JpgHuff hf, uint8_t *__restrict__ scratch)
{
    constexpr int S = JPG_S;
    constexpr int NB = kJpgModes[S].nb, NY = kJpgModes[S].ny, CHUNK = kJpgModes[S].chunk, NBLK = CHUNK * NB;
    static_assert(NBLK <= 256, "a thread per block");
    __shared__ uint32_t lbits[(NBLK * JPG_BLOCK_BITS + 31) / 32 + 3];
    __shared__ __attribute__((aligned(16))) int16_t lc[NBLK * 64];
    __shared__ uint16_t s_accode[512], s_dccode[24];
    __shared__ uint8_t s_aclen[512], s_dclen[24];
    __shared__ uint32_t boff[NBLK], ws[4];
    __shared__ int16_t sd[NBLK];
    const uint32_t t = threadIdx.x, f = blockIdx.y;
    if (((const JpgOut *)scratch)[f].status) return;
    const JpgFrame fr(l, scratch, gridDim.y, f);
    const uint32_t nch = (l.mw + CHUNK - 1) / CHUNK, r = blockIdx.x / nch, ch = blockIdx.x - r * nch;
    const uint32_t mx0 = ch * CHUNK, nm = min((uint32_t)CHUNK, l.mw - mx0), nblk = nm * NB, m0 = r * l.mw + mx0;
    s_accode[t] = (&hf.ac_code[0][0])[t];
    s_accode[t + 256] = (&hf.ac_code[0][0])[t + 256];
    s_aclen[t] = (&hf.ac_len[0][0])[t];
    s_aclen[t + 256] = (&hf.ac_len[0][0])[t + 256];
    if (t < 24) { s_dccode[t] = (&hf.dc_code[0][0])[t]; s_dclen[t] = (&hf.dc_len[0][0])[t]; }
    {
        const uint32_t *src = (const uint32_t *)(fr.coef + (size_t)m0 * (NB * 64));
        for (uint32_t k = t; k < nm * (NB * 32); k += 256) ((uint32_t *)lc)[k] = src[k];
    }
    __syncthreads();
    uint32_t x = 0;
    if (t < nblk) {
        const uint32_t mi = t / NB, bj = t - mi * NB;
        const int d = fr.dcv[(size_t)m0 * NB + t] - jpg_pred<S>(fr.dcv, m0 + mi, mx0 + mi, (int)bj), cat = jpg_category(d);
        sd[t] = (int16_t)d;
        x = fr.bbits[(size_t)m0 * NB + t] + s_dclen[(bj >= NY ? 12 : 0) + cat] + cat;
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
        const uint32_t tab = (j % NB) >= NY ? 1 : 0;
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

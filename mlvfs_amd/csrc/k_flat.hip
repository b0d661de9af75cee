// k_flat.hip -- flat-field (gain) correction on 16-bit frames in HBM and the gain plane it multiplies by (csrc/flat.cpp).
//
// The reference has no flat-field code; the definition is this project's (what `mlv_dump -t` does a frame at a time on a host core),
// in integers only.  F is the flat plane, w x h 16-bit values with a pedestal black_f:
//     s[p]    = max(F[p] - black_f, 1)
//     c       = (y & 1) * 2 + (x & 1)                                        by position in the stored frame
//     M_c     = (sum of s[p] over channel c + n_c / 2) / n_c                 64-bit sums; n_c pixels of channel c
//     gain[p] = min((M_c * 16384 + s[p] / 2) / s[p], 65535)                  Q14, 16384 = 1.0; M_c * 16384 < 2^30
//     out     = clamp(black + floor(((px - black) * gain[p] + 8192) / 16384), 0, 2^bpp - 1)
// with the frame's own black level and depth.  A gain stops at 65535 / 16384, just under 4.0.  With a dark frame the pixel is
// subtracted first (k_dark.hip's formula), in the same pass.  A frame value above 2^bpp - 1 (a damaged LJ92 stream can decode to
// one) is taken as 2^bpp - 1, in every form: the 32-bit products below rest on px <= 2^bpp - 1.
//
// All HBM-bound, laid out like k_dark.hip: one lane moves 16 bytes per load, the lanes of a wave are contiguous, frames are batched in
// grid.y, and the gain plane (and the dark plane) is read by every frame of a batch.
//   k_flat_chan_sums     the four 64-bit channel sums of s[p]: a lane takes 16 pixels in a row of the linear index and walks (y, x)
//                        from it -- with an odd width the channel pattern changes from row to row, also inside those 16 --, then the
//                        wave, then the workgroup, then one 64-bit atomic add per channel per workgroup into a zeroed buffer
//   k_flat_gain          F, black_f and the sums -> the Q14 plane, 8 pixels per lane; block 0 leaves the four M_c behind the plane
//   k_flat_apply_x16<DARK>   in place, 32-bit products: depths up to 15 bits with 0 <= black <= 32767 (32767 * 65535 + 8192 < 2^31);
//                        one lane = 16 pixels as in k_dark_sub_x16
//   k_flat_apply_generic any size, 2-byte alignment, any depth and black level: one lane = one pixel, 64-bit products
//   k_flat_unpack_x16<14 | 12 | 10, DARK>   k_unpack_x16's unpack, the optional dark frame and the gain in one pass
// Pad bytes between frames are never touched.
#include "clip.h"
#include "k_unpack_dev.h"

namespace mlv {

// ---- the gain plane ---------------------------------------------------------------------------------------------------------
// (y, x) of a linear index and the walk to the next pixel
struct BayerWalk {
    uint32_t x, y, w;
    __device__ __forceinline__ BayerWalk(uint32_t k, uint32_t w_) : x(k % w_), y(k / w_), w(w_) {}
    __device__ __forceinline__ int channel() const { return (int)((y & 1) * 2 + (x & 1)); }
    __device__ __forceinline__ void step() { if (++x == w) { x = 0; y++; } }
};

__device__ __forceinline__ uint32_t flat_signal(uint32_t f, int black_f) { return (uint32_t)max((int)f - black_f, 1); }

__device__ __forceinline__ void sum_px2(uint32_t (&acc)[4], BayerWalk &at, uint32_t two, int black_f)
{
    acc[at.channel()] += flat_signal(two & 0xFFFFu, black_f); at.step();
    acc[at.channel()] += flat_signal(two >> 16, black_f);     at.step();
}

__device__ __forceinline__ void sum_px8(uint32_t (&acc)[4], BayerWalk &at, uint4 p, int black_f)
{
    sum_px2(acc, at, p.x, black_f); sum_px2(acc, at, p.y, black_f); sum_px2(acc, at, p.z, black_f); sum_px2(acc, at, p.w, black_f);
}

// plane: 16-byte aligned (the library's own allocation); sums[4]: zeroed by the caller.  The last lane's group may be short.
__global__ __launch_bounds__(256) void k_flat_chan_sums(const uint16_t *__restrict__ plane, uint32_t npix, uint32_t w, int black_f,
                                                        unsigned long long *__restrict__ sums)
{
    __shared__ unsigned long long part[4][4];            // [wave][channel]
    const uint32_t groups = (npix + 15) / 16;
    unsigned long long total[4] = { 0, 0, 0, 0 };
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint32_t acc[4] = { 0, 0, 0, 0 };                 // 16 values below 2^16
        BayerWalk at(g * 16, w);
        if (g * 16 + 16 <= npix) {
            const uint4 lo = ((const uint4 *)plane)[(size_t)g * 2], hi = ((const uint4 *)plane)[(size_t)g * 2 + 1];
            sum_px8(acc, at, lo, black_f);
            sum_px8(acc, at, hi, black_f);
        } else {
            for (uint32_t k = g * 16; k < npix; k++) { acc[at.channel()] += flat_signal(plane[k], black_f); at.step(); }
        }
#pragma unroll
        for (int c = 0; c < 4; c++) total[c] += acc[c];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        for (int off = 32; off > 0; off >>= 1) total[c] += __shfl_down(total[c], off, 64);
        if (lane == 0) part[wave][c] = total[c];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (v) atomicAdd(&sums[threadIdx.x], v);
    }
}

struct FlatCounts { uint32_t n[4]; };                    // pixels per channel; 0: the channel does not exist and is never read

__device__ __forceinline__ uint32_t gain_px(uint32_t f, int black_f, uint32_t mean)
{
    const uint32_t s = flat_signal(f, black_f);
    return min((mean * 16384u + s / 2) / s, 65535u);     // mean <= 65535: below 2^30 + 2^15
}

__device__ __forceinline__ uint32_t gain_px2(BayerWalk &at, uint32_t two, int black_f, const uint32_t (&mean)[4])
{
    const uint32_t a = gain_px(two & 0xFFFFu, black_f, mean[at.channel()]); at.step();
    const uint32_t b = gain_px(two >> 16, black_f, mean[at.channel()]);     at.step();
    return a | (b << 16);
}

// gain: npix values, 16-byte aligned; means_out[4]: written by block 0
__global__ __launch_bounds__(256) void k_flat_gain(const uint16_t *__restrict__ plane, uint32_t npix, uint32_t w, int black_f,
                                                   const unsigned long long *__restrict__ sums, FlatCounts counts, uint16_t *__restrict__ gain,
                                                   uint32_t *__restrict__ means_out)
{
    __shared__ uint32_t mean_s[4];
    if (threadIdx.x < 4) {
        const uint32_t n = counts.n[threadIdx.x];
        const uint32_t m = n ? (uint32_t)((sums[threadIdx.x] + n / 2) / n) : 0;
        mean_s[threadIdx.x] = m;
        if (blockIdx.x == 0) means_out[threadIdx.x] = m;
    }
    __syncthreads();
    const uint32_t mean[4] = { mean_s[0], mean_s[1], mean_s[2], mean_s[3] };
    const uint32_t groups = (npix + 7) / 8;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        BayerWalk at(g * 8, w);
        if (g * 8 + 8 <= npix) {
            const uint4 p = ((const uint4 *)plane)[g];
            uint4 r;
            r.x = gain_px2(at, p.x, black_f, mean); r.y = gain_px2(at, p.y, black_f, mean);
            r.z = gain_px2(at, p.z, black_f, mean); r.w = gain_px2(at, p.w, black_f, mean);
            ((uint4 *)gain)[g] = r;
        } else {
            for (uint32_t k = g * 8; k < npix; k++) { gain[k] = (uint16_t)gain_px(plane[k], black_f, mean[at.channel()]); at.step(); }
        }
    }
}

// ---- the application --------------------------------------------------------------------------------------------------------
// px <= top <= 32767 (the callers clamp: the unpack masks, the dark frame's clamp, or clamp_px8), 0 <= black <= 32767 and
// gain <= 65535: the product and the rounding term fit 32 signed bits; >> of a negative int is arithmetic
__device__ __forceinline__ uint32_t flat_px(uint32_t px, uint32_t gain, int black, int top)
{
    const int v = black + ((((int)px - black) * (int)gain + 8192) >> 14);
    return (uint32_t)min(max(v, 0), top);
}

template <bool DARK>
__device__ __forceinline__ uint32_t flat_px2(uint32_t p, uint32_t g, uint32_t d, int black, int top, int black_d)
{
    uint32_t a = p & 0xFFFFu, b = p >> 16;
    if (DARK) {
        a = (uint32_t)min(max((int)a - (int)(d & 0xFFFFu) + black_d, 0), top);
        b = (uint32_t)min(max((int)b - (int)(d >> 16) + black_d, 0), top);
    }
    return flat_px(a, g & 0xFFFFu, black, top) | (flat_px(b, g >> 16, black, top) << 16);
}

template <bool DARK>
__device__ __forceinline__ uint4 flat_px8(uint4 p, uint4 g, uint4 d, int black, int top, int black_d)
{
    uint4 r;
    r.x = flat_px2<DARK>(p.x, g.x, d.x, black, top, black_d); r.y = flat_px2<DARK>(p.y, g.y, d.y, black, top, black_d);
    r.z = flat_px2<DARK>(p.z, g.z, d.z, black, top, black_d); r.w = flat_px2<DARK>(p.w, g.w, d.w, black, top, black_d);
    return r;
}

// decoded frames may hold anything: values above top become top (with a dark frame its clamp does that)
__device__ __forceinline__ uint32_t clamp_px2(uint32_t p, uint32_t top) { return min(p & 0xFFFFu, top) | (min(p >> 16, top) << 16); }

__device__ __forceinline__ uint4 clamp_px8(uint4 p, uint32_t top)
{
    uint4 r;
    r.x = clamp_px2(p.x, top); r.y = clamp_px2(p.y, top); r.z = clamp_px2(p.z, top); r.w = clamp_px2(p.w, top);
    return r;
}

// a lane's 16 pixels are two runs of 8, `groups` runs apart (k_dark_sub_x16's layout)
template <bool DARK>
__global__ __launch_bounds__(256) void k_flat_apply_x16(uint8_t *__restrict__ frames, size_t stride, const uint4 *__restrict__ gain,
                                                        const uint4 *__restrict__ dark, uint32_t groups, int black, int top, int black_d)
{
    uint4 *f = (uint4 *)(frames + (size_t)blockIdx.y * stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint4 a = f[g], b = f[(size_t)g + groups];
        const uint4 ga = gain[g], gb = gain[(size_t)g + groups];
        uint4 da = {}, db = {};
        if (DARK) { da = dark[g]; db = dark[(size_t)g + groups]; }
        else { a = clamp_px8(a, (uint32_t)top); b = clamp_px8(b, (uint32_t)top); }
        f[g] = flat_px8<DARK>(a, ga, da, black, top, black_d);
        f[(size_t)g + groups] = flat_px8<DARK>(b, gb, db, black, top, black_d);
    }
}

// dark: nullptr for none.  64-bit products: 16-bit frames (65535 * 65535) and any black level a header may hold are exact.
__global__ __launch_bounds__(256) void k_flat_apply_generic(uint8_t *__restrict__ frames, size_t stride, const uint16_t *__restrict__ gain,
                                                            const uint16_t *__restrict__ dark, uint32_t npix, int black, int top, int black_d)
{
    uint16_t *f = (uint16_t *)(frames + (size_t)blockIdx.y * stride);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x) {
        int px = f[k];
        px = dark ? min(max(px - (int)dark[k] + black_d, 0), top) : min(px, top);
        const long long v = (long long)black + ((((long long)px - black) * (long long)gain[k] + 8192) >> 14);
        f[k] = (uint16_t)min(max(v, 0ll), (long long)top);
    }
}

template <int BPP, bool DARK>
__global__ __launch_bounds__(256) void k_flat_unpack_x16(const uint8_t *__restrict__ packed, size_t packed_stride, uint8_t *__restrict__ out,
                                                         size_t out_stride, const uint4 *__restrict__ gain, const uint4 *__restrict__ dark,
                                                         uint32_t groups, int black, int black_d)
{
    constexpr int NW = BPP / 2;
    constexpr int top = (1 << BPP) - 1;
    const uint32_t *src = (const uint32_t *)(packed + (size_t)blockIdx.y * packed_stride);
    uint4 *dst = (uint4 *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint32_t s[NW], px[16];
#pragma unroll
        for (int i = 0; i < NW; i++) s[i] = stream_word(src[(size_t)g * NW + i]);
        const uint4 ga = gain[(size_t)g * 2], gb = gain[(size_t)g * 2 + 1];
        uint4 da = {}, db = {};
        if (DARK) { da = dark[(size_t)g * 2]; db = dark[(size_t)g * 2 + 1]; }
        unpack_x16<BPP>(s, px);
        uint4 lo, hi;
        lo.x = px[0] | (px[1] << 16);   lo.y = px[2] | (px[3] << 16);
        lo.z = px[4] | (px[5] << 16);   lo.w = px[6] | (px[7] << 16);
        hi.x = px[8] | (px[9] << 16);   hi.y = px[10] | (px[11] << 16);
        hi.z = px[12] | (px[13] << 16); hi.w = px[14] | (px[15] << 16);
        dst[(size_t)g * 2] = flat_px8<DARK>(lo, ga, da, black, top, black_d);
        dst[(size_t)g * 2 + 1] = flat_px8<DARK>(hi, gb, db, black, top, black_d);
    }
}

static uint32_t flat_grid_x(uint32_t items, uint32_t cap) { return std::min<uint32_t>((items + 255) / 256, cap); }

static bool flat_in_32_bits(const FlatFieldDev &flat) { return flat.top <= 32767 && flat.black >= 0 && flat.black <= 32767; }

// d_plane, d_gain: the library's own allocations (16-byte aligned), npix values each; d_sums[4]: zeroed here; d_means[4]: the M_c
int launch_flat_gain(const uint16_t *d_plane, uint32_t w, uint32_t h, int black_f, unsigned long long *d_sums, uint16_t *d_gain,
                     uint32_t *d_means, hipStream_t stream)
{
    const uint32_t npix = w * h;
    if (npix == 0) return MLVFS_AMD_OK;
    MLV_HIP(hipMemsetAsync(d_sums, 0, 4 * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(k_flat_chan_sums, dim3(flat_grid_x((npix + 15) / 16, 1024)), dim3(256), 0, stream, d_plane, npix, w, black_f, d_sums);
    MLV_HIP(hipGetLastError());
    FlatCounts counts;
    for (int c = 0; c < 4; c++) counts.n[c] = ((h + 1 - (uint32_t)(c >> 1)) / 2) * ((w + 1 - (uint32_t)(c & 1)) / 2);
    hipLaunchKernelGGL(k_flat_gain, dim3(flat_grid_x((npix + 7) / 8, 8192)), dim3(256), 0, stream, d_plane, npix, w, black_f,
                       (const unsigned long long *)d_sums, counts, d_gain, d_means);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// in place; dark: the dark frame to subtract first, in the same pass, or nullptr.  The callers have checked the geometry.
int launch_flat_apply(void *d_frames, size_t stride, uint32_t npix, int nframes, const FlatFieldDev &flat, const DarkFrameDev *dark,
                      hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    const bool fast = flat_in_32_bits(flat) && npix % 16 == 0 && ((uintptr_t)d_frames % 16 == 0) && ((uintptr_t)flat.d_gain % 16 == 0) &&
                      (!dark || (uintptr_t)dark->d_plane % 16 == 0) && (nframes == 1 || stride % 16 == 0);
    if (fast) {
        const uint32_t groups = npix / 16;
        const dim3 grid(flat_grid_x(groups, 8192), nframes);
        auto kern = dark ? k_flat_apply_x16<true> : k_flat_apply_x16<false>;
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, (uint8_t *)d_frames, stride, (const uint4 *)flat.d_gain,
                           (const uint4 *)(dark ? dark->d_plane : nullptr), groups, flat.black, flat.top, dark ? dark->black : 0);
    } else {
        const dim3 grid(flat_grid_x(npix, 16384), nframes);
        hipLaunchKernelGGL(k_flat_apply_generic, grid, dim3(256), 0, stream, (uint8_t *)d_frames, stride, flat.d_gain,
                           dark ? dark->d_plane : (const uint16_t *)nullptr, npix, flat.black, flat.top, dark ? dark->black : 0);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

template <int BPP>
static auto flat_unpack_kernel(bool dark) { return dark ? k_flat_unpack_x16<BPP, true> : k_flat_unpack_x16<BPP, false>; }

// packed payloads -> corrected 16-bit frames: one pass where k_unpack_x16 would run, else launch_unpack + launch_flat_apply
int launch_flat_unpack(const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride, uint32_t npix, int bpp, int nframes,
                       const FlatFieldDev &flat, const DarkFrameDev *dark, hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    const bool fast = (bpp == 14 || bpp == 12 || bpp == 10) && flat.top == (1 << bpp) - 1 && flat_in_32_bits(flat) &&
                      (!dark || (dark->top == flat.top && (uintptr_t)dark->d_plane % 16 == 0)) && npix % 16 == 0 &&
                      ((uintptr_t)d_packed % 4 == 0) && ((uintptr_t)d_out % 16 == 0) && ((uintptr_t)flat.d_gain % 16 == 0) &&
                      (nframes == 1 || (packed_stride % 4 == 0 && out_stride % 16 == 0));
    if (!fast) {
        if (int rc = launch_unpack(d_packed, packed_stride, d_out, out_stride, 0, npix, bpp, nframes, stream)) return rc;
        return launch_flat_apply(d_out, out_stride, npix, nframes, flat, dark, stream);
    }
    const uint32_t groups = npix / 16;
    const dim3 grid(flat_grid_x(groups, 8192), nframes);
    auto kern = bpp == 14 ? flat_unpack_kernel<14>(dark) : (bpp == 12 ? flat_unpack_kernel<12>(dark) : flat_unpack_kernel<10>(dark));
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream, (const uint8_t *)d_packed, packed_stride, (uint8_t *)d_out, out_stride,
                       (const uint4 *)flat.d_gain, (const uint4 *)(dark ? dark->d_plane : nullptr), groups, flat.black, dark ? dark->black : 0);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

// k_cal.hip -- the calibration stage: a frame corrected pixel by pixel with device-resident planes while it is loaded, and the
// kernels that make those planes (csrc/cal.cpp).  The reference has no such code; the definitions are this
// project's (what `mlv_dump -s` / `-a` / `-t` do a frame at a time on a host core), in integers only.
//
// Stage 0, the dark frame: a plane of w x h 16-bit values with a pedestal black_d, the black level of the clip it was averaged from
//     out     = clamp(px - dark + black_d, 0, 2^bpp - 1)                     in 32-bit signed arithmetic
//     dark[p] = (sum over the n frames of px_f[p] + n / 2) / n               32-bit unsigned sums, n <= 65536: no overflow
// Stage 0b, the flat field, on stage 0's result: F is the flat plane, w x h 16-bit values with a pedestal black_f
//     s[p]    = max(F[p] - black_f, 1)
//     c       = (y & 1) * 2 + (x & 1)                                        by position in the stored frame
//     M_c     = (sum of s[p] over channel c + n_c / 2) / n_c                 64-bit sums; n_c pixels of channel c
//     gain[p] = min((M_c * 16384 + s[p] / 2) / s[p], 65535)                  Q14, 16384 = 1.0; M_c * 16384 < 2^30
//     out     = clamp(black + floor(((px - black) * gain[p] + 8192) / 16384), 0, 2^bpp - 1)
// with the frame's own black level and depth.  A gain stops at 65535 / 16384, just under 4.0.  Both planes are applied by position in
// the stored frame (xRes x yRes): the frame's panPosX/Y and cropPosX/Y are ignored.  A frame value above 2^bpp - 1 (a damaged LJ92
// stream can decode to one) is taken as 2^bpp - 1, in every form: the 32-bit products rest on px <= 2^bpp - 1.
//
// All HBM-bound.  One lane moves 16 bytes per load; the lanes of a wave are contiguous; frames are batched in grid.y.  The planes are
// read by every frame of a batch (9.5 MB each at 3584x1320: they stay in the last-level cache).
//   k_cal_apply_x16<DARK, FLAT>   in place; one lane = 16 pixels (two runs of 8, half a frame apart) = two 128-bit loads of the frame, two
//                        of each plane, two 128-bit stores, each contiguous across the wave.  With FLAT, 32-bit products: depths up to 15
//                        bits with 0 <= black <= 32767
//   k_cal_apply_generic  any size, 2-byte alignment, any depth and black level; one lane = one pixel; 64-bit products where there is a gain
//   k_cal_unpack_x16<14 | 12 | 10, DARK, FLAT>   k_unpack_x16's unpack and the correction in one pass: packed stream in, frames out
//   k_dark_accum_x16 / k_dark_accum_generic   a batch of frames added to a uint32 plane: a lane owns its pixels, walks the batch's frames
//                        with the sums in registers and makes one read-modify-write of the plane
//   k_dark_mean          the rounded mean of the sums as 16-bit values
//   k_flat_chan_sums     the four 64-bit channel sums of s[p]: a lane takes 16 pixels in a row of the linear index and walks (y, x)
//                        from it -- with an odd width the channel pattern changes from row to row, also inside those 16 --, then the
//                        wave, then the workgroup, then one 64-bit atomic add per channel per workgroup into a zeroed buffer
//   k_flat_gain          F, black_f and the sums -> the Q14 plane, 8 pixels per lane; block 0 leaves the four M_c behind the plane
// Pad bytes between frames are never touched.
#include "clip.h"
#include "k_cal_dev.h"
#include "k_unpack_dev.h"

namespace mlv {

// ---- the application --------------------------------------------------------------------------------------------------------
// a lane's 16 pixels are two runs of 8, `groups` runs apart: the lanes of a wave are 16 bytes apart in every load and store
template <bool DARK, bool FLAT>
__global__ __launch_bounds__(256) void k_cal_apply_x16(uint8_t *__restrict__ frames, size_t stride, const uint4 *__restrict__ dark,
                                                       const uint4 *__restrict__ gain, uint32_t groups, int black_d, int black, int top)
{
    uint4 *f = (uint4 *)(frames + (size_t)blockIdx.y * stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint4 a = f[g], b = f[(size_t)g + groups];
        uint4 ga = {}, gb = {}, da = {}, db = {};
        if (FLAT) { ga = gain[g]; gb = gain[(size_t)g + groups]; }
        if (DARK) { da = dark[g]; db = dark[(size_t)g + groups]; }
        else { a = clamp_px8(a, (uint32_t)top); b = clamp_px8(b, (uint32_t)top); }   // (with a dark frame its clamp does that)
        f[g] = cal_px8<DARK, FLAT>(a, da, ga, black_d, black, top);
        f[(size_t)g + groups] = cal_px8<DARK, FLAT>(b, db, gb, black_d, black, top);
    }
}

// dark, gain: nullptr for a stage that is off (not both).  64-bit products: 16-bit frames (65535 * 65535) and any black level a
// header may hold are exact.
__global__ __launch_bounds__(256) void k_cal_apply_generic(uint8_t *__restrict__ frames, size_t stride, const uint16_t *__restrict__ dark,
                                                           const uint16_t *__restrict__ gain, uint32_t npix, int black_d, int black, int top)
{
    uint16_t *f = (uint16_t *)(frames + (size_t)blockIdx.y * stride);
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x) {
        uint32_t px = f[k];
        px = dark ? cal_px<true, false>(px, dark[k], 0, black_d, 0, top) : min(px, (uint32_t)top);
        if (gain) px = cal_px<false, true, long long>(px, 0, gain[k], 0, black, top);
        f[k] = (uint16_t)px;
    }
}

template <int BPP, bool DARK, bool FLAT>
__global__ __launch_bounds__(256) void k_cal_unpack_x16(const uint8_t *__restrict__ packed, size_t packed_stride, uint8_t *__restrict__ out,
                                                        size_t out_stride, const uint4 *__restrict__ dark, const uint4 *__restrict__ gain,
                                                        uint32_t groups, int black_d, int black)
{
    constexpr int NW = BPP / 2;
    constexpr int top = (1 << BPP) - 1;
    const uint32_t *src = (const uint32_t *)(packed + (size_t)blockIdx.y * packed_stride);
    uint4 *dst = (uint4 *)(out + (size_t)blockIdx.y * out_stride);
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint32_t s[NW], px[16];
#pragma unroll
        for (int i = 0; i < NW; i++) s[i] = stream_word(src[(size_t)g * NW + i]);
        uint4 ga = {}, gb = {}, da = {}, db = {};
        if (FLAT) { ga = gain[(size_t)g * 2]; gb = gain[(size_t)g * 2 + 1]; }
        if (DARK) { da = dark[(size_t)g * 2]; db = dark[(size_t)g * 2 + 1]; }
        unpack_x16<BPP>(s, px);
        uint4 lo, hi;
        join_x16(px, lo, hi);
        dst[(size_t)g * 2] = cal_px8<DARK, FLAT>(lo, da, ga, black_d, black, top);
        dst[(size_t)g * 2 + 1] = cal_px8<DARK, FLAT>(hi, db, gb, black_d, black, top);
    }
}

// ---- the dark plane: the mean of a clip's frames ------------------------------------------------------------------------------
__device__ __forceinline__ void add_px8(uint4 (&s)[2], uint4 p)
{
    s[0].x += p.x & 0xFFFFu; s[0].y += p.x >> 16; s[0].z += p.y & 0xFFFFu; s[0].w += p.y >> 16;
    s[1].x += p.z & 0xFFFFu; s[1].y += p.z >> 16; s[1].z += p.w & 0xFFFFu; s[1].w += p.w >> 16;
}

// sums: one uint32 per pixel; the lane's 16 sums are four 128-bit words
__global__ __launch_bounds__(256) void k_dark_accum_x16(const uint8_t *__restrict__ frames, size_t stride, int nframes, uint4 *__restrict__ sums,
                                                        uint32_t groups)
{
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        uint4 lo[2], hi[2];
        lo[0] = sums[(size_t)g * 4];     lo[1] = sums[(size_t)g * 4 + 1];
        hi[0] = sums[(size_t)g * 4 + 2]; hi[1] = sums[(size_t)g * 4 + 3];
        for (int f = 0; f < nframes; f++) {
            const uint4 *src = (const uint4 *)(frames + (size_t)f * stride);
            add_px8(lo, src[(size_t)g * 2]);
            add_px8(hi, src[(size_t)g * 2 + 1]);
        }
        sums[(size_t)g * 4] = lo[0];     sums[(size_t)g * 4 + 1] = lo[1];
        sums[(size_t)g * 4 + 2] = hi[0]; sums[(size_t)g * 4 + 3] = hi[1];
    }
}

__global__ __launch_bounds__(256) void k_dark_accum_generic(const uint8_t *__restrict__ frames, size_t stride, int nframes,
                                                            uint32_t *__restrict__ sums, uint32_t npix)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x) {
        uint32_t s = sums[k];
        for (int f = 0; f < nframes; f++) s += ((const uint16_t *)(frames + (size_t)f * stride))[k];
        sums[k] = s;
    }
}

// n in 1..65536: sums[k] + n / 2 < 2^32
__global__ __launch_bounds__(256) void k_dark_mean(const uint32_t *__restrict__ sums, uint16_t *__restrict__ dark, uint32_t npix, uint32_t n)
{
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < npix; k += gridDim.x * blockDim.x)
        dark[k] = (uint16_t)((sums[k] + n / 2) / n);
}

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

// ---- the launchers ----------------------------------------------------------------------------------------------------------
static bool aligned16(const void *p) { return (uintptr_t)p % 16 == 0; }          // (a stage that is off: nullptr)

// what an x16 form asks of the descriptor: planes the library allocated itself are 16-byte aligned, and a gain's 32-bit products
static bool planes_x16(const Calib &cal)
{
    return aligned16(cal.d_dark) && aligned16(cal.d_gain) && (!cal.d_gain || (cal.top <= 32767 && cal.black >= 0 && cal.black <= 32767));
}

// the instantiation for the stages that are on (at least one is)
static auto apply_kernel(const Calib &cal)
{
    return cal.d_gain ? (cal.d_dark ? k_cal_apply_x16<true, true> : k_cal_apply_x16<false, true>) : k_cal_apply_x16<true, false>;
}

template <int BPP>
static auto unpack_kernel(const Calib &cal)
{
    return cal.d_gain ? (cal.d_dark ? k_cal_unpack_x16<BPP, true, true> : k_cal_unpack_x16<BPP, false, true>) : k_cal_unpack_x16<BPP, true, false>;
}

// in place; the callers have checked the geometry
int launch_cal_apply(void *d_frames, size_t stride, uint32_t npix, int nframes, const Calib &cal, hipStream_t stream)
{
    if (npix == 0 || nframes <= 0 || !cal.on()) return MLVFS_AMD_OK;
    const bool fast = npix % 16 == 0 && aligned16(d_frames) && planes_x16(cal) && (nframes == 1 || stride % 16 == 0);
    if (fast) {
        const uint32_t groups = npix / 16;
        hipLaunchKernelGGL(apply_kernel(cal), dim3(grid_x(groups, 8192), nframes), dim3(256), 0, stream, (uint8_t *)d_frames, stride,
                           (const uint4 *)cal.d_dark, (const uint4 *)cal.d_gain, groups, cal.black_d, cal.black, cal.top);
    } else {
        hipLaunchKernelGGL(k_cal_apply_generic, dim3(grid_x(npix, 16384), nframes), dim3(256), 0, stream, (uint8_t *)d_frames, stride, cal.d_dark,
                           cal.d_gain, npix, cal.black_d, cal.black, cal.top);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// packed payloads -> corrected 16-bit frames: one pass where k_unpack_x16 would run, else launch_unpack + launch_cal_apply
int launch_cal_unpack(const void *d_packed, size_t packed_stride, void *d_out, size_t out_stride, uint32_t npix, int bpp, int nframes,
                      const Calib &cal, hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    const bool fast = cal.on() && fast_depth(bpp) && cal.top == (1 << bpp) - 1 && planes_x16(cal) &&
                      fits_x16(npix, nframes, d_packed, packed_stride, 4, d_out, out_stride, 16);
    if (!fast) {
        if (int rc = launch_unpack(d_packed, packed_stride, d_out, out_stride, 0, npix, bpp, nframes, stream)) return rc;
        return launch_cal_apply(d_out, out_stride, npix, nframes, cal, stream);
    }
    const uint32_t groups = npix / 16;
    auto kern = bpp == 14 ? unpack_kernel<14>(cal) : (bpp == 12 ? unpack_kernel<12>(cal) : unpack_kernel<10>(cal));
    hipLaunchKernelGGL(kern, dim3(grid_x(groups, 8192), nframes), dim3(256), 0, stream, (const uint8_t *)d_packed, packed_stride, (uint8_t *)d_out,
                       out_stride, (const uint4 *)cal.d_dark, (const uint4 *)cal.d_gain, groups, cal.black_d, cal.black);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// d_sums: npix uint32, 16-byte aligned (the library's own allocation)
int launch_dark_accum(const void *d_frames, size_t stride, uint32_t npix, int nframes, uint32_t *d_sums, hipStream_t stream)
{
    if (npix == 0 || nframes <= 0) return MLVFS_AMD_OK;
    if (npix % 16 == 0 && aligned16(d_frames) && aligned16(d_sums) && (nframes == 1 || stride % 16 == 0)) {
        const uint32_t groups = npix / 16;
        hipLaunchKernelGGL(k_dark_accum_x16, dim3(grid_x(groups, 8192)), dim3(256), 0, stream, (const uint8_t *)d_frames, stride, nframes,
                           (uint4 *)d_sums, groups);
    } else {
        hipLaunchKernelGGL(k_dark_accum_generic, dim3(grid_x(npix, 16384)), dim3(256), 0, stream, (const uint8_t *)d_frames, stride, nframes,
                           d_sums, npix);
    }
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

int launch_dark_mean(const uint32_t *d_sums, uint16_t *d_dark, uint32_t npix, uint32_t n, hipStream_t stream)
{
    if (npix == 0) return MLVFS_AMD_OK;
    if (n < 1 || n > 65536) { set_error("dark: a mean of %u frames", n); return MLVFS_AMD_ERR_ARG; }
    hipLaunchKernelGGL(k_dark_mean, dim3(grid_x(npix, 16384)), dim3(256), 0, stream, d_sums, d_dark, npix, n);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

// d_plane, d_gain: the library's own allocations (16-byte aligned), npix values each; d_sums[4]: zeroed here; d_means[4]: the M_c
int launch_flat_gain(const uint16_t *d_plane, uint32_t w, uint32_t h, int black_f, unsigned long long *d_sums, uint16_t *d_gain,
                     uint32_t *d_means, hipStream_t stream)
{
    const uint32_t npix = w * h;
    if (npix == 0) return MLVFS_AMD_OK;
    MLV_HIP(hipMemsetAsync(d_sums, 0, 4 * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(k_flat_chan_sums, dim3(grid_x((npix + 15) / 16, 1024)), dim3(256), 0, stream, d_plane, npix, w, black_f, d_sums);
    MLV_HIP(hipGetLastError());
    FlatCounts counts;
    for (int c = 0; c < 4; c++) counts.n[c] = ((h + 1 - (uint32_t)(c >> 1)) / 2) * ((w + 1 - (uint32_t)(c & 1)) / 2);
    hipLaunchKernelGGL(k_flat_gain, dim3(grid_x((npix + 7) / 8, 8192)), dim3(256), 0, stream, d_plane, npix, w, black_f,
                       (const unsigned long long *)d_sums, counts, d_gain, d_means);
    MLV_HIP(hipGetLastError());
    return MLVFS_AMD_OK;
}

}  // namespace mlv

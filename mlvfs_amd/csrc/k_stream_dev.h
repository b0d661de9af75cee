// k_stream_dev.h -- the skeleton the two streaming kernels of the fused pass share (k_frame_p.hip: k_frame_p5, k_frame_s.hip: k_frame_s).
// A WAVE owns a column of the frame 62 items wide (an item = 4 cells = 8 x 2 pixels, one per lane; lanes 0 and 63 hold the halo items
// whose neighbouring cells the outermost output items need) and walks down it one cell row per step, two rows of stream words under
// way; waves draw their tasks (frame, column, segment of seg_rows rows) from one ticket counter, and the last wave out zeroes it.
// The pieces take values, not FrameArgs: k_frame_p5 reads its arguments through cold_args() where it uses them, k_frame_s reads them
// directly -- that difference is what keeps either kernel's scalar registers where they are.  What differs stays in the kernels: the
// window of rows (and where a row's pixels wait for their medians), the warm-up depth, the reference, pixel maps and the work list.
// So do two scalars of a task, the x of lane 0's item and whether the column touches a margin (stream_output's tx0 and xm): decoded
// with the rest, ahead of the kernel's buffer descriptors, the compiler re-associates x = tx0 + 8 lane + 2 cell and k_frame_p5 pays
// one more vector instruction per task.
#pragma once
#include "k_frame_dev.h"

namespace mlv {

// Tasks per frame.  fold > 1: the frame's last column is at most 64 / fold - 2 items wide and a wave takes `fold` of its segments at
// once, one per group of 64 / fold lanes (each with its own two halo lanes): 3584 px = 7 columns of 62 items and one of 14 -- 7.25
// columns' worth of steps instead of 8
struct StreamGrid { int ncols_full, nfolded, per_frame; };
__device__ __forceinline__ StreamGrid stream_grid(int cols, int segs, int fold)
{
    StreamGrid sg;
    sg.ncols_full = fold > 1 ? cols - 1 : cols;
    sg.nfolded = fold > 1 ? (segs + fold - 1) / fold : 0;
    sg.per_frame = sg.ncols_full * segs + sg.nfolded;
    return sg;
}

// the wave's next ticket (scalar)
__device__ __forceinline__ int stream_draw(int *tickets, int lane)
{
    int task = 0;
    if (lane == 0) task = atomicAdd(&tickets[0], 1);
    return __builtin_amdgcn_readfirstlane(task);
}

// What a ticket stands for.  S_OUT: items a wave writes per row (frame_plan.h: FRAME_STREAM_COLW); rows = h / 2.
struct StreamTask {
    int f, c;                // frame, column
    int j0, j1;              // cell rows [j0, j1) (of the first group of lanes; the others lie roff rows further down)
    int nparts, P;           // a folded last column: groups of P lanes, each a segment of its own
    int pl, part, roff;      // the lane within its group, its group, the group's row offset
    int g;                   // the lane's 8-pixel group; lanes outside the frame (the halo lanes of the first and last column, the lanes
                             // behind a narrow last column) take a group inside it: their values are never used, and never "dark"
    bool writes;
    uint32_t gbyte;          // byte offset of the group within a pixel row
    uint32_t sel, sel1;      // unpack selectors of the even and the odd pixel row (the group starts in the lower / upper half of a dword)
};
// VEC = 1: rows of whole 16-pixel groups (every row starts dword-aligned); VEC = 2: w % 16 == 8 (odd pixel rows start two bytes into a
// dword: their groups' alignment is the other way round -- the selectors flip, as in k_frame's loader)
template <int VEC>
__device__ __forceinline__ StreamTask stream_task(int task, const StreamGrid &sg, int segs, int seg_rows, int fold, int S_OUT, int lane, int w, int rows)
{
    StreamTask t;
    const int gmax = (w >> 3) - 1;
    t.f = task / sg.per_frame;
    const int rem = task - t.f * sg.per_frame;
    const bool folded = rem >= sg.ncols_full * segs;
    t.c = folded ? sg.ncols_full : rem / segs;
    const int seg = folded ? (rem - sg.ncols_full * segs) * fold : rem - t.c * segs;
    t.j0 = seg * seg_rows; t.j1 = min(t.j0 + seg_rows, rows);
    t.nparts = folded ? fold : 1; t.P = folded ? 64 / fold : 64;
    t.pl = lane & (t.P - 1); t.part = folded ? lane / t.P : 0;
    t.roff = t.part * seg_rows;
    const int g_true = t.c * S_OUT + t.pl - 1;
    t.g = min(max(g_true, 0), gmax);
    t.writes = t.pl >= 1 && t.pl <= min(S_OUT, t.P - 2) && g_true <= gmax && t.j0 + t.roff < rows;
    t.gbyte = (uint32_t)t.g * 14u;
    t.sel = (t.g & 1) ? SEL_MIS : SEL_SWAP;
    t.sel1 = VEC == 2 ? t.sel ^ (SEL_SWAP ^ SEL_MIS) : t.sel;
    return t;
}

// the stream words of cell row r (14-bit, pitch bytes per pixel row): four range-checked 8-byte loads at the clamped row (rows above /
// below the frame are never used either)
__device__ __forceinline__ void stream_issue(mlv_i32x4 rs_in, int r, int roff, int rows, uint32_t pitch, uint32_t gbyte, uint32_t (&d0)[4], uint32_t (&d1)[4])
{
    const int rr = min(max(r + roff, 0), rows - 1);
    const uint32_t o0u = __umul24((uint32_t)(2 * rr), pitch) + gbyte, o0 = o0u & ~3u, o1 = (o0u + pitch) & ~3u;
    const mlv_u32x2 a0 = mlv_rbl_x2(rs_in, (int)o0, 0, AUX_DEFAULT), b0 = mlv_rbl_x2(rs_in, (int)o0 + 8, 0, AUX_DEFAULT);
    const mlv_u32x2 a1 = mlv_rbl_x2(rs_in, (int)o1, 0, AUX_DEFAULT), b1 = mlv_rbl_x2(rs_in, (int)o1 + 8, 0, AUX_DEFAULT);
    d0[0] = a0.x; d0[1] = a0.y; d0[2] = b0.x; d0[3] = b0.y;
    d1[0] = a1.x; d1[1] = a1.y; d1[2] = b1.x; d1[3] = b1.y;
}

// the low pixels of a row, wave-wide.  dark: some pixel at or below black (the row takes the loader's second form); the flag: bit 0 = a
// pixel at most 64 above black, bit 1 = less than 256 above
__device__ __forceinline__ int stream_row_low(const uint32_t (&p0)[8], const uint32_t (&p1)[8], int black, bool &dark)
{
    uint32_t lo = min(p0[0], p1[0]);
#pragma unroll
    for (int i = 1; i < 8; i++) lo = min(min(lo, p0[i]), p1[i]);
    dark = __any((int)lo <= black);
    int fl = 0;
    if (__any((int)lo <= black + 255)) fl = __any((int)lo <= black + 64) ? 3 : 2;
    return fl;
}

// k_frame's output stage on registers for row jr (top / bot: the row's pixels), then its two 16-byte stores.  tx0: x of lane 0's item,
// 8 * (t.c * S_OUT - 1); xm: the column touches the frame's left or right margin, t.c == 0 || 8 * (t.c * S_OUT + S_OUT) > w - 4.  fl: the
// flags of the rows of the window; what smoothing makes of them is added here (smoothed_low).  The variants of strip_output_t are
// chosen by scalars: margins, low pixels, bright rows.
struct StreamNoHook { __device__ __forceinline__ void operator()() const {} };
template <int METHOD, class BEFORE_STORES = StreamNoHook>
__device__ __forceinline__ void stream_output(const OutArgs &oa, const StreamTask &t, int tx0, bool xm, mlv_i32x4 rs_out, int w, int h, int black, int jr, int yl,
                                              unsigned long long msmooth, int fl, const int (&ge)[STRIP], const int (&er)[STRIP], const int (&eb)[STRIP],
                                              uint32_t (&top)[STRIP], uint32_t (&bot)[STRIP], BEFORE_STORES before_stores = BEFORE_STORES())
{
    fl |= oa.stripes && smoothed_low(er, eb) ? 1 : 0;
    auto out = [&](auto CLAMP, auto XM, auto BRIGHT) {
        strip_output_t<METHOD, true, true, CLAMP.value, XM.value, false, BRIGHT.value, NoSmem, true>(NoSmem(), oa, w, h, black, t.f, tx0, 0, jr, t.pl, msmooth,
                                                                                                     ge, 0, er, eb, false, top, bot);
    };
    constexpr std::true_type Y{};
    constexpr std::false_type N{};
    if (fl & 1) { if (xm) out(Y, Y, N); else out(Y, N, N); }
    else if (xm) out(N, Y, N);
    else if (fl == 0) out(N, N, Y);
    else out(N, N, N);
    before_stores();
    if (t.writes) {
        const uint32_t vo = (__umul24((uint32_t)yl, (uint32_t)w) + (uint32_t)(8 * t.g)) * 2u;     // (rows below the frame: beyond the buffer's range)
        const mlv_u32x4 vt = { top[0], top[1], top[2], top[3] }, vb = { bot[0], bot[1], bot[2], bot[3] };
        mlv_rbs_x4(vt, rs_out, (int)vo, 0, 2);                                                     // (2: non-temporal)
        mlv_rbs_x4(vb, rs_out, (int)vo, w * 2, 2);
    }
}

// The last wave out leaves the two counters as it found them (the next launch on this stream starts from zero), then does `after`
// (its lane 0 only).  waves_per_wg: of the kernel's workgroups (k_frame_s: 4, k_frame_p5: 16).
template <class AFTER>
__device__ __forceinline__ void stream_last_out(int *tickets, int lane, int waves_per_wg, AFTER after)
{
    if (lane == 0) {
        const int nwaves = (int)gridDim.x * waves_per_wg;
        if (atomicAdd(&tickets[1], 1) == nwaves - 1) {
            tickets[0] = 0; tickets[1] = 0;
            after();
        }
    }
}

}  // namespace mlv

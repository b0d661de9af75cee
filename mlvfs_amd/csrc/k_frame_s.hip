// k_frame_s.hip -- the fused pass for cs2x2 and cs3x3 (chroma_smooth.c:22-71 with CHROMA_SMOOTH_2X2 / _3X3: the plus-shaped five, the
// nine) as a STREAMING kernel without barriers and without planes in LDS (round 5, end).
//
// k_frame's cs2x2 instantiation executes 5 % fewer instructions than it did and takes the same time: its time is the
// dependent chain of a tile -- prefetched words -> unpack -> table gathers -> barrier -> medians -> look-ups -> stores -> barrier --
// at four workgroups per CU.  A plus-shaped window needs one cell to the left and right and one row above and below, nothing a
// workgroup has to share through LDS:
//   * a WAVE owns a column of the frame 62 items wide (an item = 4 cells = 8 x 2 pixels, one per lane; lanes 0 and 63 hold the
//     halo items whose neighbouring cell the outermost output items need) and walks down it one cell row per step;
//   * the colour differences of the row above and the row being loaded stay in registers (the stencil's vertical taps), the
//     horizontal taps of a lane's outer cells come from the neighbouring lanes (v_mov_b32_dpp wave_shr / wave_shl);
//   * a step unpacks and converts row r, then finishes row r - 1: medians, look-ups, R / B replacement, stripes, two 16-byte stores;
//     the words of rows r + 1 and r + 2 are under way meanwhile (one row ahead: 6.7 us per frame, two: 4.75);
//   * no s_barrier after the table is in LDS, 16 KiB of LDS per workgroup (the raw2ev table), 126 VGPRs: four workgroups per CU
//     (what the kernel is compiled for: <= 128 VGPRs);
//   * waves draw their tasks (frame, column, 60 rows) from one counter; the last wave out zeroes it for the next launch.
// Same arithmetic as k_frame: the loader's cell functions, mlv_median5, strip_output_t (k_frame_dev.h) -- results identical.
// Measured and not kept (profiles/r05/ab_kframe_s.log; DESIGN_HISTORY.md, round 5): compiled for five workgroups per CU (<= 96 VGPRs:
// 14-43 spilled, 6.7-10.5 us per frame against 4.75); a row's pixels waiting for their medians in the wave's own 4 KiB of LDS instead
// of in registers (no gain), and with them parked a third row of prefetch, which does not fit 128 registers otherwise (+-0); the cells
// of a row converted two at a time instead of all four; a form that finishes row r - 2 while row r's table look-ups are under way, so
// that neither wait is exposed (186 VGPRs: the in-flight conversion, three rows of colour differences, the medians' operands and two
// sets of look-ups do not fit four waves per SIMD).
// What it takes: 14-bit streams whose rows are whole 8-pixel groups (on the buffers the vector path wants), even heights, no pixel
// map, stripes in the packed 16-bit form (or none), black >= 0.  Everything else stays with k_frame (frame_plan.cpp).
#include "frame_plan.h"
#include "k_stream_dev.h"

namespace mlv {

// VEC: k_stream_dev.h (stream_task).
// METHOD = 2: the plus-shaped five; METHOD = 3: the 3x3 nine (chroma_smooth.c with CHROMA_SMOOTH_3X3) -- the same rows in registers,
// sorted columns of three (k_frame_dev.h: strip_median9's scheme), the neighbouring lanes' edge columns by DPP
template <bool SPREAD, int VEC, int METHOD>
__global__ __launch_bounds__(256, 4) void k_frame_s(const FrameArgs a, int cols, int segs, int seg_rows, int fold, int S_OUT)
{
    constexpr int BPP = 14;
    __shared__ __align__(16) uint16_t t16[MLV_T16_N + (SPREAD ? 64 : 0)];
    load_t16_rel<SPREAD>(t16, a.t16, (int)threadIdx.x);
    __syncthreads();                                     // the only barrier: from here on the waves are on their own
    const int lane = (int)threadIdx.x & 63;
    const int w = a.w, h = a.h, black = a.black;
    const int rows = h >> 1;
    const StreamGrid sg = stream_grid(cols, segs, fold);          // (the folded last column: k_stream_dev.h)
    const int ntasks = a.nframes * sg.per_frame;
    const uint32_t pitch = (uint32_t)(w >> 3) * 14u;     // bytes per pixel row (VEC 1: a multiple of 28, rows start dword-aligned)
    const OutArgs oa = out_args(cold_args());
    int *tickets = a.tickets;
    for (;;) {
        const int task = stream_draw(tickets, lane);
        if (task >= ntasks) break;
        const StreamTask t = stream_task<VEC>(task, sg, segs, seg_rows, fold, S_OUT, lane, w, rows);
        const int f = t.f, j0 = t.j0, j1 = t.j1, roff = t.roff;
        const mlv_i32x4 rs_in = frame_rsrc(a.src + (size_t)f * a.src_stride, a.src_bytes);
        const mlv_i32x4 rs_out = frame_rsrc(oa.dst + (size_t)f * oa.dst_stride, (uint32_t)w * (uint32_t)h * 2u);
        const int tx0 = 8 * (t.c * S_OUT - 1);           // x of lane 0's item
        const bool xm = t.c == 0 || 8 * (t.c * S_OUT + S_OUT) > w - 4;      // the column touches the frame's left or right margin

        uint32_t dA0[4], dA1[4], dB0[4], dB1[4];         // two rows under way
        auto issue = [&](int r, uint32_t (&d0)[4], uint32_t (&d1)[4]) { stream_issue(rs_in, r, roff, rows, pitch, t.gbyte, d0, d1); };
        // rows r - 2 (colour differences only) and r - 1 (everything: it is finished when row r is in)
        int dr2[STRIP] = { 0, 0, 0, 0 }, db2[STRIP] = { 0, 0, 0, 0 };
        int dr1[STRIP] = { 0, 0, 0, 0 }, db1[STRIP] = { 0, 0, 0, 0 }, ge1[STRIP] = { 0, 0, 0, 0 };
        uint32_t top1[STRIP] = { 0, 0, 0, 0 }, bot1[STRIP] = { 0, 0, 0, 0 };
        int flags1 = 3, flags2 = 3;                      // bit 0: a pixel at most 64 above black, bit 1: less than 256 above (rows r - 1, r - 2)
        int dark_steps = 0;
        issue(j0 - 1, dA0, dA1);
        issue(j0, dB0, dB1);
        auto step = [&](int r, uint32_t (&d0)[4], uint32_t (&d1)[4]) {
            uint32_t p0[8], p1[8];
            unpack8<BPP>(d0, t.sel, t.sel, t.sel, p0);
            unpack8<BPP>(d1, t.sel1, t.sel1, t.sel1, p1);
            if (r + 2 <= j1) issue(r + 2, d0, d1);       // the row this set is needed for next goes out while this one is converted
            bool dark;
            const int flags0 = stream_row_low(p0, p1, black, dark);
            dark_steps += dark ? 1 : 0;
            int ge[STRIP], dr[STRIP], db[STRIP];
            if (!dark) cell_multi_ev_fast<4, SPREAD>(p0, p1, black, t16, ge, dr, db);       // (four cells: their table look-ups in flight together)
            else {
#pragma unroll
                for (int cc = 0; cc < 4; cc += 2) {
                    int g2[2], r2[2], b2[2];
                    cell_multi_ev_dark<2, SPREAD>(p0 + 2 * cc, p1 + 2 * cc, black, t16, g2, r2, b2);
                    ge[cc] = g2[0]; ge[cc + 1] = g2[1]; dr[cc] = r2[0]; dr[cc + 1] = r2[1]; db[cc] = b2[0]; db[cc + 1] = b2[1];
                }
            }
            uint32_t top[STRIP], bot[STRIP];
#pragma unroll
            for (int cc = 0; cc < STRIP; cc++) { top[cc] = p0[2 * cc] | (p0[2 * cc + 1] << 16); bot[cc] = p1[2 * cc] | (p1[2 * cc + 1] << 16); }
            if (r - 1 >= j0) {
                // ---- row r - 1: medians of the plus-shaped five, then k_frame's output stage on registers
                const int jr = r - 1, y = 2 * jr, yl = y + 2 * roff;
                const bool smooth_row = y + 2 * (t.nparts - 1) * seg_rows >= 4 && y < h - 5;     // chroma_smooth.c:25 (scalar: some group's row)
                int er[STRIP] = { 0, 0, 0, 0 }, eb[STRIP] = { 0, 0, 0, 0 };
                if (smooth_row && METHOD == 2) {
                    const int lr = dpp_prev_i(dr1[3]), lb = dpp_prev_i(db1[3]);                // the cell left of cell 0: the lane before's last
                    const int rr_ = dpp_next_i(dr1[0]), rb = dpp_next_i(db1[0]);               // the cell right of cell 3: the next lane's first
#pragma unroll
                    for (int cc = 0; cc < STRIP; cc++) {
                        const int vr[5] = { dr2[cc], cc ? dr1[cc - 1] : lr, dr1[cc], cc < 3 ? dr1[cc + 1] : rr_, dr[cc] };
                        const int vb[5] = { db2[cc], cc ? db1[cc - 1] : lb, db1[cc], cc < 3 ? db1[cc + 1] : rb, db[cc] };
                        int o[1];
                        mlv_median5(vr, o); er[cc] = wadd(ge1[cc], o[0]);
                        mlv_median5(vb, o); eb[cc] = wadd(ge1[cc], o[0]);
                    }
                }
                if (smooth_row && METHOD == 3) {
                    // columns of three (rows r - 2, r - 1, r) sorted once; the lane before's last column and the next lane's first by DPP
                    auto med9 = [&](const int (&up)[STRIP], const int (&mid)[STRIP], const int (&dn)[STRIP], int (&e)[STRIP]) {
                        int lo[STRIP + 2], mi[STRIP + 2], hi[STRIP + 2];
#pragma unroll
                        for (int cc = 0; cc < STRIP; cc++) {
                            lo[cc + 1] = min(min(up[cc], mid[cc]), dn[cc]);
                            hi[cc + 1] = max(max(up[cc], mid[cc]), dn[cc]);
                            mi[cc + 1] = med3i(up[cc], mid[cc], dn[cc]);
                        }
                        lo[0] = dpp_prev_i(lo[STRIP]); mi[0] = dpp_prev_i(mi[STRIP]); hi[0] = dpp_prev_i(hi[STRIP]);
                        lo[STRIP + 1] = dpp_next_i(lo[1]); mi[STRIP + 1] = dpp_next_i(mi[1]); hi[STRIP + 1] = dpp_next_i(hi[1]);
#pragma unroll
                        for (int cc = 0; cc < STRIP; cc++)
                            e[cc] = wadd(ge1[cc], med3i(max(max(lo[cc], lo[cc + 1]), lo[cc + 2]), med3i(mi[cc], mi[cc + 1], mi[cc + 2]),
                                                         min(min(hi[cc], hi[cc + 1]), hi[cc + 2])));
                    };
                    med9(dr2, dr1, dr, er);
                    med9(db2, db1, db, eb);
                }
                const unsigned long long msmooth = lanes_ge(yl, 4) & lanes_lt(yl, h - 5);       // (a lane mask in a register pair: put_rb moves it to VCC)
                // (the three rows loaded; stream_output adds what smoothing makes of them)
                stream_output<METHOD>(oa, t, tx0, xm, rs_out, w, h, black, jr, yl, msmooth, flags0 | flags1 | flags2, ge1, er, eb, top1, bot1);
            }
#pragma unroll
            for (int cc = 0; cc < STRIP; cc++) {
                dr2[cc] = dr1[cc]; db2[cc] = db1[cc];
                dr1[cc] = dr[cc]; db1[cc] = db[cc]; ge1[cc] = ge[cc];
                top1[cc] = top[cc]; bot1[cc] = bot[cc];
            }
            flags2 = flags1; flags1 = flags0;
        };
        for (int r = j0 - 1; r <= j1; r += 2) {
            step(r, dA0, dA1);
            if (r + 1 <= j1) step(r + 1, dB0, dB1);
        }
        if (lane == 0 && dark_steps) atomicAdd(&a.wl_ctl[0], dark_steps);       // (what the host's choice of kernel for this stream looks at)
    }
    stream_last_out(tickets, lane, 4, [&] { if (a.wl_stat) { __atomic_store_n(a.wl_stat, a.wl_ctl[0], __ATOMIC_RELAXED); __threadfence_system(); } });
}

// k_frame_s as the plan lays it out (frame_plan.cpp: which launches it takes, its grid and tasks)
void launch_frame_s(const FramePlan &pl, int method, int vec, bool spread, hipStream_t stream, const FrameArgs &a)
{
    with_layout(method, true, vec, spread, [&](auto M, auto P, auto V, auto S) {
        if constexpr ((M.value == 2 || M.value == 3) && P.value && (V.value == 1 || V.value == 2))
            hipLaunchKernelGGL((k_frame_s<S.value, V.value, M.value>), dim3(pl.first_grid), dim3(256), 0, stream, a, pl.cols, pl.segs, pl.seg_rows,
                               pl.fold, FRAME_STREAM_COLW);
    });
}

void preload_k_frame_s() { hipFuncAttributes fa; (void)hipFuncGetAttributes(&fa, (const void *)k_frame_s<false, 1, 2>); (void)hipGetLastError(); }

}  // namespace mlv

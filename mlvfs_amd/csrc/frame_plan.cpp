// frame_plan.cpp -- the fused pass's choice of kernels and their launch geometry (frame_plan.h), host arithmetic only.
//   k_frame     the tile kernel (k_frame.hip): every launch the others do not take; in list mode, what k_frame_p / k_frame_p5 listed
//   k_frame_p   cs5x5 on the vector layouts, packed medians once per tile (k_frame_p.hip)
//   k_frame_p5  the same as a streaming kernel: long launches of 14-bit streams (k_frame_p.hip)
//   k_frame_s   cs2x2 / cs3x3 as a streaming kernel, alone: long launches of 14-bit streams without a pixel map (k_frame_s.hip)
#include "frame_plan.h"

#include "clip.h"

namespace mlv {

namespace {
constexpr int WGS_PER_CU = 4;      // every kernel of the pass: four workgroups of four waves per CU (their __launch_bounds__; k_frame_p5
                                   // takes the same sixteen waves as ONE workgroup: launch_frame_p launches first_grid / 4 of them)
constexpr int RUN_MAX = 22;        // k_frame: tiles per run at most
constexpr int P5_SEG = 60;         // k_frame_p5: rows per task (or half as many for launches half as long)
constexpr int S_SEG = 60;          // k_frame_s: rows per task

int cus(const FramePassInputs &in) { return in.num_cu > 0 ? in.num_cu : 256; }

int env_switch(const char *name) { const char *e = getenv(name); return e ? atoi(e) : 1; }

// what the streaming kernels read: 14-bit streams in rows of whole 8-pixel groups (the vector layouts), even heights, a black level
// of 0 .. 16384 (the range in which launch_frame admits the packed stripes form; above it the reference has no raw2ev table and
// smooths nothing: main.c:171-175), stripes in the packed 16-bit form or none
bool streamable(const FramePassInputs &in)
{
    return in.packed && in.bpp == 14 && (in.vec == 1 || in.vec == 2) && in.black >= 0 && in.black <= 16384 && in.stripes != StripeForm::generic &&
           in.w >= 16 && in.w % 8 == 0 && in.h >= 2 && in.h % 2 == 0;
}

// Does k_frame_s take the launch?  Long launches only: a task is a column of 60 rows (~50 us of one wave), and a wave needs a handful
// of them for the chip to end together -- 3584x1320, us per frame at 8 / 25 / 50 / 100 / 200 / 400 frames per launch: k_frame 10.7 /
// 5.7 / 5.7 / 5.5 / 5.3 / 4.9, k_frame_s 13.1 / 7.3 / 7.1 / 5.5 / 5.0 / 4.8 (shorter tasks do not help: two rows of warm-up each;
// profiles/r05/ab_kframe_s.log).
bool s_takes(const FramePassInputs &in, const FrameSwitches &sw)
{
    if ((in.method != 2 && in.method != 3) || sw.s == 0 || in.pixel_map || !streamable(in)) return false;
    const StreamGeom g = stream_geom(in.w, in.h, S_SEG);
    const long long waves = (long long)cus(in) * WGS_PER_CU * 4;
    return sw.s == 2 || (long long)in.nframes * g.cols * g.segs * 2 >= waves * 7;               // >= 3.5 tasks per wave
}

// k_frame_p5's rows per task, 0: k_frame_p does the launch.  At least 3.5 tasks per wave, in tasks of 60 rows or, for launches half
// as long, of 30 (two warm-up rows per task: 3584x1320, us per frame at 50 / 100 / 200 / 400 frames per launch: k_frame_p 7.7 / 7.4
// / 7.1 / 6.9, tasks of 60 rows 8.3 / 7.4 / 6.6 / 6.1, of 30 rows 8.6 / 6.9 / 6.7 / 6.2; profiles/r05/ab_p5.log).  The CU count is
// k_frame's grid / 4, on whose grid it runs.
int p5_seg_rows(const FramePassInputs &in, const FrameSwitches &sw, int grid)
{
    if (in.method != 5 || sw.p5 == 0 || !streamable(in)) return 0;
    const long long cols = stream_geom(in.w, in.h, P5_SEG).cols, rows = in.h / 2;
    const long long waves = (long long)(grid / 4 > 0 ? grid / 4 : 256) * 16;
    for (int seg : { P5_SEG, P5_SEG / 2 })
        if ((long long)in.nframes * cols * ((rows + seg - 1) / seg) * 2 >= waves * 7) return seg;
    return sw.p5 == 2 ? P5_SEG / 2 : 0;
}

// tile columns that n consecutive cells can touch
int tile_cols_spanned(int n) { return (n + FRAME_TCW - 2) / FRAME_TCW + 1; }
}  // namespace

FrameSwitches frame_switches() { return FrameSwitches{ env_switch("MLVFS_AMD_KF_P"), env_switch("MLVFS_AMD_KF_P5"), env_switch("MLVFS_AMD_KF_S") }; }

StreamGeom stream_geom(int w, int h, int seg_rows)
{
    StreamGeom g;
    g.cols = (w / 8 + FRAME_STREAM_COLW - 1) / FRAME_STREAM_COLW;
    g.segs = (h / 2 + seg_rows - 1) / seg_rows;
    const int last_items = w / 8 - (g.cols - 1) * FRAME_STREAM_COLW;
    g.fold = g.segs < 2 ? 1 : last_items + 2 <= 16 ? 4 : last_items + 2 <= 32 ? 2 : 1;
    g.tasks_per_frame = g.fold > 1 ? (g.cols - 1) * g.segs + (g.segs + g.fold - 1) / g.fold : g.cols * g.segs;
    return g;
}

FrameWatch frame_pass_watch(const FramePassInputs &in, const FrameSwitches &sw)
{
    FrameWatch wt;
    // (k_frame_s takes cs2x2 / cs3x3, k_frame_p and k_frame_p5 cs5x5: at most one of the two words is watched)
    if (s_takes(in, sw)) { wt.word = 1; wt.adaptive = sw.s == 1; wt.status = wt.adaptive; }
    else if (in.method == 5 && in.vec != 0 && sw.p != 0) { wt.word = 0; wt.adaptive = sw.p == 1; wt.status = true; }
    return wt;
}

int check_frame_pass(const FramePassInputs &in)
{
    if (in.method != 0 && in.method != 2 && in.method != 3 && in.method != 5) set_error("Unsupported chroma smooth method %d", in.method);
    else if (in.nframes <= 0 || in.vec < 0 || in.vec > 4) set_error("fused pass: %d frames, layout %d", in.nframes, in.vec);
    else if ((long long)frame_tiles_x(in.w) * frame_tiles_y(in.h, frame_geo_of(in.method)) * in.nframes >= (1ll << 30))
        set_error("too many tiles in one launch (%d frames): split the batch", in.nframes);
    else if (in.w < 2 || in.h < 2 || (in.w & 1) || (long long)in.w * in.h >= (1ll << 28))     // 32-bit bit / byte offsets inside a frame
        set_error("frame geometry %dx%d unsupported", in.w, in.h);
    else return MLVFS_AMD_OK;
    return MLVFS_AMD_ERR_ARG;
}

int plan_frame_pass(const FramePassInputs &in, const FrameSwitches &sw, const StreamVerdict &v, FramePlan *out)
{
    if (const int rc = check_frame_pass(in)) return rc;
    FramePlan p;
    const int tiles_x = frame_tiles_x(in.w);
    p.tiles = (long long)tiles_x * frame_tiles_y(in.h, frame_geo_of(in.method)) * in.nframes;

    // k_frame: four workgroups per CU (39 KiB of LDS, <= 128 VGPRs), a multiple of 8 (one XCD each), no more than the tiles
    p.grid = (cus(in) * WGS_PER_CU + 7) / 8 * 8;
    if (p.grid > p.tiles) p.grid = (int)((p.tiles + 7) / 8 * 8);
    // Groups: workgroups that draw from one range of the tile list.  Until round 4 a group was one CU's four residents; the CUs of a
    // chip do not run at one speed (their workgroups ended between 780 and 835 us of an 844-us launch: 5.5 % of the launch was its
    // tail), and drawing runs instead of single tiles made the atomics rare enough for larger groups: eight CUs (a quarter of an XCD:
    // blocks b, b + groups, ... share b % 8, i.e. their XCD, as long as groups is a multiple of 8) share a range, 123.0 -> 128.4 k fps;
    // 16 / 24 / 32 / 64 groups and runs of 11 / 22 / 44 tiles are within 0.5 % of each other, one group per XCD (8) loses the gain to
    // its 1 408 single tiles (profiles/r04/ab_groups.log).
    const int per_cu = std::min(std::max(p.grid / 4, 1), FRAME_MAX_GROUPS);
    p.groups = per_cu >= 64 ? per_cu / 8 / 8 * 8 : per_cu;
    // tiles per run: at most half a column of the benchmark's geometry (same-box sweep with one CU per group: 4 / 8 / 11 / 22 / 44
    // tiles per run -> 117.2 / 117.5 / 117.7 / 118.0-121.0 / 120.5 k fps), a sixteenth of the range for short launches; the last
    // eight tiles per workgroup of a group's range go out one by one
    const int band = (int)(p.tiles / p.groups);
    p.run = std::min(std::max(band / 16, 1), RUN_MAX);
    p.singles = p.run > 1 ? 8 * std::max(p.grid / p.groups, 1) : 0;

    p.watch = frame_pass_watch(in, sw);
    const bool held = p.watch.adaptive && v.held;
    if (p.watch.word == 1 && !held) {
        p.first = FirstKernel::s;
        p.seg_rows = S_SEG;
    } else if (p.watch.word == 0 && !held) {
        p.list_after = true;
        p.seg_rows = v.some_listed && sw.p5 != 2 ? 0 : p5_seg_rows(in, sw, p.grid);
        p.first = p.seg_rows ? FirstKernel::p5 : FirstKernel::p;
        p.first_grid = p.grid;                                   // (k_frame_p5 too runs on k_frame's tile grid)
    }
    if (p.seg_rows) {
        const StreamGeom g = stream_geom(in.w, in.h, p.seg_rows);
        p.cols = g.cols; p.segs = g.segs; p.fold = g.fold;
        p.tasks = (long long)in.nframes * g.tasks_per_frame;
    }
    if (p.first == FirstKernel::s) {
        p.first_grid = cus(in) * WGS_PER_CU;
        if ((long long)p.first_grid * 4 > p.tasks) p.first_grid = (int)((p.tasks + 3) / 4);
        p.steps = (long long)in.nframes * ((p.cols - 1) * p.fold + 1) * (in.h / 2) / p.fold;
    }
    if (p.list_after) {
        // k_frame_p lists at most every tile once.  k_frame_p5 appends, per task and part of a folded task, one entry for each tile
        // column that the lanes of the part with uncertain strips span (k_frame_p.hip, the end of a task): 256 consecutive cells, or
        // 256 / fold -- more than the frame's tiles where a frame is one tile row high.
        long long most = p.tiles;
        if (p.first == FirstKernel::p5) {
            const int full_cols = p.fold > 1 ? p.cols - 1 : p.cols, folded = p.fold > 1 ? (p.segs + p.fold - 1) / p.fold : 0;
            const long long per_frame = (long long)full_cols * p.segs * std::min(tiles_x, tile_cols_spanned(4 * 64)) +
                                        (long long)folded * p.fold * std::min(tiles_x, tile_cols_spanned(4 * 64 / p.fold));
            most = std::max(most, in.nframes * per_frame);
        }
        p.wl_entries = std::max(most, 4096ll);
    }
    *out = p;
    return MLVFS_AMD_OK;
}

namespace {
struct LastPlan { FramePlan plan; bool set = false; };
LastPlan &last_plan() { static thread_local LastPlan t; return t; }

// a plan as the 15 fields of the test hooks (include/mlvfs_amd.h: mlvfs_amd_test_frame_plan)
void plan_fields(const FramePlan &p, long long *out)
{
    const long long o[15] = { (long long)p.first, p.list_after, p.grid, p.groups, p.run, p.singles, p.first_grid,
                              p.seg_rows, p.cols, p.segs, p.fold, p.tasks, p.steps, p.wl_entries, p.watch.word };
    for (int i = 0; i < 15; i++) out[i] = o[i];
}
}  // namespace

void record_frame_plan(const FramePlan &p) { LastPlan &l = last_plan(); l.plan = p; l.set = true; }

}  // namespace mlv

// Test hook, host only (no GPU): how the streaming kernels cut a frame of width x height pixels into tasks of seg_rows cell rows
// (stream_geom).  0, or MLVFS_AMD_ERR_ARG for a frame the kernels do not take.
extern "C" int mlvfs_amd_test_stream_plan(int width, int height, int seg_rows, int *cols, int *segs, int *fold, int *tasks_per_frame)
{
    if (width < 16 || width % 8 || height < 2 || height % 2 || seg_rows < 1 || !cols || !segs || !fold || !tasks_per_frame) return MLVFS_AMD_ERR_ARG;
    const mlv::StreamGeom g = mlv::stream_geom(width, height, seg_rows);
    *cols = g.cols; *segs = g.segs; *fold = g.fold; *tasks_per_frame = g.tasks_per_frame;
    return MLVFS_AMD_OK;
}

// Test hook, host only (no GPU): the plan of one launch (include/mlvfs_amd.h), the switches read as a launch reads them
extern "C" int mlvfs_amd_test_frame_plan(const int *in, long long *out)
{
    if (!in || !out) return MLVFS_AMD_ERR_ARG;
    const mlv::FramePassInputs fi{ in[0], in[1], in[2], in[3], in[4], in[5] != 0, in[6], in[7] != 0,
                                   in[8] == 2 ? mlv::StripeForm::generic : in[8] == 1 ? mlv::StripeForm::packed : mlv::StripeForm::none,
                                   in[9], in[10] };
    const mlv::StreamVerdict v{ in[11] != 0, in[12] != 0 };
    mlv::FramePlan p;
    if (const int rc = mlv::plan_frame_pass(fi, mlv::frame_switches(), v, &p)) return rc;
    mlv::plan_fields(p, out);
    return MLVFS_AMD_OK;
}

// Test hook: what the finished launches on a stream have listed for the list-mode k_frame (clip.h: stream_listed_tiles)
extern "C" int mlvfs_amd_test_stream_listed(void *stream, long long *tiles)
{
    return tiles ? mlv::stream_listed_tiles((hipStream_t)stream, tiles) : MLVFS_AMD_ERR_ARG;
}

// Test hook, host only: the plan that the calling thread's most recent launch of the fused pass committed, in the same 15 fields
extern "C" int mlvfs_amd_test_last_frame_plan(long long *out)
{
    const mlv::LastPlan &l = mlv::last_plan();
    if (!out || !l.set) return MLVFS_AMD_ERR_ARG;
    mlv::plan_fields(l.plan, out);
    return MLVFS_AMD_OK;
}

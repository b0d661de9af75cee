// frame_plan.h -- which kernels one launch of the fused pass runs, and how each is laid out (frame_plan.cpp).  Host arithmetic only:
// k_frame.hip (launch_frame) reads the stream's status words, plans, and executes the plan.
#pragma once

namespace mlv {

constexpr int FRAME_STREAM_COLW = 62;       // k_frame_s, k_frame_p5: lanes 1 .. 62 of a wave write a row's items, 0 and 63 are the halo
constexpr int FRAME_MAX_GROUPS = 1024;      // k_frame: tile-range groups at most (the stream's ticket counters: k_frame.hip)

enum class FirstKernel { none, p, p5, s };  // what runs first: nothing (k_frame alone), k_frame_p, k_frame_p5, k_frame_s (alone)
enum class StripeForm { none, packed, generic };

struct FramePassInputs {
    int w, h, bpp, black;
    int method;              // chroma smoothing: 0, 2, 3, 5
    bool packed;             // packed stream of bpp bits per pixel, else 16-bit frames
    int vec;                 // k_frame's input layout (launch_frame): 0 any, 1 / 2 rows of whole 16- / 8-pixel groups, 3 12-bit, 4 10-bit
    bool pixel_map;
    StripeForm stripes;      // packed: the packed 16-bit epilogue (FrameArgs::coef_pk)
    int nframes, num_cu;     // (num_cu 0: unknown, taken as 256)
};

// MLVFS_AMD_KF_P (k_frame_p / k_frame_p5 with the list-mode k_frame), _KF_P5 (k_frame_p5 rather than k_frame_p), _KF_S (k_frame_s):
// 0 never, 1 (default) as the stream's status words say, 2 whenever the kernel can run.  Read at every launch (the tests switch them).
struct FrameSwitches { int p = 1, p5 = 1, s = 1; };
FrameSwitches frame_switches();

// The status word whose back-off (k_frame.hip: Backoff) decides whether a launch starts with its first kernel: word 1 counts k_frame_s's
// steps that took the loader's form for pixels at or below black, word 0 the tiles k_frame_p / k_frame_p5 listed for k_frame.
struct FrameWatch {
    int word = -1;           // the word the candidate first kernel reports to; -1: there is none, k_frame runs alone
    bool adaptive = false;   // its back-off decides (switch at 1)
    bool status = false;     // the launch needs the word allocated (k_frame_s leaves it alone unless it is adaptive)
};
FrameWatch frame_pass_watch(const FramePassInputs &in, const FrameSwitches &sw);

struct StreamVerdict {
    bool held = false;        // the watched back-off holds the first kernel back: k_frame alone (counts only where adaptive)
    bool some_listed = false; // word 0's last look found more than a few per cent of the tiles listed: k_frame_p, whose skipping of
                              // the tiles behind an uncertain one pays there, rather than k_frame_p5 (unless _KF_P5=2)
};

// How a streaming kernel cuts a frame: columns of FRAME_STREAM_COLW items (8 x 2 pixels), segments of seg_rows cell rows, `fold`
// segments of a narrow last column side by side in one wave (a last column of <= 14 items: 4, <= 30 items: 2), tasks per frame.
struct StreamGeom { int cols, segs, fold, tasks_per_frame; };
StreamGeom stream_geom(int w, int h, int seg_rows);

struct FramePlan {
    FirstKernel first = FirstKernel::none;
    bool list_after = false;  // the list-mode k_frame follows and does again what the first kernel listed
    FrameWatch watch;
    long long tiles = 0;      // k_frame's tiles in the launch
    int grid = 0, groups = 0, run = 0, singles = 0;       // k_frame (and k_frame_p / k_frame_p5, which run on its grid)
    int first_grid = 0;       // workgroups of the first kernel
    int seg_rows = 0, cols = 0, segs = 0, fold = 0;       // k_frame_s, k_frame_p5 (stream_geom)
    long long tasks = 0;
    long long steps = 0;      // k_frame_s: wave-steps, what its dark steps are a share of (word 1's back-off)
    long long wl_entries = 0; // work-list entries the launch needs (list_after)
};

// MLVFS_AMD_OK, or MLVFS_AMD_ERR_ARG (set_error) for a launch the fused pass does not take
int check_frame_pass(const FramePassInputs &in);
int plan_frame_pass(const FramePassInputs &in, const FrameSwitches &sw, const StreamVerdict &v, FramePlan *out);

// The plan the calling thread's most recent launch committed, kept for mlvfs_amd_test_last_frame_plan (a thread-local copy on the host:
// the tests ask which kernels the launch they have just made took)
void record_frame_plan(const FramePlan &p);

}  // namespace mlv

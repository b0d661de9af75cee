"""The cases of the tests of k_frame_p5's step loop (tests/test_p5_loop_edges.py on the CPU, tests/test_gpu_p5_loop_edges.py on the GPU).

The kernel runs a task of n cell rows in n + 4 steps: four that fill the five-row window (rows j0 - 2 .. j0 + 1, no output), then pairs
of steps with an output stage and a prefetch while the first of a pair still has a row to fetch, then the last one or two steps, which
fetch nothing (csrc/k_frame_p.hip).  So the number of rows of a task decides which of these parts run and how often; a short launch is
cut into tasks of 30 rows, and the heights below give a frame's last (or only) task every length at which the parts change."""
import stream_shapes as S

SEG_ROWS = 30                 # a forced short launch (csrc/frame_plan.cpp: p5_seg_rows)

# one narrow column of two items; one of 14 items, folded in four where there are two segments and more (both VEC 1); a full column and
# one of one item, and of three items (both w % 16 == 8, the other unpack alignment: VEC 2)
WIDTHS = (16, 112, 504, 520)
# tasks of 1 .. 5 rows (warm-up and one last step; two last steps; then a main loop of one, one and two pairs, behind it one, two and
# one last steps), a last task of 1 and of 2 rows behind a full one, and 30 + 30 + 1
HEIGHTS = (2, 4, 6, 8, 10, 62, 64, 122)
CASES = [(w, h) for w in WIDTHS for h in HEIGHTS]
LOW_LIGHT_CASE = (520, 62)    # rows with and without pixels at or below black where the main loop hands over to the last steps

case_id = lambda c: f"{c[0]}x{c[1]}"


def task_rows(h):
    """Rows of the tasks a column of a w x h frame is cut into"""
    rows = h // 2
    return [min(SEG_ROWS, rows - j0) for j0 in range(0, rows, SEG_ROWS)]


def loop_parts(n):
    """(warm-up steps, pairs of the main loop, last steps) of a task of n rows, as the kernel's three loops count them: r runs from
    j0 - 2; the main loop takes pairs while r < j1; the rest are last steps, up to r = j1 + 1"""
    r, j0, j1 = -2, 0, n
    warm = 0
    while r < j0 + 2:
        r += 2
        warm += 2
    pairs = 0
    while r < j1:
        r += 2
        pairs += 1
    last = j1 + 1 - r + 1
    assert warm + 2 * pairs + last == n + 4 and 1 <= last <= 2, (n, warm, pairs, last)
    return warm, pairs, last


def allowed_listed(w, h, nframes):
    """Tiles a launch without a pixel map may list: at most stream_shapes.CALM_PERCENT of them"""
    return S.launch_tiles(w, h, nframes) * S.CALM_PERCENT // 100

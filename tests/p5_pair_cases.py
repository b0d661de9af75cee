"""The cases of the tests of k_frame_p5's pair step (tests/test_p5_pair_cases.py on the CPU, tests/test_gpu_p5_pair.py on the GPU).

A pair step takes cell rows r and r + 1 of a task and finishes rows r - 2 and r - 1: the two windows share four rows, sorted once, and
each adds its own fifth (csrc/k_frame_p.hip).  A task's rows come in from j0 - 2 in pairs; its last one (a task of an odd number of rows)
or two rows are single steps.  So what can go wrong depends on the parity of a task's length, on tasks shorter than the warm-up, and on
rows of one pair that differ in what they need: the loader's form, a pixel-map cell, an uncertain strip."""
import numpy as np

import stream_shapes as S
from mlvfs_amd import synth

# ------------------------------------------------------------------ task lengths
# Last segments of 1, 2, 3 and 4 cell rows behind full tasks, with tasks of 30 and of 60 rows: 61, 122, 63 and 64 cell rows.  The first
# two are geometries of stream_shapes.GEOMETRIES; 112 px are one column of 14 items, folded in four wherever there are two segments
PARITY_GEOMETRIES = [(504, 122), (744, 244), (112, 126), (112, 128)]
SHORT_GEOMETRY = (3584, 6)        # one segment of three rows: shorter than the warm-up
LOW_GEOMETRY = (744, 12)          # rows 2 and 3 are smoothed (4 <= y < h - 5), rows 0, 1, 4, 5 are not: the cut falls between pair steps and inside the last rows
# (w, h, seg_rows)
CASES = [(w, h, sr) for w, h in PARITY_GEOMETRIES for sr in S.SEG_ROWS] + [SHORT_GEOMETRY + (30,), LOW_GEOMETRY + (30,)]
case_id = lambda c: f"{c[0]}x{c[1]}-{c[2]}rows"


def all_classes():
    return ["odd task", "even task", "task of <= 4 rows", "folded last column"] + [f"last segment of {n} row(s)" for n in (1, 2, 3, 4)]


def classes(w, h, seg_rows):
    """What the cut of a geometry (the library's own: stream_shapes.shape) gives the pair step to get wrong"""
    s = S.shape(w, h, seg_rows)
    lengths = {seg_rows} if s["segs"] > 1 else set()
    lengths.add(s["last_rows"])
    out = set()
    for n in lengths:
        out.add("odd task" if n % 2 else "even task")
        if n <= 4:
            out.add("task of <= 4 rows")
    if s["segs"] > 1 and s["last_rows"] <= 4:
        out.add(f"last segment of {s['last_rows']} row(s)")
    if s["fold"] > 1:
        out.add("folded last column")
    return out


def missing(cases, seg_rows):
    hit = set()
    for w, h, sr in cases:
        if sr == seg_rows:
            hit |= classes(w, h, sr)
    return [c for c in all_classes() if c not in hit]


# ------------------------------------------------------------------ seams between the two rows of a pair
# One column, one task of 30 rows: rows come in in pairs (0, 1) .. (28, 29) (counted from j0 - 2: even first), rows go out in pairs
# (0, 1) .. (26, 27) and singly 28, 29.  ROW_A is the first row of a pair, ROW_B the second row of another.
SEAM_GEOMETRY = (256, 60)
ROW_A, ROW_B = 10, 13
SEAM_KINDS = ("dark", "pixel_map", "uncertain")
LEVEL = 3000                      # above black: every pixel bright, the loader's common form in every row


def flat_frame(w, h, seed):
    """Neutral grey, 0 .. 15 of noise: colour differences near zero, nothing uncertain, nothing dark"""
    rng = np.random.default_rng(seed)
    return (synth.BLACK + LEVEL + rng.integers(0, 16, (h, w))).astype(np.uint16)


def seam_frames(kind):
    """Two frames: what the case is about happens in ROW_A only in frame 0 and in ROW_B only in frame 1"""
    w, h = SEAM_GEOMETRY
    frames = [flat_frame(w, h, 5 + k) for k in range(2)]
    for f, row in zip(frames, (ROW_A, ROW_B)):
        if kind == "dark":
            f[2 * row, 80] = synth.BLACK              # one pixel at black: the whole wave converts this row in the loader's second form
        if kind == "uncertain":
            # 5 rows x 3 columns of cells with red four stops up: 15 of the 25 cells of the windows of (row, 40 .. 42), at most 12 of
            # any window of the rows above and below -- the median leaves the packed range in that row alone
            lin = f[2 * (row - 2):2 * (row + 3):2, 2 * 40:2 * 43:2].astype(np.int64) - synth.BLACK
            f[2 * (row - 2):2 * (row + 3):2, 2 * 40:2 * 43:2] = synth.BLACK + lin // 16
    return frames


def seam_pixel_map(kind):
    """The clip's pixel map: a cell in ROW_A and one in ROW_B (different pairs: each pair has one row with a cell and one without)"""
    if kind != "pixel_map":
        return None
    return np.array([[83, 2 * ROW_A], [170, 2 * ROW_B + 1]], np.int32)


def rows_with(frame, what):
    """Cell rows of a frame with a pixel at or below black / whose 5x5 median of red minus green lies a stop and more from zero"""
    h, w = frame.shape
    if what == "dark":
        return sorted(set(np.nonzero((frame <= synth.BLACK).reshape(h // 2, 2, w).any(axis=(1, 2)))[0].tolist()))
    lin = np.log2(np.maximum(frame.astype(np.float64) - synth.BLACK, 1))
    d = lin[0::2, 0::2] - (lin[0::2, 1::2] + lin[1::2, 0::2]) / 2
    out = []
    for j in range(2, h // 2 - 2):
        for i in range(2, w // 2 - 2):
            if abs(np.median(d[j - 2:j + 3, i - 2:i + 3])) >= 1.0:
                out.append(j)
                break
    return out


# Tiles that the parent commit's k_frame_p5 listed for these inputs (one launch of the two frames, recorded on an MI355X): the pair step
# lists the same ones
PARENT_LISTED = {"dark": 0, "pixel_map": 0, "uncertain": 2}

"""What the tests of k_frame_p5's EV table share (tests/test_p5_table_cases.py on the CPU, tests/test_gpu_p5_table.py on the GPU).

k_frame_p5 keeps raw2ev itself in LDS, indexed by pixel - black + 1 (csrc/k_frame_p.hip): entry 0 is what a pixel below black reads,
entry 1 a pixel AT black, entry 2 the first level above it, and a pixel of 16383 at black 0 reads the last entry.  The cases put
pixels on every one of those edges, at black levels on both ends of the table:

  table edges   the benchmark's footage kind with a seeded 1 % of every band of four pixel rows replaced by 0, black - 1, black,
                black + 1 and 16383 (kept inside 0 .. 16383), at black 0, 1, 2048, 8191, 16383 and 16384, on a frame of one full
                column (504x122) and on one whose only column is folded (112x484, 14 items)
  dark rows     504x122 at black 2048: bands of four pixel rows at or below black -- all AT black, all below, mixed -- between bright
                bands of twelve that carry black + 1 and 16383 alone, so the loader changes its form from step to step and a whole
                wave reads entry 0 or entry 1 at once.  A window of 5 x 5 cells then holds at most two dark cell rows, 10 cells of
                25, and its median is a bright cell's: k_frame_p5 can settle every strip itself and must (the dark bands keep
                clear of the rows a task takes its reference from)
  few tasks     one frame of 112x484: fewer tasks than a workgroup has waves"""
import numpy as np

import level_cases as LC

GEOMETRIES = ((504, 122), (112, 484))        # one full column of 62 items and a margin item; one folded column of 14 items
NFRAMES = 3
BAND = 4                                     # pixel rows
SHARE = 0.01

# black level and its white, paired as level_cases pairs them (white_of); all inside the packed stripes form, which the streaming
# kernels ask for
LEVELS = ((0, "15000"), (1, "16383"), (2048, "inner"), (8191, "above"), (16383, "inner"), (16384, "above"))
BLACKS = tuple(b for b, _ in LEVELS)
# At black 16383 no pixel lies above black and at 16384 all lie below: nothing to smooth, the loader's edges remain
JUDGED_BLACKS = tuple(b for b in BLACKS if b != 16383)

DARK_ROWS_GEOMETRY, DARK_ROWS_BLACK = (504, 122), 2048
FEW_TASKS_GEOMETRY = (112, 484)


def white_of(black):
    return LC.white_of(black, dict(LEVELS)[black])


def case_id(case):
    (w, h), black = case
    return f"{w}x{h}-black{black}"


CASES = [(g, b) for g in GEOMETRIES for b in BLACKS]


def edge_values(black):
    """The values sprinkled at a black level, inside the 14-bit range, without repeats"""
    return sorted({min(max(v, 0), 16383) for v in (0, black - 1, black, black + 1, 16383)})


def sprinkle(f, black, seed):
    """SHARE of every band of BAND pixel rows (five pixels at least) replaced by the five edge values in turn, at seeded places"""
    h, w = f.shape
    rng = np.random.default_rng(seed)
    values = [min(max(v, 0), 16383) for v in (0, black - 1, black, black + 1, 16383)]
    for y0 in range(0, h, BAND):
        rows = min(BAND, h - y0)
        n = max(5, -(-int(round(SHARE * rows * w)) // 5) * 5)
        at = rng.choice(rows * w, n, replace=False)
        f[y0 + at // w, at % w] = np.resize(values, n)
    return f


def footage(w, h, black, n=NFRAMES):
    """n frames of the benchmark's footage kind at `black` (level_cases.scaled), sprinkled with the edge values"""
    return [sprinkle(LC.scaled("normal", w, h, k, black).copy(), black, 7919 * black + 31 * w + k) for k in range(n)]


DARK_BAND_KINDS = ("at", "below", "mixed")
DARK_PERIOD, DARK_OFFSET = 16, 2             # pixel rows: a dark band of BAND rows starts at DARK_OFFSET + k * DARK_PERIOD


def dark_bands(h=DARK_ROWS_GEOMETRY[1]):
    """(first pixel row, kind) of every dark band"""
    return [(y0, DARK_BAND_KINDS[k % 3]) for k, y0 in enumerate(range(DARK_OFFSET, h - BAND + 1, DARK_PERIOD))]


def reference_rows(h, seg_rows):
    """The pixel rows a task of k_frame_p5 takes its reference from (csrc/k_frame_p.hip: four rows from min(j0 + j1, (h - 4) & ~1) & ~1,
    j0 / j1 the task's first cell row and the one behind its last)"""
    rows = h // 2
    out = set()
    for j0 in range(0, rows, seg_rows):
        y0 = min(j0 + min(j0 + seg_rows, rows), (h - 4) & ~1) & ~1
        out |= set(range(y0, y0 + 4))
    return out


def dark_rows_footage(n=NFRAMES):
    """Bright rows (with a few pixels of black + 1 and 16383 per four of them: the table's ends on the loader's common path) and dark
    bands of four pixel rows in turn: every pixel AT black, every pixel below it, both mixed"""
    (w, h), black = DARK_ROWS_GEOMETRY, DARK_ROWS_BLACK
    out = []
    for k in range(n):
        f = LC.scaled("normal", w, h, k, black).copy()
        rng = np.random.default_rng(1000 + k)
        f[f <= black] = black + 2
        for y0 in range(0, h, BAND):
            band = f[y0:y0 + BAND]
            at = rng.choice(band.size, 10, replace=False)
            band.reshape(-1)[at] = np.resize([black + 1, 16383], 10)           # (a view: the band's rows are contiguous)
        for y0, kind in dark_bands(h):
            band = f[y0:y0 + BAND]
            below = rng.integers(0, black, band.shape)
            band[...] = black if kind == "at" else below if kind == "below" else np.where(rng.random(band.shape) < 0.5, black, below)
        out.append(f)
    return out


def row_classes(f, black, y0, y1):
    """The classes (below / at / above black) the pixels of rows y0 .. y1 - 1 fall into"""
    lin = f[y0:y1].astype(np.int64) - black
    return {name for name, m in (("below", lin < 0), ("at", lin == 0), ("above", lin > 0)) if m.any()}


def band_classes(f, black):
    """Per band of BAND pixel rows: the set of classes (below / at / above black) its pixels fall into"""
    return [row_classes(f, black, y0, y0 + BAND) for y0 in range(0, f.shape[0], BAND)]


def interior_cells_changed(f, smoothed, bright_rows_only=False):
    """(cells whose pixels chroma smoothing changed, cells) away from the frame's two outermost cells; bright_rows_only: outside the
    dark-rows case's dark bands (what lies at or below black comes out as it went in)"""
    d = f != smoothed
    cells = d[0::2, 0::2] | d[0::2, 1::2] | d[1::2, 0::2] | d[1::2, 1::2]
    rows = np.arange(cells.shape[0])
    keep = (rows >= 2) & (rows < cells.shape[0] - 2)
    if bright_rows_only:
        for y0, _ in dark_bands(f.shape[0]):
            keep &= (rows < y0 // 2) | (rows >= (y0 + BAND) // 2)
    inner = cells[keep][:, 2:-2]
    return int(inner.sum()), inner.size

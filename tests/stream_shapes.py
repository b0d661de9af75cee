"""What the task-shape tests of the streaming kernels share (tests/test_stream_shapes.py on the CPU, tests/test_gpu_stream_shapes.py on
the GPU): the geometry list, the shape classes a geometry falls into -- taken from the library's own cut (mlvfs_amd_test_stream_plan,
csrc/frame_plan.cpp: stream_geom), not from a restatement of it --, the plan hooks and the footage.

k_frame_p5 and k_frame_s cut a frame into columns of items (8 pixels each), segments of seg_rows cell rows, and fold a narrow last column
(2 or 4 segments side by side in one wave); nearly all of their index arithmetic depends on the shape of that cut.  A class is one value
of one property of the cut; the list must reach every class with 30-row and with 60-row tasks (test_stream_shapes.py)."""
import ctypes as C

import numpy as np

from mlvfs_amd import lib, synth

SEG_ROWS = (30, 60)
HEADLINE = (3584, 1320)

# Every class below at both task lengths (test_stream_shapes.py names the classes a change of the cut would leave without a geometry).
# All but the headline geometry are at most 0.8 Mpix: the oracle's cs5x5 costs well under a second per frame.
GEOMETRIES = [
    (504, 240), (600, 242), (608, 304), (616, 394), (736, 240), (744, 244), (624, 182), (728, 362),
    (992, 480), (112, 484), (600, 608), (616, 788), (120, 480), (736, 724), (504, 122),
    (112, 960),
    (1096, 124),
    HEADLINE,
]

# A subset that still reaches every class with 60-row tasks: k_frame_p5 gets those on long launches only (thousands of small frames)
LONG_GEOMETRIES = [(112, 484), (504, 122), (616, 788), (736, 240), (744, 244), (992, 480), (112, 960), (1096, 124), (600, 242)]

# focus-pixel maps through k_frame_p5: the frame and grid (dx, dy) of tests/test_gpu_stream.py: test_dense_focus_pixel_map, and a thinner grid
FOCUS_GEOMETRY = (416, 264)
DENSE_GRID, THIN_GRID = (5, 3), (48, 8)

KINDS = ("normal", "low_light", "colour_cast", "adversarial")

PLAN_KEYS = ("first", "list_after", "grid", "groups", "run", "singles", "first_grid", "seg_rows", "cols", "segs", "fold", "tasks", "steps",
             "wl_entries", "word")
P_NONE, P_TILES, P_P5, P_S = 0, 1, 2, 3          # first kernel: k_frame alone, k_frame_p, k_frame_p5, k_frame_s


def stream_plan(w, h, seg_rows):
    """(cols, segs, fold, tasks_per_frame) of the library's cut"""
    v = [C.c_int() for _ in range(4)]
    rc = lib.load().mlvfs_amd_test_stream_plan(w, h, seg_rows, *[C.byref(x) for x in v])
    assert rc == 0, (w, h, seg_rows)
    return tuple(x.value for x in v)


_col_items = None


def col_items():
    """Items in a full column: the widest frame of one column, found through the hook"""
    global _col_items
    if _col_items is None:
        n = 2
        while stream_plan(8 * (n + 1), 64, 30)[0] == 1:
            n += 1
            assert n < 4096
        _col_items = n
    return _col_items


def shape(w, h, seg_rows):
    """The cut of a w x h frame into tasks of seg_rows cell rows, as the properties the kernels' index arithmetic depends on"""
    cols, segs, fold, tasks = stream_plan(w, h, seg_rows)
    folded = tasks - (cols - 1) * segs if fold > 1 else 0            # folded tasks of the last column
    return dict(cols=cols, segs=segs, fold=fold, tasks=tasks, vec=1 if w % 16 == 0 else 2,
                last_items=w // 8 - col_items() * (cols - 1),
                last_rows=h // 2 - seg_rows * (segs - 1),
                folded=folded, last_parts=segs - fold * (folded - 1) if fold > 1 else 0)


def all_classes():
    out = [f"last column of {n} items" for n in ("1", "13-14", "15-16", "29-30", "31", "a full column's")]
    out += [f"fold {f}, VEC {v}" for f in (1, 2, 4) for v in (1, 2)]
    out += [f"fold {f}, {p} part(s) in the last folded task" for f in (2, 4) for p in range(1, f + 1)]
    out += [f"last segment of {n}" for n in ("1 row", "2 rows", "some rows", "a full task")]
    out += [f"{n} folded task(s) per column" for n in ("1", "2", ">= 3")]
    out += [f"{n} column(s)" for n in ("1", "2", ">= 3")]
    return out


def classes(w, h, seg_rows):
    """The classes a geometry falls into; only geometries of two segments and more count"""
    s = shape(w, h, seg_rows)
    if s["segs"] < 2:
        return set()
    out = set()
    li = s["last_items"]
    for name, values in (("1", (1,)), ("13-14", (13, 14)), ("15-16", (15, 16)), ("29-30", (29, 30)), ("31", (31,)), ("a full column's", (col_items(),))):
        if li in values:
            out.add(f"last column of {name} items")
    out.add(f"fold {s['fold']}, VEC {s['vec']}")
    if s["fold"] > 1:
        out.add(f"fold {s['fold']}, {s['last_parts']} part(s) in the last folded task")
        out.add(f"{s['folded'] if s['folded'] < 3 else '>= 3'} folded task(s) per column")
    lr = s["last_rows"]
    out.add("last segment of " + ("1 row" if lr == 1 else "2 rows" if lr == 2 else "a full task" if lr == seg_rows else "some rows"))
    out.add(f"{s['cols'] if s['cols'] < 3 else '>= 3'} column(s)")
    assert out <= set(all_classes()), out - set(all_classes())
    return out


def missing(geometries, seg_rows):
    """Classes that no geometry of the list reaches with tasks of seg_rows rows"""
    hit = set()
    for w, h in geometries:
        hit |= classes(w, h, seg_rows)
    return [c for c in all_classes() if c not in hit]


def task_regions(w, h, seg_rows):
    """The cell ranges (cx_lo, cx_hi, cy_lo, cy_hi) whose pixel-map records a task collects: a column's items with the halo item on
    either side (4 cells each), a segment's rows with two halo rows above and below, clipped to the frame"""
    cols, segs, _, _ = stream_plan(w, h, seg_rows)
    out = []
    for c in range(cols):
        for sg in range(segs):
            j0, j1 = sg * seg_rows, min((sg + 1) * seg_rows, h // 2)
            out.append((max(4 * (c * col_items() - 1), 0), min(4 * ((c + 1) * col_items() + 1), w // 2), max(j0 - 2, 0), min(j1 + 2, h // 2)))
    return out


def records_per_region(points, w, h, seg_rows):
    """Cells of a pixel map (one record per repaired cell) in every task's region"""
    cells = np.unique(np.stack([points[:, 0] // 2, points[:, 1] // 2], 1), axis=0)
    return [int(((cells[:, 0] >= x0) & (cells[:, 0] < x1) & (cells[:, 1] >= y0) & (cells[:, 1] < y1)).sum())
            for x0, x1, y0, y1 in task_regions(w, h, seg_rows)]


# ------------------------------------------------------------------ the plan of a launch
def frame_plan(w, h, cs, nframes, cus, pmap, stripes, bpp=14, black=synth.BLACK, packed=1):
    """mlvfs_amd_test_frame_plan for a launch on a fresh stream (nothing held back, nothing listed), the switches as the environment has
    them; None for a launch the fused pass refuses"""
    out = (C.c_longlong * 15)()
    vec = 1 if w % 16 == 0 else 2
    rc = lib.load().mlvfs_amd_test_frame_plan((C.c_int * 13)(w, h, bpp, black, cs, packed, vec, int(pmap), int(stripes), nframes, cus, 0, 0), out)
    return None if rc else dict(zip(PLAN_KEYS, out))


def last_plan():
    """The plan the calling thread's last launch took (mlvfs_amd_test_last_frame_plan)"""
    out = (C.c_longlong * 15)()
    rc = lib.load().mlvfs_amd_test_last_frame_plan(out)
    assert rc == 0, "no launch on this thread yet"
    return dict(zip(PLAN_KEYS, out))


def assert_took(first, w=None, h=None, seg_rows=0, what=""):
    """The last launch started with `first`; for the streaming kernels: in tasks of seg_rows rows, cut as the hook cuts w x h"""
    p = last_plan()
    assert p["first"] == first, f"{what}: the launch took first kernel {p['first']}, not {first}: {p}"
    if first in (P_P5, P_S):
        cols, segs, fold, tasks = stream_plan(w, h, seg_rows)
        got = tuple(p[k] for k in ("seg_rows", "cols", "segs", "fold"))
        assert got == (seg_rows, cols, segs, fold), f"{what}: {got} != {(seg_rows, cols, segs, fold)}"
        assert p["list_after"] == (first == P_P5)
    return p


def stripes_form(clip_stream, stripes):
    """How a launch with stripes sorts the clip's coefficients (csrc/k_frame.hip: launch_frame): 0 none (not asked for, or the clip needs
    none), 1 the packed 16-bit form, 2 beyond it -- the streaming kernels do not take those, k_frame_p / k_frame do"""
    if not stripes:
        return 0
    needed, co = clip_stream.get_stripes()
    if not needed:
        return 0
    packed = all(-32768 < int(c) - 65536 < 32768 for c in co) and clip_stream.white > clip_stream.black + 64 and 0 <= clip_stream.black <= 16384
    return 1 if packed else 2


# The share of a launch's tiles listed above which the library itself calls a stream "not calm" and moves its next launches from
# k_frame_p5 to k_frame_p (csrc/k_frame.hip: KF_P5_CALM_PERCENT).  k_frame in list mode does every listed tile again, so a k_frame_p5
# that computed nothing right and listed everything would still give the oracle's bytes: on the benchmark's footage kind, which the
# library's default policy must keep on k_frame_p5, a long launch has to stay below this share.
CALM_PERCENT = 5


def listed_tiles():
    """Tiles listed for the list-mode k_frame on torch's current stream so far (mlvfs_amd_test_stream_listed); synchronises"""
    import torch
    torch.cuda.current_stream().synchronize()
    n = C.c_longlong(0)
    rc = lib.load().mlvfs_amd_test_stream_listed(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(n))
    assert rc in (0, lib.ERR_ARG), rc
    return n.value if rc == 0 else 0


def launch_tiles(w, h, nframes):
    """k_frame's tiles in a launch: 64 x 15 cells (128 x 30 pixels) each"""
    return -(-w // 128) * -(-h // 30) * nframes


def frames_for_60_rows(w, h, cus, pmap, stripes, limit=1 << 20):
    """The smallest frame count at which a cs5x5 launch goes to k_frame_p5 in tasks of 60 rows (MLVFS_AMD_KF_P / _KF_P5 as set)"""
    def ok(n):
        p = frame_plan(w, h, 5, n, cus, pmap, stripes)
        return p is not None and p["first"] == P_P5 and p["seg_rows"] == 60
    hi = 1
    while not ok(hi):
        hi *= 2
        assert hi <= limit, (w, h)
    lo = hi // 2                                     # not ok (or 0)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            hi = mid
        else:
            lo = mid
    return hi


# ------------------------------------------------------------------ footage
def footage(kind, w, h, n):
    """n distinct frames of a footage kind, as tests/test_gpu_stream.py makes them"""
    gen = getattr(synth, kind + "_frame")
    if kind in ("low_light", "colour_cast"):
        return [gen(w, h, seed=3 + k) for k in range(n)]
    return [gen(w, h, frame=k) for k in range(n)]


def grid_map(w, h, dx, dy):
    """A focus-pixel map as some cameras have it: a regular grid, some cells with two repaired pixels, and the frame's edges (the edge
    rules of cs.c:479-497) -- tests/test_gpu_stream.py: test_dense_focus_pixel_map is grid_map(w, h, 5, 3)"""
    ys, xs = np.mgrid[6:h - 6:dy, 7:w - 8:dx]
    pts = np.stack([xs.reshape(-1), ys.reshape(-1)], 1).astype(np.int32)
    edge = [[1, 50], [w - 2, 60], [100, 1], [120, h - 2], [2, 2], [w - 1, h - 1], [0, 100]]
    return np.concatenate([pts, pts[::7] + [1, 0], edge]).astype(np.int32)

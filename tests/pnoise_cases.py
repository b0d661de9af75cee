"""The cases of the pattern-noise correction (tests/test_gpu_pnoise.py runs them on the GPU against the oracle; tests/test_pnoise_cases.py
proves on the CPU that the definition below is the oracle's, that the cases reach what they claim and that each wrong form of the
definition shows on a case that names it).  Everything here is deterministic; nothing needs a GPU or the oracle.

fix(frame, white, flags, wrong) is fix_pattern_noise (mlvfs/patternnoise.c:49-380) restated in Python ints with every int16 store
written out as a wrap; `wrong` names one deliberately wrong form (WRONG).  It is for small frames only.

A case is a dict: name, w, h, white, frame (uint16, (h, w)), tells (the wrong forms it is there for; content cases only) and geometry
(True where only the oracle judges it: the sizes at which the launcher changes the column-median kernel)."""
import numpy as np

THR, REACH, GRAD, MIN_SAMPLES = 500, 25, 500, 10

WRONG = [
    "reach_right_25",      # 25 pixels to the right of the centre (the reference: x + 25 exclusive, so 24)
    "reach_left_24",       # 24 pixels to the left (the reference: x - 25 inclusive)
    "thr_lt",              # the run goes on while |avg - centre| < 500 (the reference: <= 500)
    "grad_ge",             # masked from |gradient| >= 500 (the reference: > 500)
    "white_gt",            # masked from pixel > white (the reference: >= white)
    "min_9",               # a column's offset from 9 samples (the reference: 10)
    "min_11",              # ... from 11
    "upper_run",           # upper median of an even run
    "upper_col",           # upper median of a column's even number of samples
    "upper_offs",          # upper median of an even number of column offsets
    "avg_floor",           # (g1 + g2) >> 1 (the reference: C division, towards zero)
    "mg_floor",            # (mg1 + mg2) >> 1
    "no_wrap_rb",          # r - avg, b - avg kept wider than int16
    "no_wrap_noise",       # original - smoothed kept wider than int16
    "no_wrap_grad",        # the flat-array gradient kept wider than int16
    "no_wrap_sum",         # median + mg kept wider than int16 (unobservable: UNOBSERVABLE)
    "clamp1_32768",        # the first clamp's lower end at -32768 (unobservable: UNOBSERVABLE)
    "clamp_32767",         # the final clamp's upper end at 32767 (the reference: 32760)
    "no_clamp_0",          # no final clamp at 0
    "grad_per_row",        # the gradient taken inside a row only (the reference: on the flat array, across row ends)
    "grad_drop_edge",      # no gradient at flat indices 2 and n - 3 (the reference: 0 only at 0, 1, n - 2, n - 1)
    "wrap_sub",            # run medians by bisection whose "value > mid" test is a wrapping 16-bit mid - v < 0 (the kernel: saturating)
]
# wrong forms that no input can show, each with its reason (tests/test_pnoise_cases.py asserts that they change nothing on any case)
UNOBSERVABLE = {
    "no_wrap_sum": "the smoothed planes are int16 in every view, and the noise wraps orig - smoothed again: both see the sum modulo 2^16",
    "clamp1_32768": "a column offset is a negated int16 median, so the offsets' median is >= -32767: -32767 - mc and -32768 - mc are "
                    "both <= 0 and the final clamp makes both 0",
}
VIEWS = (2, 4, 8, 3, 5, 9)                                  # debug_flags: denoised / noise / mask of the column pass, then of the row pass


def _w16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def _cdiv2(s):
    return -((-s) >> 1) if s < 0 else s >> 1                # C's s / 2: towards zero


def _median(vals, upper=False):
    s = sorted(vals)
    return s[len(s) // 2 if upper else (len(s) - 1) // 2]


def _median_wrap_sub(vals):
    """the kernel's bisection (smallest mid with #{v <= mid} >= rank) with v > mid decided by the sign of a wrapping 16-bit mid - v"""
    a, b, need = min(vals), max(vals), (len(vals) - 1) // 2 + 1
    while a < b:
        mid = (a + b) >> 1
        if sum(1 for v in vals if _w16(mid - v) >= 0) >= need:
            b = mid
        else:
            a = mid + 1
    return a


def _column_pass(raw, white, view, wrong, stats):
    """one direction on an int16 frame (h, w) -> the int16 frame after it (or the view of it)"""
    h, w = raw.shape
    hw, hh = w // 2, h // 2
    n = hw * hh
    if stats is not None:
        stats["pass"] += 1
    P = [raw[c >> 1:2 * hh:2, c & 1:2 * hw:2].astype(np.int64).reshape(-1).tolist() for c in range(4)]        # r, g1, g2, b
    r, g1, g2, b = P
    # ---- the smoothed planes (patternnoise.c:88-180)
    div_avg = (lambda s: s >> 1) if wrong == "avg_floor" else _cdiv2
    div_mg = (lambda s: s >> 1) if wrong == "mg_floor" else _cdiv2
    wrap_rb = (lambda v: v) if wrong == "no_wrap_rb" else _w16
    wrap_sum = (lambda v: v) if wrong == "no_wrap_sum" else _w16
    run_median = _median_wrap_sub if wrong == "wrap_sub" else (lambda v: _median(v, wrong == "upper_run"))
    within = (lambda d: abs(d) < THR) if wrong == "thr_lt" else (lambda d: abs(d) <= THR)
    right, left = REACH + (wrong == "reach_right_25"), REACH - (wrong == "reach_left_24")
    avg = [div_avg(p + q) for p, q in zip(g1, g2)]
    drg = [wrap_rb(p - a) for p, a in zip(r, avg)]
    dbg = [wrap_rb(p - a) for p, a in zip(b, avg)]
    if stats is not None:
        stats["neg_odd_avg"] += sum(1 for p, q in zip(g1, g2) if p + q < 0 and (p + q) & 1)
    S = [[0] * n for _ in range(4)]
    for y in range(hh):
        o = y * hw
        ag = avg[o:o + hw]
        prev = None
        for x in range(hw):
            centre = ag[x]
            hi, lo = min(x + right, hw), max(x - left, 0)
            xr, xl = x + 1, x - 1
            while xr < hi and within(ag[xr] - centre):
                xr += 1
            while xl >= lo and within(ag[xl] - centre):
                xl -= 1
            if (xl, xr) != prev:                              # the same run gives the same medians (patternnoise.c:146-153)
                prev = (xl, xr)
                a0, a1 = o + xl + 1, o + xr
                mg1, mg2 = run_median(g1[a0:a1]), run_median(g2[a0:a1])
                mg = div_mg(mg1 + mg2)
                mr, mb = wrap_sum(run_median(drg[a0:a1]) + mg), wrap_sum(run_median(dbg[a0:a1]) + mg)
                if stats is not None:
                    stats["runs"].add(xr - xl - 1)
                    stats["neg_odd_mg"] += int(mg1 + mg2 < 0 and (mg1 + mg2) & 1)
            S[0][o + x], S[1][o + x], S[2][o + x], S[3][o + x] = mr, mg1, mg2, mb
    # ---- per plane: the mask, the column offsets, the correction (patternnoise.c:185-282)
    wrap_noise = (lambda v: v) if wrong == "no_wrap_noise" else _w16
    wrap_grad = (lambda v: v) if wrong == "no_wrap_grad" else _w16
    g_lo, g_hi = (3, n - 3) if wrong == "grad_drop_edge" else (2, n - 2)
    min_samples = 9 if wrong == "min_9" else 11 if wrong == "min_11" else MIN_SAMPLES
    out = np.empty((h, w), np.int16)
    out[...] = raw
    for c in range(4):
        orig, sm = P[c], S[c]
        noise = [wrap_noise(p - s) for p, s in zip(orig, sm)]
        masked = [False] * n
        for i in range(n):
            g = 0
            if g_lo <= i < g_hi and not (wrong == "grad_per_row" and not 2 <= i % hw < hw - 2):
                g = wrap_grad(orig[i - 2] - orig[i + 2])
            edge = abs(g) >= GRAD if wrong == "grad_ge" else abs(g) > GRAD
            masked[i] = edge or (orig[i] > white if wrong == "white_gt" else orig[i] >= white)
            if stats is not None:
                stats["grads"].add(abs(g))
                stats["at_white"] += int(orig[i] == white)
        if view == 2:
            res = [_w16(s) for s in sm]
        elif view == 4:
            res = [_w16((-100 if m else v) + 100) for m, v in zip(masked, noise)]
        elif view == 8:
            res = [1000 * int(m) for m in masked]
        else:
            offs = []
            for x in range(hw):
                col = [noise[i] for i in range(x, n, hw) if not masked[i]]
                offs.append(0 if len(col) < min_samples else -_median(col, wrong == "upper_col"))
                if stats is not None:
                    stats["samples"].add((stats["pass"], len(col)))
            first_lo = -32768 if wrong == "clamp1_32768" else -32767
            v1 = [min(max(orig[i] + offs[i % hw], first_lo), 32767) for i in range(n)]
            mc = _median(offs, wrong == "upper_offs")
            top = 32767 if wrong == "clamp_32767" else 32760
            res = [min(v - mc, top) for v in v1]
            res = [_w16(v) for v in res] if wrong == "no_clamp_0" else [max(v, 0) for v in res]
        out[c >> 1:2 * hh:2, c & 1:2 * hw:2] = np.array(res, np.int64).astype(np.int16).reshape(hh, hw)
    return out


def new_stats():
    """what a run of fix() met: the run lengths, the numbers of unmasked samples of the columns as (pass, samples) -- pass 1 is the
    first direction run, 2 the second --, the |gradients|, how many pixels equal white, and how many negative odd sums each of the two
    divisions by 2 saw (where C division and a shift differ)"""
    return {"pass": 0, "runs": set(), "samples": set(), "grads": set(), "at_white": 0, "neg_odd_avg": 0, "neg_odd_mg": 0}


def fix(frame, white, flags=0, wrong=None, stats=None):
    """fix_pattern_noise(frame, w, h, white, flags) -> uint16 (h, w); the frame itself is left alone"""
    assert wrong is None or wrong in WRONG
    raw = np.ascontiguousarray(frame).view(np.int16).copy()
    view = 2 if flags & 2 else 4 if flags & 4 else 8 if flags & 8 else 0
    if not flags or not flags & 1:
        raw = _column_pass(raw, white, view, wrong, stats)
    if not flags or flags & 1:
        raw = np.ascontiguousarray(_column_pass(np.ascontiguousarray(raw.T), white, view, wrong, stats).T)
    return raw.view(np.uint16)


# ---------------------------------------------------------------- material
def _hash(n, seed):
    """n 64-bit values from a counter (splitmix64): the same on every machine and numpy"""
    with np.errstate(over="ignore"):
        z = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed) * np.uint64(0xD1B54A32D192ED03)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def rnd(shape, seed, lo, hi):
    """integers in lo..hi (both included), int64"""
    n = int(np.prod(shape))
    return (lo + (_hash(n, seed) % np.uint64(hi - lo + 1)).astype(np.int64)).reshape(shape)


def mosaic(r, g1, g2, b):
    """four half-resolution planes of signed values -> the Bayer frame, uint16 (the int16 bits)"""
    hh, hw = r.shape
    f = np.zeros((2 * hh, 2 * hw), np.int64)
    f[0::2, 0::2], f[0::2, 1::2], f[1::2, 0::2], f[1::2, 1::2] = r, g1, g2, b
    return (f & 0xFFFF).astype(np.uint16)


def walk_frame(hw, hh, seed, centre=32768, step=40, noise=300):
    """a slow random walk along every row around `centre` (as uint16: 32768 is where int16 turns negative), a few hundred counts of
    noise on it, and a fixed offset per column and row for the correction to find"""
    base = centre + np.cumsum(rnd((hh, hw), seed, -step, step), axis=1) + rnd((hh, 1), seed + 1, -150, 150)
    cols, rows = rnd((1, hw), seed + 2, -40, 40), rnd((hh, 1), seed + 3, -40, 40)
    planes = [base + cols + rows + rnd((hh, hw), seed + 10 + c, -noise, noise) for c in range(4)]
    return mosaic(*planes)


def white_edge_frame(hw, hh, seed, white):
    """only the values white - 1, white, white + 1 (modulo 2^16)"""
    return mosaic(*[white + rnd((hh, hw), seed + c, -1, 1) for c in range(4)])


def _case(name, frame, white, tells=(), geometry=False):
    h, w = frame.shape
    assert frame.dtype == np.uint16 and w % 2 == 0 and h % 2 == 0
    assert all(t in WRONG for t in tells), tells
    return dict(name=name, w=w, h=h, white=int(white), frame=frame, tells=tuple(tells), geometry=geometry)


# ---------------------------------------------------------------- content cases
def _fullrange():
    return _case("fullrange", mosaic(*[rnd((24, 48), 40 + c, -32768, 32767) for c in range(4)]), 65535,
                 ("no_wrap_rb", "no_wrap_grad", "upper_run", "wrap_sub", "no_clamp_0", "avg_floor", "mg_floor", "grad_per_row", "grad_drop_edge"))


def _walk():
    return _case("walk", walk_frame(80, 32, 7), 65535,
                 ("avg_floor", "mg_floor", "no_clamp_0", "no_wrap_rb", "no_wrap_noise", "no_wrap_grad", "upper_run", "upper_col", "grad_ge",
                  "reach_right_25", "reach_left_24", "clamp_32767", "wrap_sub"))


def _walk_tall():
    """the walk seen by the row pass first in its views, white inside the walk's range"""
    return _case("walk_tall", np.ascontiguousarray(walk_frame(48, 20, 9, centre=32768 + 200).T), 32768 + 300 - 65536,
                 ("white_gt", "upper_col", "min_11", "no_wrap_noise", "wrap_sub", "grad_drop_edge"))


def _rb_far():
    """red and blue more than 32767 away from green, either way round: r - avg and b - avg wrap"""
    hw, hh = 32, 16
    sign = np.where(np.arange(hh)[:, None] % 2 == 0, 1, -1)
    g1 = -16000 * sign + rnd((hh, hw), 50, -200, 200)
    g2 = -16000 * sign + rnd((hh, hw), 51, -200, 200)
    r = 16700 * sign + rnd((hh, hw), 52, -3000, 3000)           # r - avg around +-32700: a run's differences lie on both sides of the wrap
    b = 17000 * sign + rnd((hh, hw), 53, -6000, 6000)
    return _case("rb_far", mosaic(r, g1, g2, b), 65535, ("no_wrap_rb", "upper_offs", "wrap_sub"))


def _g_split():
    """g1 and g2 far apart, their average inside the threshold: a run's g1 and g2 span more than half the int16 range"""
    hw, hh = 32, 16
    flip = np.where(rnd((hh, hw), 60, 0, 1) == 1, 1, -1)
    g1 = 30000 * flip + rnd((hh, hw), 61, -200, 200)
    g2 = -30000 * flip + rnd((hh, hw), 62, -200, 200)
    r = rnd((hh, hw), 63, -300, 300) + 28000 * np.where(rnd((hh, hw), 64, 0, 2) == 0, flip, 0)
    b = rnd((hh, hw), 65, 1000, 1600)
    return _case("g_split", mosaic(r, g1, g2, b), 65535, ("wrap_sub", "upper_run", "mg_floor", "avg_floor", "min_9", "no_wrap_noise"))


def _extremes():
    """real 32767 and -32768 inside runs and at their ends: rows around 0 where g1 = 32767 meets g2 = -32768 (average 0), rows near
    either end of the range, a row that is 32767 throughout and one that is -32768"""
    hw, hh = 40, 16
    planes = [rnd((hh, hw), 70 + c, -200, 200) for c in range(4)]
    r, g1, g2, b = planes
    for y in range(0, 6):
        for x in (0, 1, 7, 8, 20, 33, hw - 2, hw - 1):
            top = (x + y) % 2 == 0
            g1[y, x], g2[y, x] = (32767, -32768) if top else (-32768, 32767)
            r[y, x], b[y, x] = (32767, -32768) if (x + y) % 3 else (-32768, 32767)
    for y in (6, 7, 8):                                       # near the top: a step ends a run next to planted 32767s
        for p in planes:
            p[y] = 32600 + rnd((hw,), 80 + y, -160, 160)
            p[y, 24:] -= 3000
        g1[y, [0, 5, 23, 24, hw - 1]] = 32767
        g2[y, [0, 6, 23, hw - 1]] = 32767
        r[y, [0, 4, 23]] = 32767
    for y in (9, 10, 11):                                     # near the bottom
        for p in planes:
            p[y] = -32600 + rnd((hw,), 90 + y, -160, 160)
            p[y, :13] += 3000
        g1[y, [12, 13, 14, 30, hw - 1]] = -32768
        g2[y, [13, 31, hw - 1]] = -32768
        b[y, [13, 20, hw - 1]] = -32768
    for p in planes:
        p[12], p[13] = 32767, -32768
        p[14], p[15] = 32767, -32768
    g1[14, 3::7], g2[15, 2::5] = 32760, -32761
    return _case("extremes", mosaic(r, g1, g2, b), 65535, ("wrap_sub", "upper_run", "clamp_32767", "no_wrap_noise", "no_wrap_grad"))


def _white_edge(name, white, tells):
    return _case(name, white_edge_frame(40, 12, 100 + (white & 255), white), white, tells)


def _steps():
    """the green average steps by exactly 500 and 501 along a row (g1 = level + d, g2 = level - d: the average is the level itself)"""
    hw, hh = 60, 12
    widths = rnd((hh, 16), 110, 2, 7)
    level = np.zeros((hh, hw), np.int64)
    for y in range(hh):
        x, lv, k = 0, 3000 + 700 * y - (9000 if y % 3 == 2 else 0), 0
        while x < hw:
            level[y, x:x + widths[y, k % 16]] = lv
            x += widths[y, k % 16]
            lv += (500, 501, -500, -501, 500, 500, -501, 501)[(k + y) % 8]
            k += 1
    d = rnd((hh, hw), 111, -120, 120)
    r = level + rnd((hh, hw), 112, -150, 150)
    b = level + rnd((hh, hw), 113, -150, 150)
    return _case("steps", mosaic(r, level + d, level - d, b), 65535, ("thr_lt", "upper_run", "mg_floor", "min_9", "min_11"))


def _grads(transposed):
    """same-plane pixels four apart in the flat array (two either side of a pixel) differing by exactly 500 and 501, either sign: inside
    rows, across row ends, and around flat indices 0..3 and n-4..n-1; 10 samples per column, so that one more masked sample silences
    a column's offset, and a fixed offset per column to silence"""
    hw, hh = 36, 10
    n = hw * hh
    cols = (np.arange(hw) % 7 - 3) * 25
    planes = []
    for c in range(4):
        p = (4000 + 600 * c + cols[None, :] + rnd((hh, hw), 120 + c, -12, 12)).reshape(-1)
        # (flat index of the pixel whose gradient is planted, difference in[i - 2] - in[i + 2])
        plant = [(2, 1200), (n - 3, -1200), (3, 500), (n - 4, 501), (hw - 1, 501), (hw, -501), (hw + 1, 500), (2 * hw - 2, -500),
                 (3 * hw - 1, 700), (4 * hw, -700), (5 * hw + 1, 900), (6 * hw - 2, -900), (3 * hw + 10, 500), (3 * hw + 20, 501),
                 (5 * hw + 15, -500), (5 * hw + 25, -501), (7 * hw + 9, 65300), (8 * hw + 17, -501), (8 * hw + 27, -65250)]
        plant = plant[c:] + plant[:c] if c else plant
        for i, d in plant:
            if abs(d) > 32767:                                # a difference that wraps to a small one: -236, 286
                p[i - 2] = 32700 if d > 0 else -32600
            p[i + 2] = p[i - 2] - d
        p[0], p[1], p[n - 1], p[n - 2] = p[4] + 2000, p[5] - 2000, p[n - 5] + 2000, p[n - 6] - 2000       # what a gradient at 0, 1, n-2, n-1 would see
        planes.append(p.reshape(hh, hw))
    f = mosaic(*planes)
    return _case("grads_t" if transposed else "grads", np.ascontiguousarray(f.T) if transposed else f, 65535,
                 ("grad_ge", "grad_per_row", "grad_drop_edge", "no_wrap_grad", "min_9", "min_11", "upper_offs"))


def _flat(name, hw, hh, seed, tells):
    """flat and noisy: every run is as long as the reach and the row's ends allow; a fixed offset per column and row"""
    cols, rows = rnd((1, hw), seed, -60, 60), rnd((hh, 1), seed + 1, -60, 60)
    planes = [2000 + 300 * c + cols + rows + rnd((hh, hw), seed + 2 + c, -90, 90) for c in range(4)]
    return _case(name, mosaic(*planes), 65535, tells)


def _mask_counts(transposed):
    """12 samples per column; bright pixels (far above white, so that they stay above it after the first direction) leave 0, 9, 10 and
    11 unmasked samples in some columns"""
    hw, hh = 30, 12
    cols = (np.arange(hw) * 7 % 11 - 5) * 12
    planes = [6000 + 500 * c + cols[None, :] + rnd((hh, hw), 140 + c, -25, 25) for c in range(4)]
    for x, masked in ((3, 12), (9, 3), (15, 2), (21, 1), (26, 3), (28, 2)):
        rows = [(5 * k + x) % hh for k in range(masked)] if masked < hh else range(hh)
        for p in planes:
            for y in rows:
                p[y, x] = 20000 + 37 * y
    f = mosaic(*planes)
    return _case("mask_counts_t" if transposed else "mask_counts", np.ascontiguousarray(f.T) if transposed else f, 12000,
                 ("min_9", "min_11", "upper_col", "upper_offs"))


def _clamps():
    """rows near 32767 whose columns get positive offsets (the first clamp, then 32760), rows near 32760, and rows of small pixels
    under a positive median of the offsets (clamped to 0)"""
    hw, hh = 32, 16
    cols = np.where(np.arange(hw) % 3 == 0, 12, -6)[None, :] + rnd((1, hw), 150, -2, 2)       # most columns low: their offsets, and the median, positive
    level = np.array([32764, 32766, 32761, 32758, 32765, 32755, 3, 0, 5, 1, 8, 2, 32763, 4, 32760, 6])[:, None]
    planes = [np.clip(level + cols + rnd((hh, hw), 151 + c, -4, 4), -32768, 32767) for c in range(4)]
    return _case("clamps", mosaic(*planes), 65535, ("clamp_32767", "no_clamp_0", "upper_offs", "avg_floor"))


def content_cases():
    return [
        _walk(), _walk_tall(), _fullrange(), _rb_far(), _g_split(), _extremes(),
        _white_edge("white_edge_12000", 12000, ("white_gt", "min_9", "min_11")),
        _white_edge("white_edge_65535", 65535, ()),
        _white_edge("white_edge_neg", -1, ("white_gt", "min_9")),
        _steps(), _grads(False), _grads(True),
        _flat("flat_wide", 80, 10, 130, ("reach_right_25", "reach_left_24", "upper_run", "upper_col", "upper_offs")),
        _flat("flat_hw25", 25, 12, 131, ("upper_run", "upper_col")),           # odd half widths below 26: one run per row, the whole row
        _flat("flat_hw21", 21, 26, 132, ("upper_run", "upper_col", "reach_right_25")),
        _flat("flat_hw13", 13, 14, 133, ("upper_run", "upper_col")),
        _mask_counts(False), _mask_counts(True), _clamps(),
    ]


# ---------------------------------------------------------------- geometry cases
# the launcher takes k_pn_column_offsets<12> up to a half-extent of 768, <32> up to 2048, <0> above, for the column height and, by the
# half width, for the median of the offsets: 768, 769, 2048, 2049 on both, and the smallest legal frames
GEOMETRY_SIZES = [(1536, 24), (1538, 24), (24, 1536), (24, 1538), (4096, 24), (4098, 24), (24, 4096), (24, 4098), (2, 2), (4, 20), (20, 4)]


def geometry_frame(w, h, seed=0):
    """the long side carries the walk, with a rise across 32768 and a stretch of white-edge material in it; along the long side bright pixels leave 9, 10 and 11
    of a short column's 12 samples unmasked.  -> (frame, white)"""
    wide = w >= h
    L, S = (w, h) if wide else (h, w)                       # long and short side
    hl, hs = L // 2, S // 2
    white = 32100                                            # inside the walk: stretches of it are masked, and now and then it crosses 32768
    f = walk_frame(hl, hs, 200 + seed + L, centre=32768 - 1200, step=25, noise=120).view(np.int16).astype(np.int64)
    if L >= 64:
        x = np.arange(L) // 2
        f += np.maximum(0, 1600 - 20 * np.abs(x - 2 * hl // 3))[None, :]      # a rise of 20 a pixel that takes the walk across 32768 and back
        a = hl // 3 & ~1
        f[:, 2 * a:2 * a + 64] = white_edge_frame(32, hs, 300 + seed, white).view(np.int16)
    if hs == 12:
        for k, x in enumerate(range(5, hl - 3, 11)):
            masked = 1 + k % 3                               # 11, 10, 9 samples remain
            for j in range(masked):
                y = (3 * k + 4 * j) % hs
                f[2 * y:2 * y + 2, 2 * x:2 * x + 2] = 32767 - 13 * j
    f = (f & 0xFFFF).astype(np.uint16)
    return (f if wide else np.ascontiguousarray(f.T)), white


def geometry_cases():
    out = []
    for k, (w, h) in enumerate(GEOMETRY_SIZES):
        f, white = geometry_frame(w, h, k)
        out.append(_case(f"geom_{w}x{h}", f, white, geometry=True))
    return out


def pair_flip(f, axis):
    """the frame mirrored in units of two pixels, so that every pixel stays in its Bayer plane"""
    h, w = f.shape
    if axis == 1:
        return np.ascontiguousarray(f.reshape(h, w // 2, 2)[:, ::-1, :].reshape(h, w))
    return np.ascontiguousarray(f.reshape(h // 2, 2, w)[::-1, :, :].reshape(h, w))


def batch_of(case):
    """three different frames of the case's size and white level, for a batch: the case's own, then for a geometry case two more of
    its kind from other seeds, for a content case its mirror images (left-right, then upside down)"""
    f = case["frame"]
    if case["geometry"]:
        return [f] + [geometry_frame(case["w"], case["h"], seed)[0] for seed in (50, 51)]
    return [f, pair_flip(f, 1), pair_flip(f, 0)]

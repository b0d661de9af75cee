"""Frames for the stripe analysis's histograms (csrc/k_stripes.hip), shared by tests/test_stripes_hist_cases.py (CPU: the cases are what
they are there for) and tests/test_gpu_stripes_hist.py (GPU: the device histogram is the oracle's, bin by bin).

A group is eight pixels pa..ph plus pa2, pb2 (the next group's pa, pb): pa, pb, pa2, pb2 are the reference pixels `a` of the 24
add_pixel calls (stripes.c:175-203), pc..ph the corrected pixels `b`.  A call is accepted when min(a, b) >= 32 and
max(a, b) <= white / 1.5 (values above black; stripes.c:113-117); its bin is (int)(32768 + log2(af / bf) * 32768), clamped to
0 .. 65535, with af, bf the values dithered by rand() % 1024 / 1024 - 0.5."""
import numpy as np

from mlvfs_amd import synth

# the constants of csrc/k_stripes.hip -- keep in step with it
GROUPS_PER_BLOCK = 256          # k_stripes_count: one group per lane, 256 lanes
BLOCKS_PER_QUAD = 4             # k_stripes_hist: a workgroup takes four blocks per round
SCAN_PASS = 1024                # k_scan_blocks: block totals per pass
LWIN = 8192                     # k_stripes_hist: the window of bins counted in LDS ...
LWIN_LO = 32768 - LWIN // 2     # ... is [LWIN_LO, LWIN_LO + LWIN)
RECHECK_CAP = 1 << 16           # clip.h: samples the host may have to re-bin per call
WINDOW_EDGE_BINS = (LWIN_LO - 1, LWIN_LO, LWIN_LO + LWIN - 1, LWIN_LO + LWIN)

LEVELS = [(2048, 15000), (0, 16383), (1, 10000), (2048, 2100), (8192, 60000), (16384, 65535)]
WIDTHS = [10, 11, 18, 19, 256, 266]       # no group; one; one; two, the second up to the row's last pixels; 8 k; not 8 k
SMALL_H = 128
NOTHING = ["at_31", "too_bright", "below_black", "one_call"]
SMALL_CASES = ["ratio", "flat", "threshold"] + NOTHING

# (histogram, reference pixel, corrected pixel) of the 24 calls, pixel slots 0..9 = pa..ph, pa2, pb2
CALLS = np.array([(2, 0, 2), (2, 0, 2), (2, 0, 2), (2, 8, 2), (3, 1, 3), (3, 1, 3), (3, 1, 3), (3, 9, 3),
                  (4, 0, 4), (4, 0, 4), (4, 8, 4), (4, 8, 4), (5, 1, 5), (5, 1, 5), (5, 9, 5), (5, 9, 5),
                  (6, 0, 6), (6, 8, 6), (6, 8, 6), (6, 8, 6), (7, 1, 7), (7, 9, 7), (7, 9, 7), (7, 9, 7)])


def level_id(lv):
    return f"black{lv[0]}-white{lv[1]}"


def groups_per_row(w: int) -> int:
    return (w - 10 + 7) // 8 if w > 10 else 0


def limit_of(white: int) -> int:
    """the largest value above black that add_pixel accepts: floor(white / 1.5)"""
    return int(white / 1.5)


def scale_of(black: int, white: int) -> float:
    """the 2048 / 15000 values times this stay between 32 and white / 1.5, and inside 16 bits"""
    return min(limit_of(white), 65535 - black) / 10000.0


def calls_of(f: np.ndarray, black: int, white: int):
    """MIN / MAX of stripes.c:113-117 over the 24 calls of stripes.c:175-203, restated: (a, b, accepted), each of shape
    (rows, groups, 24) in the order the reference makes the calls"""
    h, w = f.shape
    gpr = groups_per_row(w)
    v = f.astype(np.int64) - black
    x = (np.arange(gpr) * 8)[:, None] + np.arange(10)[None, :]
    px = v[:, x] if gpr else np.zeros((h, 0, 10), np.int64)
    a, b = px[:, :, CALLS[:, 1]], px[:, :, CALLS[:, 2]]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return a, b, ~(lo < 32) & ~(hi.astype(np.float64) > white / 1.5)


def positions_of(f: np.ndarray, black: int, white: int, rnd: np.ndarray):
    """(histogram, r1, r2, 32768 + log2(af / bf) * 32768) of the accepted calls in raster order; rnd: rand() % 1024, two per call"""
    a, b, ok = calls_of(f, black, white)
    n = int(ok.sum())
    r1, r2 = rnd[0:2 * n:2].astype(np.int64), rnd[1:2 * n:2].astype(np.int64)
    af, bf = a[ok] + r1 / 1024.0 - 0.5, b[ok] + r2 / 1024.0 - 0.5
    j = np.broadcast_to(CALLS[:, 0], ok.shape)[ok]
    return j, r1, r2, 32768 + np.log2(af / bf) * 32768


def _to_u16(v, black):
    v = np.asarray(v, np.int64) + black
    assert v.min() >= 0 and v.max() <= 65535
    return np.ascontiguousarray(v.astype(np.uint16))


def ratio_frame(w: int, h: int, black: int, white: int) -> np.ndarray:
    """log2(a / b) where the bins are interesting, by row: +0.125 EV and -0.125 EV (the two ends of the LDS window: 32768 +/- 4096),
    ratio 2 and ratio 1 / 2 (the clamp to bins 65535 and 0).  The smaller value steps with the group index around the exact ratio, so
    that samples fall on both sides of each edge."""
    s = scale_of(black, white)
    big, two = int(9000 * s), int(4000 * s)
    near, half = int(round(big / 2 ** 0.125)), two // 2
    k1, k2 = max(1, int(round(10 * s))), max(1, int(round(4 * s)))
    y, x = np.mgrid[0:h, 0:w]
    g = x // 8 + 3 * (y // 4)
    ref = (x % 8) < 2                                             # pa, pb (and pa2, pb2 of the group before)
    small = near + g % (2 * k1 + 1) - k1
    halved = half + g % (2 * k2 + 1) - k2
    layouts = [np.where(ref, big, small), np.where(ref, small, big), np.where(ref, two, halved), np.where(ref, halved, two)]
    v = np.choose(y % 4, layouts)
    assert v.min() >= 32 and v.max() <= white / 1.5
    return _to_u16(v, black)


def flat_value(black: int, white: int) -> int:
    return black + min(1000, limit_of(white))


def flat_frame(w: int, h: int, black: int, white: int) -> np.ndarray:
    """one value, accepted everywhere: a call whose two dither values are equal has af / bf == 1, exactly on the edge of bin 32768"""
    return np.full((h, w), flat_value(black, white), np.uint16)


def threshold_frame(w: int, h: int, black: int, white: int, seed: int = 1) -> np.ndarray:
    """pixels at 31, 32, floor(white / 1.5) and one more above black, below black (at black 0: at it), and ordinary ones"""
    rng = np.random.default_rng(seed)
    top = limit_of(white)
    kind = rng.integers(0, 12, (h, w))
    ordinary = rng.integers(32, top + 1, (h, w))
    below = -rng.integers(1, 301, (h, w)) if black else np.zeros((h, w), np.int64)
    v = np.choose(np.minimum(kind, 5), [np.full((h, w), 31), np.full((h, w), 32), np.full((h, w), top), np.full((h, w), top + 1),
                                        np.maximum(below, -black), ordinary])
    return _to_u16(v, black)


def deciding_values(f: np.ndarray, black: int, white: int):
    """calls decided by min == 31 (refused), min == 32 (accepted), max == floor(white / 1.5) (accepted), max one above (refused by
    the maximum alone)"""
    a, b, ok = calls_of(f, black, white)
    lo, hi, top = np.minimum(a, b), np.maximum(a, b), limit_of(white)
    return {"min31": int(((lo == 31) & ~ok).sum()), "min32": int(((lo == 32) & ok).sum()),
            "max_at": int(((hi == top) & ok).sum()), "max_above": int(((hi == top + 1) & (lo >= 32) & ~ok).sum())}


def nothing_frame(name: str, w: int, h: int, black: int, white: int) -> np.ndarray:
    """frames on which no call is accepted; 'one_call': exactly one (pa2 / pc of a row's last group: stripes.c:178)"""
    if name == "at_31":
        return np.full((h, w), black + 31, np.uint16)
    if name == "too_bright":
        return np.full((h, w), black + limit_of(white) + 1, np.uint16)
    if name == "below_black":
        return np.full((h, w), black - min(black, 100), np.uint16)
    assert name == "one_call"
    f = np.full((h, w), black + 31, np.uint16)
    gpr = groups_per_row(w)
    if gpr:
        x = 8 * (gpr - 1)
        f[h // 2, x + 8] = f[h // 2, x + 2] = black + 32
    return f


def expected_calls(name: str, w: int) -> int:
    return 1 if name == "one_call" and groups_per_row(w) else 0


def small_case(name: str, w: int, black: int, white: int, h: int = SMALL_H) -> np.ndarray:
    if name == "ratio":
        return ratio_frame(w, h, black, white)
    if name == "flat":
        return flat_frame(w, h, black, white)
    if name == "threshold":
        return threshold_frame(w, h, black, white, seed=w)
    return nothing_frame(name, w, h, black, white)


# ------------------------------------------------------------------ the long geometry
LONG_W = 2070                    # 258 groups per row, not a multiple of 8
LONG_BANDS = {"flat": (300, 316), "dark": (700, 706)}      # rows; the ratio band: the eight rows before the last four


def long_properties(w: int, h: int, cus: int) -> dict:
    n_groups = groups_per_row(w) * h
    nblk = -(-n_groups // GROUPS_PER_BLOCK)
    quads = -(-nblk // BLOCKS_PER_QUAD)
    return dict(n_groups=n_groups, nblk=nblk, quads=quads,
                three_passes_last_ragged=nblk > 2 * SCAN_PASS and nblk % SCAN_PASS != 0,
                third_round_for_some=quads > 2 * cus and quads % cus != 0,
                ragged_quad=nblk % BLOCKS_PER_QUAD != 0,
                ragged_block=n_groups % GROUPS_PER_BLOCK != 0)


def long_geometry(cus: int):
    """The smallest frame of width 2070 on which, on a device of `cus` compute units, k_scan_blocks makes three passes with a ragged last
    one, the workgroups of k_stripes_hist (one per compute unit) run a third round and the last round is not for all of them, the
    last quad has sub-blocks past the last block, and the last block has lanes past the last group."""
    w = LONG_W
    for h in range(1, 1 << 14):
        p = long_properties(w, h, cus)
        if all(p[k] for k in ("three_passes_last_ragged", "third_round_for_some", "ragged_quad", "ragged_block")):
            break
    p = long_properties(w, h, cus)
    assert p["nblk"] > 2 * SCAN_PASS and p["nblk"] % SCAN_PASS != 0, p           # 1: three passes, the last ragged
    assert p["quads"] > 2 * cus and p["quads"] % cus != 0, p                     # 2: a third round, the last one not for everyone
    assert p["nblk"] % BLOCKS_PER_QUAD != 0, p                                   # 3
    assert p["n_groups"] % GROUPS_PER_BLOCK != 0, p                              # 4
    return w, h


def long_frame(w: int, h: int, black: int = synth.BLACK, white: int = synth.WHITE) -> np.ndarray:
    """normal_frame with a flat band (recheck volume), a band below black + 32 (blocks whose total is 0, groups without calls between
    accepted ones) and a band of ratio_frame"""
    f = synth.normal_frame(w, h, black=black).copy()
    r0, r1 = LONG_BANDS["flat"]
    f[r0:r1] = flat_value(black, white)
    r0, r1 = LONG_BANDS["dark"]
    f[r0:r1] = black + 20 + (np.arange(w) % 12)[None, :]
    f[h - 12:h - 4] = ratio_frame(w, 8, black, white)
    return f

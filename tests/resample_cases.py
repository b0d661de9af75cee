"""Rendered frames resampled from the full-size rendering (include/mlvfs_amd.h, "rendered frames resampled from the full-size
rendering"): the cases the CPU and GPU tests share.  The definition itself is mlvfs_amd/resample.py.  The parameter
sets and content generators are those of tests/demosaic_cases.py (every batch of three holds both matrix paths); this module adds the
sizes, the white frames and the wrong definitions the cases have to tell from the right one.  tests/test_resample_cases.py proves
that the cases are not vacuous."""
import numpy as np

from mlvfs_amd import demosaic, render, scale

import demosaic_cases as dc
import scale_cases as sc

# k_resample_x16 (csrc/clip.h, pinned by tests/test_resample_cases.py through mlvfs_amd_test_resample_plan): the most source columns of
# a strip, the source rows a band covers at least, the source rows of a step
STRIP, BAND_ROWS, ROWS = 512, 32, 4

# (width, height) for mlvfs_amd_render_resampled_dev: the smallest frame, odd sizes, the smallest fast shape; fast shapes of one
# workgroup and one with several steps; an odd size that takes the generic form only; two that cross strips (one with a band seam);
# many bands; the widest the fast form takes
SOURCES = [(4, 4), (5, 4), (7, 5), (16, 4), (32, 8), (48, 6), (96, 34), (418, 267), (528, 65), (1040, 6), (16, 600), (65520, 4)]
WHITE = [(65520, 4), (65535, 4)]                   # the widest fast frame, and the widest there is (generic): the largest sum
MOUNT_SIZES = dc.MOUNT_SIZES
BIG_W, BIG_H = dc.BIG_W, dc.BIG_H
BIG_SIZES = [(1920, 707), (2560, 943)]


def out_sizes(w, h):
    """the output sizes of one source: the identity, one less a side, one more than the half size, the 3 : 2 ratio where it divides,
    the full width at a third of the height, a full row, a full column, one pixel, and one size below half the width -- each once"""
    sizes = [(w, h), (w - 1, h - 1), (w // 2 + 1, h // 2 + 1)]
    if w % 3 == 0 and h % 3 == 0:
        sizes.append((2 * w // 3, 2 * h // 3))
    sizes += [(w, (h + 2) // 3), (w, 1), (1, h), (1, 1), (max(1, (w - 1) // 2 - 1), max(1, h // 2))]
    return list(dict.fromkeys(sizes))


def takes_fast(w, ow):
    return w % 16 == 0 and 2 * ow >= w


# (frames, source offset, destination offset, aligned strides) per output size, cycling: k_resample_x16 (where the sizes allow it) and
# k_resample_generic take turns, in batches of 1 and 3
PLACEMENTS = [(3, 0, 0, True), (3, 2, 3, False), (1, 16, 1, True), (1, 2, 0, False)]


def dev_cases(w, h):
    """what tests/test_gpu_resample.py runs at one source size: [(ow, oh, frames with parameters, src_off, dst_off, aligned)].  Every
    output size runs through an aligned placement (the fast form where the sizes allow it) and a misaligned one (generic)."""
    out, first = [], (w * 7 + h) % 11
    for k, (ow, oh) in enumerate(out_sizes(w, h)):
        for n, src_off, dst_off, aligned in (PLACEMENTS[2 * (k % 2)], PLACEMENTS[2 * (k % 2) + 1]):
            out.append((ow, oh, dc.batch(w, h, n, first), src_off, dst_off, aligned))
            first += 1
    return out


def white_cases(w, h):
    """a white frame (every d_c = 65535) stays at 65535 at every size: sc.white_cases' frame and probes -- each channel in turn probed at
    65535 (byte 1) -- at the identity, one less a side, a full row and one pixel.  The horizontal sum of the one-pixel size is 65535 W."""
    sizes = [(w, h), (w - 1, h - 1), (w, 1), (1, 1)]
    return [(f, p, ow, oh, byte) for f, p, _, _, byte in sc.white_cases(w, h) for ow, oh in sizes]


def extreme_sets():
    """black at both ends of its type and below zero, A at its cap, the largest K a forward matrix of shorts can give, K at the ends of
    int32, and all zero"""
    import render_cases as rc
    big_k = render.params(0, 65535, (1, 1) * 3, (32767, -32768, 32767) * 3, 256)[4:]
    end_k = [(1 << 31) - 1, -(1 << 31), (1 << 31) - 1, -(1 << 31), (1 << 31) - 1, -(1 << 31), -(1 << 31), -(1 << 31), (1 << 31) - 1]
    return [[-(1 << 31), 1, 3, 2] + rc.param_set(0)[1][4:], [(1 << 31) - 1, 5, 5, 5] + rc.param_set(1)[1][4:],
            [-5000, render.A_MAX, 70000, 1 << 20] + rc.param_set(2)[1][4:], [100, 4000, 4100, 4200] + big_k,
            [65535, render.A_MAX, render.A_MAX, render.A_MAX] + big_k, [2048, 20000, 9000, 14000] + end_k, [0, 0, 0, 0] + [0] * 9]


# ---- the wrong definitions
def _avg(a, n_out, how):
    """scale.average with the division done wrong: "trunc" without the rounding term, "down" with a half rounded down, an int: that
    divisor in the place of the length"""
    a = np.asarray(a, np.int64)
    n = a.shape[-1]
    s = scale.weights(n, n_out) @ a[..., None]
    s = s[..., 0]
    if how == "trunc":
        return s // n
    if how == "down":
        return (s + ((n - 1) >> 1)) // n
    return (s + (how >> 1)) // how


def wrong(kind, frame, p, ow, oh, lut):
    """the rendering under one of the wrong definitions: trunc, down, 2d (one division by W H), early (averaged before step 2's clamp),
    late (averaged after the matrix), clamp (the edge-repeat border), half (W' and H' as divisors)"""
    st = demosaic.stages(frame, p, "clamp" if kind == "clamp" else "reflect")
    d = st["n"]
    h, w = frame.shape
    K = p[4:13]
    both = lambda a, hx, hy: _avg(_avg(a, ow, hx).transpose(0, 2, 1), oh, hy).transpose(0, 2, 1)
    if kind in ("trunc", "down"):
        m = both(d, kind, kind)
    elif kind == "half":
        m = np.minimum(both(d, w // 2, h // 2), 65535)
    elif kind == "2d":
        s = np.einsum("vy,cyx,ux->cvu", scale.weights(h, oh), d, scale.weights(w, ow))
        m = (s + (w * h >> 1)) // (w * h)
    elif kind == "early":
        m = np.clip(_signed_average((st["s"] + 8) >> 4, ow, oh), 0, 65535)
    elif kind == "late":
        acc = np.stack([sum(np.int64(K[3 * i + j]) * d[j] for j in range(3)) for i in range(3)])
        acc = _signed_average(acc, ow, oh)
        return render.tone(np.clip((acc + 32768) >> 16, 0, 4095), lut)
    else:
        m = scale.average(scale.average(d, ow).transpose(0, 2, 1), oh).transpose(0, 2, 1)        # clamp: only the source differs
    acc = np.stack([sum(np.int64(K[3 * i + j]) * m[j] for j in range(3)) for i in range(3)])
    return render.tone(np.clip((acc + 32768) >> 16, 0, 4095), lut)


def _signed_average(a, ow, oh):
    """the two passes on values of either sign (Python's floor division)"""
    a = np.asarray(a, np.int64)
    one = lambda b, n_out: ((scale.weights(b.shape[-1], n_out) @ b[..., None])[..., 0] + (b.shape[-1] >> 1)) // b.shape[-1]
    return one(one(a, ow).transpose(0, 2, 1), oh).transpose(0, 2, 1)


WRONG = ("trunc", "down", "2d", "early", "late", "clamp", "half")


def params_array(ps):
    return sc.params_array(ps)

"""Rendered frames at 16 bits (include/mlvfs_amd.h, "rendered frames at 16 bits"): the cases the CPU and GPU tests
share.  The definition itself is mlvfs_amd/look.py (stages16, apply16) behind render.py, demosaic.py and scale.py.  The triples, the
shaper values and the tables are those of tests/look_cases.py; the frames, levels and parameters those of tests/render_cases.py,
tests/demosaic_cases.py and tests/scale_cases.py.  tests/test_deep_cases.py proves that the cases reach what they claim and that each of
six wrong definitions changes some sample of them."""
import numpy as np

from mlvfs_amd import demosaic, look, render, scale

import demosaic_cases as dc
import look_cases as lc
import render_cases as rc
import scale_cases as sc

NS = (0, 2, 3, 65)


def case_shaper16(seed=0):
    """65536 random 16-bit values -- not monotone --, the first len(lc.U) of them lc.U: index k < len(lc.U) reads lc.U[k], so
    lc.case_triples() reach here what they reach behind lc.case_shaper()"""
    S = np.random.default_rng(7500 + seed).integers(0, 65536, 65536, dtype=np.uint16)
    S[:len(lc.U)] = lc.U
    return S


def random_triples16(count=100000, seed=0):
    return np.random.default_rng(7600 + seed).integers(0, 65536, (3, count), dtype=np.int64)


def looks():
    """[(name, S16, N, T)]: no table behind the identity (the file holds t), behind a constant and behind the case shaper; a random table
    at N = 2, 3 and 65 behind the case shaper; look_cases' edge table; a random 17^3 table behind the sRGB shaper"""
    out = [("linear0", look.shaper16_linear(), 0, None),
           ("const0", np.full(65536, 12345, np.uint16), 0, None),
           ("case0", case_shaper16(0), 0, None)]
    out += [(f"random{n}", case_shaper16(n), n, lc.random_table(n)) for n in NS if n]
    out.append(("edge2", case_shaper16(1), 2, lc.edge_table()))
    out.append(("srgb17", look.shaper16_srgb(), 17, lc.random_table(17)))
    return out


def look_of(name):
    return next(l[1:] for l in looks() if l[0] == name)


# ---- frames.  (width, height, frames, source offset, destination offset, aligned strides) for mlvfs_amd_render2_deep_dev.
# k_render2_deep_x16 takes W % 16 == 0 with the source and the destination on 16-byte boundaries: one group; two groups a row, two rows;
# three frames at padded strides.  k_render2_deep_generic takes the rest: the smallest frame; an odd row and column that are never
# read; a width that is no multiple of 16, three frames; the fast shape with the source off a 16-byte boundary; the fast shape with the
# destination 8 bytes off one (enough for the 8-bit x16 kernel, not for this one)
HALF_FAST = [(16, 2, 1, 0, 0, True), (32, 4, 1, 0, 0, True), (48, 6, 3, 16, 16, True)]
HALF_GENERIC = [(2, 2, 1, 0, 0, True), (3, 3, 1, 0, 0, True), (18, 6, 3, 0, 0, True), (32, 4, 1, 2, 0, True), (32, 4, 1, 0, 8, True)]
# per size of tests/demosaic_cases.py and per output size of tests/scale_cases.py: (frames, source offset, destination offset, aligned
# strides).  The first two take the x16 kernel where the width allows it, the others the generic one: a destination 8 bytes off (an
# odd one for the scaled route, whose x16 kernel stores 16-bit values), and everything odd
FULL_PLACEMENTS = [(3, 0, 0, True), (1, 16, 16, True), (1, 0, 8, True), (3, 2, 3, False)]
SCALED_PLACEMENTS = [(3, 0, 0, True), (1, 16, 2, True), (1, 0, 1, True), (3, 2, 3, False)]


def batch(w, h, n, first):
    """rc.batch with the second frame of three on demosaic_cases' wide parameters, whose matrix does not fit 32 bits, and single frames
    on them every third time: both matrix paths of k_render1_deep_x16 and k_scale_deep_x16, in one launch and alone"""
    b = rc.batch(w, h, n, first)
    if n == 3:
        b[1] = (b[1][0], dc.wide_param_set(first + 1)[1])
    elif first % 3 == 1:
        b[0] = (b[0][0], dc.wide_param_set(first)[1])
    return b


def _names():
    return [l[0] for l in looks()]


def rounding_frame():
    """16 x 2 with black = 0, A = 4096 and K the unit matrix in Q0 (1, not 4096): acc_i is the raw value of channel i, so step 3d's
    rounding is met from both sides by construction -- 2047 | 2048 (t = 0 | 1: (acc + 2048) & 4095 = 4095 | 0) and 6143 | 6144 --
    and t16 is (raw + 2048) >> 12"""
    f = np.zeros((2, 16), np.uint16)
    f[0, 0::2] = [2047, 2048, 6143, 6144, 0, 65535, 2046, 2049]                  # R
    f[0, 1::2] = f[1, 0::2] = [6144, 6143, 2048, 2047, 65535, 0, 10239, 10240]  # both greens alike
    f[1, 1::2] = [2048, 2047, 6144, 6143, 4096, 4095, 63487, 63488]             # B
    return f, [0, 4096, 4096, 4096, 1, 0, 0, 0, 1, 0, 0, 0, 1]


def half_cases():
    """[(frames with parameters, src_off, dst_off, aligned, look name)]: the shapes above with a look each, and the rounding frame as
    a linear file through both kernels"""
    names = _names()
    out = [(batch(w, h, n, k), so, do, al, names[k % len(names)]) for k, (w, h, n, so, do, al) in enumerate(HALF_FAST + HALF_GENERIC)]
    return out + [([rounding_frame()], 0, 0, True, "linear0"), ([rounding_frame()], 0, 8, True, "linear0")]


def full_cases(w, h):
    names, first = _names(), (w * 7 + h) % 11
    return [(batch(w, h, n, first + k), so, do, al, names[(first + k) % len(names)]) for k, (n, so, do, al) in enumerate(FULL_PLACEMENTS)]


def scaled_cases(w, h):
    """[(ow, oh, frames with parameters, src_off, dst_off, aligned, look name)]: every output size of scale_cases through an x16
    placement and a generic one"""
    names, out = _names(), []
    for k, (ow, oh) in enumerate(sc.out_sizes(w, h)):
        for j in (k % 2, 2 + k % 2):
            n, so, do, al = SCALED_PLACEMENTS[j]
            out.append((ow, oh, batch(w, h, n, 2 * k + j), so, do, al, names[(k + j + w) % len(names)]))
    return out


def stages(route, f, p, size=None):
    """the route's stages(): 2 half size, 1 full size, 0 scaled to `size`"""
    if route == 2:
        return render.stages(f, p)
    if route == 1:
        return demosaic.stages(f, p)
    return scale.stages(f, p, size[0], size[1])


def definition(route, f, p, look16, size=None):
    """(oh, ow, 3) uint16"""
    return render.develop(stages(route, f, p, size), look16=look16)


def file_bytes(samples):
    """the samples as the file holds them: little-endian, R, G, B"""
    return np.ascontiguousarray(samples).astype("<u2").tobytes()


# ---- the wrong definitions: each must change some sample of the cases
WRONG = ("shl4", "no_rounding", "round32768", "shaper_shr4", "step4d", "big_endian")


def wrong(kind, st, S, n, T):
    """steps 3d and 4 done wrongly in one respect on a stages() result: the file's bytes"""
    acc, t16 = st["acc"], st["t16"]
    if kind == "shl4":                                           # the 8-bit routes' index, widened
        return file_bytes(render.tone16(st["t"] << 4, (S, n, T)))
    if kind == "no_rounding":
        return file_bytes(render.tone16(np.clip(acc >> 12, 0, 65535), (S, n, T)))
    if kind == "round32768":                                     # the 8-bit routes' rounding term kept
        return file_bytes(render.tone16(np.clip((acc + 32768) >> 12, 0, 65535), (S, n, T)))
    if kind == "shaper_shr4":                                    # a 4096-entry shaper's indexing
        return file_bytes(render.tone16(t16 >> 4, (S, n, T)))
    if kind == "step4d":
        return file_bytes((render.tone16(t16, (S, n, T)).astype(np.int64) + 128) // 257)
    if kind == "big_endian":
        return np.ascontiguousarray(render.tone16(t16, (S, n, T))).astype(">u2").tobytes()
    raise ValueError(kind)

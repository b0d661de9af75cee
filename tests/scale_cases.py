"""Rendered frames at any smaller size (include/mlvfs_amd.h, "rendered frames at any smaller size"): the cases the CPU
and GPU tests share.  The definition itself is mlvfs_amd/scale.py.  The parameter sets and content generators are those of
tests/render_cases.py; this module adds the sizes, and frames whose averages are known by construction.  tests/test_scale_cases.py
proves that the cases are not vacuous."""
import numpy as np

import render_cases as rc

# k_scale_x16 (csrc/clip.h, pinned by tests/test_scale_cases.py through mlvfs_amd_test_scale_plan): the superpixels of a source row a
# step stages, the most output columns of a strip, and the source rows a band of output rows covers at least
CHUNK, STRIP, BAND_ROWS = 1024, 1024, 8

# (width, height) for mlvfs_amd_render_scaled_dev, the smallest at which each mechanism can fail: two fast shapes of one workgroup;
# one with bands of more than one output row; an odd size the fast form does not take; several strips; several bands; the widest
# grid the fast form takes (W' = 65528) and the widest there is (65535, generic), where one column's span is 64 chunks; the tallest
SOURCES = [(32, 8), (48, 6), (96, 34), (418, 267), (4112, 8), (16, 600), (131056, 2), (131070, 2), (2, 131070)]
MOUNT_SIZES = rc.MOUNT_SIZES
BIG_W, BIG_H = rc.BIG_W, rc.BIG_H


def out_sizes(w, h):
    """the output sizes of one source: the identity, one pixel, one less a side, the integer ratios 2 and 3 where they divide, 7x5,
    a full row and a full column -- in that order, each once"""
    pw, ph = w // 2, h // 2
    sizes = [(pw, ph), (1, 1), (max(pw - 1, 1), max(ph - 1, 1))]
    for r in (2, 3):
        if pw % r == 0 and ph % r == 0:
            sizes.append((pw // r, ph // r))
    sizes += [(min(7, pw), min(5, ph)), (pw, 1), (1, ph)]
    return list(dict.fromkeys(sizes))


# (frames, source offset, destination offset, aligned strides) per output size, cycling: k_scale_x16 (where the width allows it) and
# k_scale_generic take turns, in batches of 1 and 3
PLACEMENTS = [(3, 0, 0, True), (3, 2, 3, False), (1, 16, 1, True), (1, 2, 0, False)]


def dev_cases(w, h):
    """what tests/test_gpu_scale.py runs at one source size: [(ow, oh, frames with parameters, src_off, dst_off, aligned)].  Every
    output size runs through both forms: an aligned placement (the fast form where w % 16 == 0) and a misaligned one (generic)."""
    out, first = [], 0
    for k, (ow, oh) in enumerate(out_sizes(w, h)):
        for n, src_off, dst_off, aligned in (PLACEMENTS[2 * (k % 2)], PLACEMENTS[2 * (k % 2) + 1]):
            out.append((ow, oh, rc.batch(w, h, n, first), src_off, dst_off, aligned))
            first += 1
    return out


# ---- frames whose balanced channels are known: with black = 0 and A = 4096, n_j is the raw value (both greens alike)
def frame_from_n(n):
    """(3, H', W') values 0 .. 65535 -> the (2 H', 2 W') RGGB frame whose n, with unit parameters, they are"""
    n = np.asarray(n)
    f = np.zeros((2 * n.shape[1], 2 * n.shape[2]), np.uint16)
    f[0::2, 0::2], f[0::2, 1::2], f[1::2, 0::2], f[1::2, 1::2] = n[0], n[1], n[1], n[2]
    return f


def probe_params(j, at):
    """13 parameters under which every output byte is 1 where m_j >= at and 0 below, given that channel (j + 1) % 3 holds
    probe_level(at) everywhere: black 0, A = 4096, every row of K the same -- +1 for channel j and +-1 for the constant one, so that
    acc + 32768 reaches 65536 exactly at m_j = at -- and LUT[0] = 0, LUT[1] = 1.  Two probes, at E and at E + 1, pin m_j = E."""
    assert 0 <= at <= 65536
    row = [0, 0, 0]
    row[j], row[(j + 1) % 3] = 1, -1 if at >= 32768 else 1
    return [0, 4096, 4096, 4096] + row * 3


def probe_level(at):
    return abs(at - 32768)


def probe_frame(line, j, at, vertical=False):
    """a frame one superpixel deep (or, vertical, one wide) whose channel j is `line` and whose channel (j + 1) % 3 is
    probe_level(at) everywhere"""
    line = np.asarray(line, np.int64)
    n = np.zeros((3, 1, len(line)), np.int64)
    n[j, 0], n[(j + 1) % 3, 0] = line, probe_level(at)
    return frame_from_n(n.transpose(0, 2, 1) if vertical else n)


def remainder_line(d, q, r):
    """d values whose sum is q d + r: q everywhere, q + 1 at r places spread over the line"""
    line = np.full(d, q, np.int64)
    line[(np.arange(r) * d) // max(r, 1)] += 1
    assert line.sum() == q * d + r
    return line


# (divisor, quotient, remainder, the average the definition gives): the remainder exactly the half (an even divisor only: it rounds
# up), one below it and one above it, for an even and an odd divisor; the quotient once small and once at the top of the 16 bits.
# The divisors are W' (horizontal: a (2 d) x 2 frame to 1 x 1) and H' (vertical: a 16 x (2 d) frame to 8 x 1, 2 x (2 d) to 1 x 1).
ROUNDING = [(d, q, r, q + (1 if r + (d >> 1) >= d else 0))
            for d in (8, 24, 5, 11, 300) for q in (7, 65534) for r in sorted({0, (d >> 1) - 1, d >> 1, (d >> 1) + 1, d - 1})]


def rounding_cases():
    """[(frame, 13 parameters, ow, oh, the byte every output holds)]: each entry of ROUNDING horizontally and vertically, on each
    channel in turn, probed at the expected average (byte 1) and one above it (byte 0).  Widths of 16 and 48 take the fast form."""
    out = []
    for k, (d, q, r, want) in enumerate(ROUNDING):
        j = k % 3
        for at, byte in ((want, 1), (want + 1, 0)):
            line = remainder_line(d, q, r)
            out.append((probe_frame(line, j, at), probe_params(j, at), 1, 1, byte))
            out.append((probe_frame(line, j, at, vertical=True), probe_params(j, at), 1, 1, byte))
            wide = np.tile(probe_frame(line, j, at, vertical=True), (1, 8))                  # 16 wide: the fast form, 8 columns
            out.append((wide, probe_params(j, at), 8, 1, byte))
    return out


def half_case(a, j=0):
    """two source values a and a + 1 averaged 1 : 1 give a + 1: (frame 32 x 2, parameters, ow, oh, byte) probed at a + 1 and a + 2"""
    line = np.tile([a, a + 1], 8)
    return [(probe_frame(line, j, at), probe_params(j, at), 8, 1, byte) for at, byte in ((a + 1, 1), (a + 2, 0))]


def white_cases(w, h):
    """a white frame (every n_j = 65535) to 1 x 1 stays at 65535: each channel in turn probed at 65535 (byte 1); the sum of the
    widest span, 65535 * 65535 + 32767, is the largest a 32-bit accumulator has to hold"""
    f = np.full((h, w), 65535, np.uint16)
    out = []
    for j in range(3):
        # channel (j + 1) % 3 balanced to 65535 - 32768 by its A: c' = 1 with black = 65534, n = (A + 2048) >> 12
        A = [65535 << 12] * 3
        A[(j + 1) % 3] = probe_level(65535) << 12
        out.append((f, [65534] + A + probe_params(j, 65535)[4:], 1, 1, 1))
    return out


def constant_frame(w, h, c):
    return np.full((h, w), c, np.uint16)


def params_array(ps):
    return rc.params_array(ps)

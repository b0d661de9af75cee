"""Rendered half-size sRGB frames: the cases of tests/render_cases.py are not vacuous, and the committed table is the curve (no GPU,
no library).  Over the cases tests/test_gpu_render.py runs, every clamp of the definition (mlvfs_amd/render.py) acts and every branch
of its rounding is taken."""
import os

import numpy as np

from mlvfs_amd import render

import render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "srgb_lut12.bin")


def all_cases():
    for w, h in rc.SIZES:
        for frames, _, _, _ in rc.dev_cases(w, h):
            yield from frames


def test_the_cases_reach_every_clamp_and_rounding():
    below_black = n_clipped = acc_negative = t_top = odd = even = 0
    seen = np.zeros(4096, bool)
    for frame, p in all_cases():
        s = render.stages(frame, p)
        h, w = frame.shape
        q = frame[:h // 2 * 2, :w // 2 * 2].astype(np.int64)
        below_black += int((q < p[0]).sum())
        assert ((s["c"] == 0) >= (np.stack([q[0::2, 0::2], (s["green_sum"] + 1) >> 1, q[1::2, 1::2]]) <= p[0])).all()
        for j in range(3):
            raw = (s["c"][j] * np.int64(p[1 + j]) + 2048) >> 12
            n_clipped += int((raw > 65535).sum())
        acc_negative += int(((s["acc"] + 32768) >> 16 < 0).sum())
        t_top += int(((s["acc"] + 32768) >> 16 > 4095).sum())
        odd += int((s["green_sum"] & 1).sum())
        even += int((~s["green_sum"] & 1).sum())
        seen[s["t"].ravel()] = True
    assert below_black > 1000 and n_clipped > 1000 and acc_negative > 1000 and t_top > 1000 and odd > 1000 and even > 1000
    assert seen.sum() >= 1000, int(seen.sum())
    assert seen[0] and seen[4095]


def test_the_parameter_sets_differ_by_channel_and_frame():
    sets = [rc.param_set(k)[1] for k in range(14)]
    assert any(len({p[1], p[2], p[3]}) == 3 for p in sets), "no neutral with three different A"
    assert len({tuple(p) for p in sets}) == len(sets)
    assert len({tuple(p[4:]) for p in sets}) == len(rc.FORWARD)
    for p in sets:
        assert all(-(1 << 31) <= v < (1 << 31) for p_ in sets for v in p_)
        assert any(v < 0 for v in p[4:]), "a matrix without a negative entry cannot drive acc below 0"
    # a batch of three never repeats a parameter set
    for frames, _, _, _ in rc.dev_cases(16, 4):
        assert len({tuple(p) for _, p in frames}) == len(frames)


def test_render_reads_no_odd_last_column_or_row():
    (black, white), p = rc.param_set(2)
    f = rc.range_frame(7, 5, black, white)
    g = f.copy()
    g[4, :] = 0xFFFF
    g[:, 6] = 0
    assert np.array_equal(render.render(f, p), render.render(g, p)) and render.render(f, p).shape == (2, 3, 3)


def test_unity_balance_of_a_grey_frame_is_grey():
    """a frame at (black + white) / 2 under a unit neutral: n = 32768 in every channel, and a forward matrix's rows sum to D50 white,
    which S takes to equal R, G and B within the rounding of K"""
    p = render.params(2048, 15000, (1, 1) * 3, rc.FORWARD[0], 256)
    f = np.full((4, 4), 2048 + (15000 - 2048) // 2, np.uint16)
    s = render.stages(f, p)
    assert (np.abs(s["n"] - 32768) <= 4).all()
    assert np.ptp(s["t"]) <= 2 and abs(int(s["t"][1, 0, 0]) - 2048) <= 4


def test_the_golden_table_is_the_curve():
    lut = np.fromfile(GOLDEN, np.uint8)
    assert lut.size == 4096
    curve = render.srgb_curve12()
    assert np.array_equal(lut, np.floor(curve + 0.5).astype(np.uint8)) and np.array_equal(lut, render.srgb_lut12())
    # no entry hangs on a libm: the curve stays clear of every rounding boundary
    assert np.abs(curve - np.floor(curve) - 0.5).min() > 1e-9
    assert (np.diff(lut.astype(np.int32)) >= 0).all() and lut[0] == 0 and lut[4095] == 255
    assert len(np.unique(lut)) == 256


def test_the_header_array_holds_the_same_bytes():
    text = open(os.path.join(ROOT, "mlvfs_amd", "csrc", "srgb_lut12.h")).read()
    body = text[text.index("{") + 1:text.rindex("}")]
    values = [int(v) for v in body.replace("\n", " ").split(",") if v.strip()]
    assert bytes(values) == open(GOLDEN, "rb").read()

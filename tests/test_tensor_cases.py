"""The tensor pass's cases on the CPU (tests/tensor_cases.py; the GPU runs them in tests/test_gpu_tensor.py): the cases reach what they
claim -- every byte value, the 16-bit samples 0, 1, 2, 3 and 65535, half results that are subnormal, that tie to even in both directions
and that overflow, bfloat16 ties in both directions, negative px - black and px above white, both parities of a mixed clip's levels, both
forms at shapes either could take -- and each wrong definition (a fused multiply-add, unit * scale folded, truncation for half and for
bfloat16, subnormal halves flushed, B, G, R order, G1 and G2 swapped, the layouts exchanged, Bayer clamped at black) differs from the
definition on at least one of them.  The definition's two conversions are also checked against torch's on the CPU.  No GPU."""
import numpy as np
import pytest

from mlvfs_amd import tensor as T

import tensor_cases as tc

RGB, BAYER = tc.rgb_cases(), tc.bayer_cases()
ALL = RGB + BAYER


def f32_values(case, k):
    """the definition's binary32 values of frame k, (h, w, C)"""
    data = tc.frames(case)[k]
    scale, bias = tc.scale_bias(case)
    if case["kind"] == T.RGB:
        return T.f32_value(data.astype(np.int64), T.unit_of(case["bits"]), scale, bias)
    black, _, unit = T.bayer_levels(*tc.levels(case)[k])
    return T.f32_value(T.bayer_planes(data).astype(np.int64) - black, unit, scale, bias)


def all_values(dtype):
    return np.concatenate([f32_values(c, k).reshape(-1) for c in ALL if c["dtype"] == dtype for k in range(c["n"])])


def test_the_case_lists_cover_every_size_dtype_layout_and_form():
    assert {(c["w"], c["h"]) for c in RGB} == set(tc.RGB_SIZES) and {(c["w"], c["h"]) for c in BAYER} == set(tc.BAYER_SIZES)
    for cases, depths in ((RGB, (8, 16)), (BAYER, (16,))):
        for bits in depths:
            legal = [d for d in (T.F32, T.F16, T.BF16, T.U8, T.U16) if T.legal(d, bits)]
            assert len(legal) == 4
            for w, h in {(c["w"], c["h"]) for c in cases}:
                got = {(c["dtype"], c["layout"], c["n"], c["aligned"]) for c in cases if (c["w"], c["h"], c["bits"]) == (w, h, bits)}
                assert got == {(d, ly, n, a) for d in legal for ly in (T.NCHW, T.NHWC) for n, a in ((1, True), (3, True), (3, False), (1, False))}
    # both forms run at shapes either could take, and the narrow shapes never take the fast one
    for cases, mult in ((RGB, 8), (BAYER, 16)):
        for w, h in {(c["w"], c["h"]) for c in cases}:
            forms = {tc.takes_fast_form(c) for c in cases if (c["w"], c["h"]) == (w, h)}
            assert forms == ({True, False} if w % mult == 0 else {False}), (w, h)
    # every set of scales and biases meets every float dtype in both forms; each is inside the range, at whose ends "big" lies
    for dtype in tc.FLOATS:
        for fast in (True, False):
            assert {c["set"] for c in ALL if c["dtype"] == dtype and tc.takes_fast_form(c) == fast} == set(tc.SET_NAMES)
    for scale, bias in tc.SETS.values():
        assert all(T.factor_ok(x) for x in scale) and all(T.factor_ok(x) for x in bias)
    assert tc.SETS["big"][0][2] == np.float32(T.FACTOR_MAX) and tc.SETS["big"][1][2] == np.float32(T.FACTOR_MIN)
    assert not T.factor_ok(2.0 ** 65) and not T.factor_ok(2.0 ** -65) and not T.factor_ok(np.inf) and not T.factor_ok(np.nan) and T.factor_ok(0.0)
    # strides: padded ones on both sides, and the placement never lets two frames touch
    for c in ALL:
        ss, so, ds, do = tc.placement(c)
        assert ss >= tc.src_bytes(c) and ds >= tc.out_bytes(c) and ds % T.ELEM[c["dtype"]] == 0 and do % T.ELEM[c["dtype"]] == 0
    assert any(tc.placement(c)[0] > tc.src_bytes(c) and tc.placement(c)[2] > tc.out_bytes(c) for c in ALL)


def test_the_samples_reach_every_byte_value_and_the_16_bit_ends():
    seen8, seen16 = set(), set()
    for c in RGB:
        for f in tc.frames(c):
            (seen8 if c["bits"] == 8 else seen16).update(np.unique(f).tolist())
    assert seen8 == set(range(256))
    assert {0, 1, 2, 3, 65535} <= seen16
    big = next(c for c in RGB if c["bits"] == 8 and (c["w"], c["h"]) == (1032, 3) and tc.takes_fast_form(c))
    for ch in range(3):                                               # in one frame of the fast form, in every channel
        assert set(np.unique(tc.frames(big)[0][..., ch]).tolist()) == set(range(256))
    for c in RGB:                                                     # the integer dtypes keep the samples
        if c["dtype"] in (T.U8, T.U16):
            f = tc.frames(c)[0]
            assert tc.compute(c, 0) == (f.transpose(2, 0, 1) if c["layout"] == T.NCHW else f).tobytes()


def test_the_half_results_are_subnormal_tie_both_ways_and_overflow():
    f = all_values(T.F16)
    a = np.abs(f)
    b = f.view(np.uint32)
    h = T.f16_bits(f)
    sub = (a > 0) & (a < np.float32(2.0 ** -14))
    assert sub.any() and ((h[sub] & 0x7FFF) != 0).any(), "no subnormal half"
    assert (((h[sub] & 0x7C00) == 0) & ((h[sub] & 0x3FF) != 0)).any()
    inexact_sub = sub & (np.ldexp(a.astype(np.float64), 24) % 1 != 0)            # a subnormal half that is rounded, not merely kept
    assert inexact_sub.any()
    normal = (a >= np.float32(2.0 ** -14)) & (a < np.float32(65504.0))
    tie = normal & ((b & 0x1FFF) == 0x1000)
    assert (tie & ((b & 0x2000) == 0)).any(), "no half tie that goes down to even"
    assert (tie & ((b & 0x2000) != 0)).any(), "no half tie that goes up to even"
    assert ((h & 0x7FFF) == 0x7C00).any() and np.isfinite(f).all(), "no half overflow from a finite value"
    assert (h == 0x7C00).any() and (h == 0xFC00).any()                 # to either infinity
    # ties that real arithmetic produced, not only the planted biases: a Bayer batch at a power-of-two range
    natural = np.concatenate([f32_values(c, k).reshape(-1) for c in BAYER if c["dtype"] == T.F16 and c["set"] == "identity" for k in range(c["n"])])
    nb = natural.view(np.uint32)
    nt = (np.abs(natural) >= np.float32(2.0 ** -14)) & ((nb & 0x1FFF) == 0x1000)
    assert (nt & ((nb & 0x2000) == 0)).any() and (nt & ((nb & 0x2000) != 0)).any()


def test_the_bfloat16_results_tie_both_ways():
    f = all_values(T.BF16)
    b = f.view(np.uint32)
    tie = (b & 0xFFFF) == 0x8000
    assert (tie & ((b & 0x10000) == 0)).any() and (tie & ((b & 0x10000) != 0)).any()
    got = T.bf16_bits(f)
    assert (got[tie & ((b & 0x10000) == 0)] == (b[tie & ((b & 0x10000) == 0)] >> 16)).all()
    assert (got[tie & ((b & 0x10000) != 0)] == (b[tie & ((b & 0x10000) != 0)] >> 16) + 1).all()


def test_the_bayer_cases_go_below_black_above_white_and_through_a_mixed_clip():
    below = above = False
    for c in BAYER:
        for k, (black, white) in enumerate(tc.levels(c)):
            px = tc.frames(c)[k].astype(np.int64)
            below |= bool((px < black).any())
            above |= bool((px > white).any())
            if c["dtype"] == T.F32 and c["set"] == "identity" and (px < black).any():
                v = np.frombuffer(tc.compute(c, k), np.float32)
                assert (v < 0).any(), "a pixel below black is not negative in the tensor"
    assert below and above
    x4 = lambda a, b: (4 * a[0], 4 * a[1]) == b
    pairs = [(tc.levels(c)[k], tc.levels(c)[k + 1]) for c in BAYER if c["n"] == 3 for k in range(2)]
    assert any(x4(a, b) for a, b in pairs) and any(x4(b, a) for a, b in pairs), "a mixed clip's levels in one parity only"
    for c in BAYER[:64]:
        arr = tc.levels_array(c)
        for k, (black, white) in enumerate(tc.levels(c)):
            assert arr[k, 0] == black and arr[k, 1] == max(white - black, 1) and arr[k, 3] == 0
            assert arr[k, 2:3].view(np.float32)[0] == np.float32(1.0 / max(white - black, 1))
    with pytest.raises(ValueError):
        T.bayer_levels((1 << 30) + 1, 0)
    assert T.bayer_levels(-(1 << 30), 5)[1] == (1 << 30) + 5


RELEVANT = {"fma": tc.FLOATS, "folded": tc.FLOATS, "trunc_f16": (T.F16,), "trunc_bf16": (T.BF16,), "flush_f16": (T.F16,), "bgr": None,
            "g1g2": None, "layouts": None, "clamp_black": tc.FLOATS}


@pytest.mark.parametrize("variant", tc.WRONG)
def test_each_wrong_definition_differs_on_a_case_the_gpu_runs(variant):
    cases = BAYER if variant in ("g1g2", "clamp_black") else RGB if variant == "bgr" else ALL
    told = {}
    for c in cases:
        if RELEVANT[variant] is not None and c["dtype"] not in RELEVANT[variant]:
            continue
        key = (c["kind"], tc.takes_fast_form(c))                     # in both kinds' both forms (a 1-ulp slip can hide in a half)
        if told.get(key):
            continue
        told[key] = any(tc.compute(c, k, variant) != tc.compute(c, k) for k in range(c["n"]))
    assert told and all(told.values()), (variant, [k for k, v in told.items() if not v])


def test_the_definitions_conversions_are_torchs():
    import torch
    f = np.concatenate([all_values(T.F16), all_values(T.BF16)])
    t = torch.from_numpy(f.copy())
    assert np.array_equal(t.to(torch.float16).view(torch.int16).numpy().view(np.uint16), T.f16_bits(f))
    assert np.array_equal(t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16), T.bf16_bits(f))


def test_normalisation_is_computed_in_double_and_rounded_once():
    scale, bias = T.normalisation((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), 3)
    assert scale.dtype == np.float32 and scale[0] == np.float32(1.0 / 0.229) and bias[1] == np.float32(-0.456 / 0.224) and scale[3] == 1 and bias[3] == 0
    scale, bias = T.normalisation(None, None, 4)
    assert scale.tolist() == [1, 1, 1, 1] and bias.tolist() == [0, 0, 0, 0]
    scale, bias = T.normalisation(0.5, 0.25, 4)
    assert scale.tolist() == [4, 4, 4, 4] and bias.tolist() == [-2, -2, -2, -2]
    assert T.unit_of(8) == np.float32(1.0 / 255.0) and T.unit_of(16) == np.float32(1.0 / 65535.0)

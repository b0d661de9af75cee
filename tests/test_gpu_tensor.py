"""The tensor pass on the GPU (csrc/k_tensor.hip, csrc/tensor.cpp): mlvfs_amd_tensor_rgb_dev and mlvfs_amd_tensor_bayer_dev
against the numpy definition of mlvfs_amd/tensor.py on the cases of tests/tensor_cases.py (which tests/test_tensor_cases.py proves to
reach the ties, the subnormal halves, the overflows and the levels they claim, and to tell the wrong definitions apart): every legal
dtype x layout x source depth, batches of 1 and 3 with per-frame levels, padded strides on both sides, aligned and misaligned bases so
that both forms run at shapes either could take; the destination is filled with 0xA5 beforehand and every byte outside the tensors keeps
it; the source is unchanged.  All comparisons are of bytes, so floats are compared by their bits."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import lib, tensor as T

import tensor_cases as tc
from test_gpu_mlv_transcode import PAD, device_buffer, split

pytestmark = pytest.mark.gpu
RGB, BAYER = tc.rgb_cases(), tc.bayer_cases()


def spec_of(case):
    spec = lib.TensorSpec(kind=case["kind"], dtype=case["dtype"], layout=case["layout"], gain_q8=256)
    scale, bias = tc.scale_bias(case)
    spec.scale[:], spec.bias[:] = scale.tolist(), bias.tolist()
    return spec


def run_case(gpu, torch, case):
    """-> (the n tensors as bytes, every other byte of the destination); asserts that the source is unchanged"""
    fr = tc.frames(case)
    ss, so, ds, do = tc.placement(case)
    n, size = case["n"], tc.out_bytes(case)
    src = device_buffer(torch, fr, ss, so)
    before = src.clone()
    dst = torch.full((do + n * ds + 64,), PAD, dtype=torch.uint8, device="cuda")
    spec = spec_of(case)
    s, d = C.c_void_p(src.data_ptr() + so), C.c_void_p(dst.data_ptr() + do)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    if case["kind"] == T.RGB:
        lib.check(gpu.mlvfs_amd_tensor_rgb_dev(s, ss, case["w"], case["h"], case["bits"], C.byref(spec), d, ds, n, None), "tensor_rgb_dev")
    else:
        lv = torch.from_numpy(tc.levels_array(case).reshape(-1)).cuda()
        lib.check(gpu.mlvfs_amd_tensor_bayer_dev(s, ss, case["w"], case["h"], C.c_void_p(lv.data_ptr()), C.byref(spec), d, ds, n, None), "tensor_bayer_dev")
    torch.cuda.synchronize()
    assert torch.equal(src, before), "the source changed"
    parts, rest = split(dst, n, ds, size, do)
    return [p.tobytes() for p in parts], rest


def check_cases(gpu, cases):
    import torch
    assert cases
    for case in cases:
        got, rest = run_case(gpu, torch, case)
        label = tc.case_id(case)
        assert (rest == PAD).all(), (label, "bytes outside the tensors changed")
        for k, want in enumerate(tc.want(case)):
            if got[k] != want:
                a, b = np.frombuffer(got[k], np.uint8), np.frombuffer(want, np.uint8)
                first = int(np.flatnonzero(a != b)[0])
                raise AssertionError(f"{label} frame {k}: {int((a != b).sum())} of {a.size} bytes differ from the definition, the first at {first}: "
                                     f"{a[first:first + 8].tolist()} for {b[first:first + 8].tolist()}")


@pytest.mark.parametrize("w,h", tc.RGB_SIZES, ids=lambda v: str(v))
def test_tensor_rgb_dev_equals_the_definition(gpu, w, h):
    check_cases(gpu, [c for c in RGB if (c["w"], c["h"]) == (w, h)])


@pytest.mark.parametrize("w,h", tc.BAYER_SIZES, ids=lambda v: str(v))
def test_tensor_bayer_dev_equals_the_definition(gpu, w, h):
    check_cases(gpu, [c for c in BAYER if (c["w"], c["h"]) == (w, h)])


def test_the_bayer_parameters_are_the_helpers(gpu):
    """what the cases upload as a frame's levels is what mlvfs_amd_tensor_bayer_params writes for a header with them"""
    from mlvfs_amd import abi
    for black, white in tc.LEVELS:
        fh = abi.make_frame_headers(64, 48, black=black, white=white)
        out = np.full(4, -1, np.int32)
        assert gpu.mlvfs_amd_tensor_bayer_params(C.byref(fh), lib.ptr(out)) == 0
        b, r, u = T.bayer_levels(black, white)
        assert out.tolist() == [b, r, int(np.array([u], np.float32).view(np.int32)[0]), 0]


def test_refusals_leave_the_destination(gpu):
    import torch
    src = torch.full((8192,), 7, dtype=torch.uint8, device="cuda")
    dst = torch.full((8192,), PAD, dtype=torch.uint8, device="cuda")
    lv = torch.zeros(16, dtype=torch.int32, device="cuda")
    s, d, p = src.data_ptr(), dst.data_ptr(), lv.data_ptr()
    vp = lambda a: C.c_void_p(a) if a else None

    def spec(dtype=T.F16, layout=T.NCHW, scale=1.0, bias=0.0):
        sp = lib.TensorSpec(dtype=dtype, layout=layout)
        sp.scale[:], sp.bias[:] = [scale] * 4, [bias] * 4
        return sp

    rgb = lambda sp_, st, w, h, bits, spec_, dp, ost, n: gpu.mlvfs_amd_tensor_rgb_dev(vp(sp_), st, w, h, bits, C.byref(spec_) if spec_ else None, vp(dp), ost, n, None)
    bay = lambda sp_, st, w, h, lp, spec_, dp, ost, n: gpu.mlvfs_amd_tensor_bayer_dev(vp(sp_), st, w, h, vp(lp), C.byref(spec_) if spec_ else None, vp(dp), ost, n, None)
    ok = spec()
    bad_rgb = [(0, 192, 8, 8, 8, ok, d, 384, 1), (s, 192, 8, 8, 8, None, d, 384, 1), (s, 192, 8, 8, 8, ok, 0, 384, 1), (s, 192, 0, 8, 8, ok, d, 384, 1),
               (s, 192, 8, -1, 8, ok, d, 384, 1), (s, 192, 1 << 14, 1 << 14, 8, ok, d, 384, 1), (s, 192, 8, 8, 12, ok, d, 384, 1), (s, 192, 8, 8, 8, ok, d, 384, -1),
               (s, 191, 8, 8, 8, ok, d, 384, 2), (s, 192, 8, 8, 8, ok, d, 382, 2), (s, 192, 8, 8, 8, ok, d, 385, 2), (s, 192, 8, 8, 8, ok, d + 1, 384, 1),
               (s + 1, 384, 8, 8, 16, ok, d, 384, 1), (s, 385, 8, 8, 16, ok, d, 384, 2), (d + 1024, 192, 8, 8, 8, ok, d + 1024, 384, 1),
               (d + 1024, 192, 8, 8, 8, ok, d + 1024 + 190, 384, 1), (d + 1024, 192, 8, 8, 8, ok, d + 1024 - 382, 384, 1),
               (s, 192, 8, 8, 8, spec(T.U16), d, 384, 1), (s, 384, 8, 8, 16, spec(T.U8), d, 192, 1), (s, 192, 8, 8, 8, spec(5), d, 384, 1),
               (s, 192, 8, 8, 8, spec(-1), d, 384, 1), (s, 192, 8, 8, 8, spec(layout=2), d, 384, 1), (s, 192, 8, 8, 8, spec(scale=float("inf")), d, 384, 1),
               (s, 192, 8, 8, 8, spec(bias=float("nan")), d, 384, 1), (s, 192, 8, 8, 8, spec(scale=2.0 ** 65), d, 384, 1),
               (s, 192, 8, 8, 8, spec(bias=2.0 ** -65), d, 384, 1)]
    for args in bad_rgb:
        assert rgb(*args) == lib.ERR_ARG, args[:5] + args[6:]
    bad_bay = [(0, 512, 16, 16, p, ok, d, 512, 1), (s, 512, 16, 16, 0, ok, d, 512, 1), (s, 512, 16, 16, p, ok, 0, 512, 1), (s, 512, 1, 16, p, ok, d, 512, 1),
               (s, 512, 16, 1, p, ok, d, 512, 1), (s, 512, 1 << 14, 1 << 14, p, ok, d, 512, 1), (s, 510, 16, 16, p, ok, d, 512, 2), (s, 513, 16, 16, p, ok, d, 512, 2),
               (s, 512, 16, 16, p, ok, d, 510, 2), (s + 1, 512, 16, 16, p, ok, d, 512, 1), (s, 512, 16, 16, p + 2, ok, d, 512, 1), (s, 512, 16, 16, p, ok, d + 1, 512, 1),
               (s, 512, 16, 16, p, spec(T.U8), d, 512, 1), (s, 512, 16, 16, p, spec(scale=-float("inf")), d, 512, 1), (d + 1024, 512, 16, 16, p, ok, d + 1024 + 510, 512, 1),
               (s, 512, 16, 16, d + 64, ok, d, 512, 1)]
    for args in bad_bay:
        assert bay(*args) == lib.ERR_ARG, args[:5] + args[6:]
    torch.cuda.synchronize()
    assert bool((dst == PAD).all()) and bool((src == 7).all())
    # an integer dtype reads neither scale nor bias; directly behind the source is no overlap; nothing to do is no error
    assert rgb(s, 192, 8, 8, 8, spec(T.U8, scale=float("nan")), d, 192, 1) == 0
    assert rgb(s, 192, 8, 8, 8, ok, d, 384, 0) == 0 and bay(s, 512, 16, 16, p, ok, d, 512, 0) == 0
    assert rgb(d + 1024, 192, 8, 8, 8, spec(T.U8, T.NHWC), d + 1024 + 192, 192, 1) == 0
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:192] == 7).all() and (host[192:1024 + 192] == PAD).all() and (host[1024 + 192:1024 + 384] == PAD).all() and (host[1024 + 384:] == PAD).all()

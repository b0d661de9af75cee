"""Pattern noise on the GPU (csrc/k_pnoise.hip, csrc/patternnoise.cpp) over the whole int16 range, at the exact limits and on long columns:
the drop-in fix_pattern_noise and the batched mlvfs_amd_fix_pattern_noise_dev against the oracle on the cases of tests/pnoise_cases.py
(which tests/test_pnoise_cases.py proves to reach what they claim, to tell every wrong form of the definition apart, and to be judged alike
by the oracle and the reference's own code).  Content cases run at debug_flags 0 and in every debug view, geometry cases -- half-extents
768, 769, 2048 and 2049, where the launcher changes the column-median kernel, and the smallest frames -- at 0 and in one view per
direction.  Every case also goes through the batched entry with its own white level in the geometry: alone, as the first of three
different frames with padded strides whose padding must stay untouched (the 4098 x 24 and 24 x 4098 batches run the any-height kernel
with frame strides), and some with the scratch capped so that three frames go out one by one.  Every comparison is equality of bytes."""
import ctypes as C
import functools

import numpy as np
import pytest

from mlvfs_amd import lib

import pnoise_cases as pc
from test_gpu_mlv_transcode import PAD, device_buffer, split

pytestmark = pytest.mark.gpu
CONTENT, GEOMETRY = pc.content_cases(), pc.geometry_cases()
ALL = CONTENT + GEOMETRY
by_name = {c["name"]: c for c in ALL}
GEOMETRY_VIEWS = (4, 9)                                     # the noise of the column pass, the mask of the row pass
STRIDE_PAD = 34                                             # even, as the entry asks, and no multiple of 4: frames 1 and 2 start off a dword


@functools.lru_cache(maxsize=None)
def batch_frames(name):
    return pc.batch_of(by_name[name])


_WANTED = {}


def wanted(oracle, name, k, flags):
    """the oracle's bytes for frame k of the case's batch (frame 0 is the case itself): computed once, shared, never changed"""
    key = (name, k, flags)
    if key not in _WANTED:
        _WANTED[key] = oracle.fix_pattern_noise(batch_frames(name)[k], by_name[name]["white"], flags)
        _WANTED[key].setflags(write=False)
    return _WANTED[key]


def report(label, got, want):
    """fails with the number of differing pixels and the first one's (x, y, plane), planes r, g1, g2, b as in the kernels"""
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    y, x = (int(v) for v in bad[0])
    raise AssertionError(f"{label}: {len(bad)} of {got.size} px differ, the first at x {x}, y {y}, plane {(x & 1) + 2 * (y & 1)}: "
                         f"{int(got[y, x])} for {int(want[y, x])}")


def dropin(gpu, frame, white, flags=0):
    got = frame.copy()
    gpu.fix_pattern_noise(lib.ptr(got), frame.shape[1], frame.shape[0], white, flags)
    return got


def pn_frame_bytes(w, h):
    """pattern_noise_batch_frame_bytes (csrc/k_pnoise.hip): the scratch that one frame of a sub-batch takes"""
    up = lambda b: (b + 255) // 256 * 256
    n = w * h
    return up(n * 2) * 2 + up(n * 4) + up((2 * max(w, h) + 8) * 4) + 256


def run_batch(gpu, case, frames, pad):
    """the frames through mlvfs_amd_fix_pattern_noise_dev, size + pad bytes apart -> the frames after it; the padding must keep its bytes"""
    import torch
    w, h, n, size = case["w"], case["h"], len(frames), case["w"] * case["h"] * 2
    stride = size + pad
    buf = device_buffer(torch, frames, stride)
    geom = lib.Geom(w, h, 14, 0, case["white"], 0, 0)
    lib.check(gpu.mlvfs_amd_fix_pattern_noise_dev(C.byref(geom), C.c_void_p(buf.data_ptr()), stride, n, None), "fix_pattern_noise_dev")
    parts, rest = split(buf, n, stride, size)
    assert (rest == PAD).all(), (case["name"], n, "bytes outside the frames changed")
    return [p.view(np.uint16).reshape(h, w) for p in parts]


@pytest.mark.parametrize("name", [c["name"] for c in ALL])
def test_the_dropin_equals_the_oracle(gpu, oracle, name):
    c = by_name[name]
    for flags in (0,) + (GEOMETRY_VIEWS if c["geometry"] else pc.VIEWS):
        report(f"{name} flags {flags}", dropin(gpu, c["frame"], c["white"], flags), wanted(oracle, name, 0, flags))


@pytest.mark.parametrize("name", [c["name"] for c in ALL])
def test_batches_equal_the_oracle_and_the_dropin(gpu, oracle, name):
    c = by_name[name]
    frames = batch_frames(name)
    for n, pad in ((1, 0), (1, STRIDE_PAD), (3, STRIDE_PAD)):
        got = run_batch(gpu, c, frames[:n], pad)
        for k in range(n):
            report(f"{name} frame {k} of {n}, pad {pad}", got[k], wanted(oracle, name, k, 0))
            report(f"{name} frame {k} of {n}, pad {pad}, against the drop-in", got[k], dropin(gpu, frames[k], c["white"]))


@pytest.mark.parametrize("name", ["walk", "extremes", "grads_t", "mask_counts", "geom_1538x24", "geom_24x4098", "geom_4x20"])
def test_a_batch_cut_into_single_frames_equals_the_oracle(gpu, oracle, name):
    """the scratch capped at one frame's: three frames go out as 1 + 1 + 1"""
    c = by_name[name]
    frames = batch_frames(name)
    gpu.mlvfs_amd_test_pn_scratch_cap(pn_frame_bytes(c["w"], c["h"]))
    try:
        got = run_batch(gpu, c, frames, STRIDE_PAD)
    finally:
        gpu.mlvfs_amd_test_pn_scratch_cap(0)
    for k in range(3):
        report(f"{name} frame {k} of 1 + 1 + 1", got[k], wanted(oracle, name, k, 0))

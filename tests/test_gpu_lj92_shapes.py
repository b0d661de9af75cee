"""The LJ92 decoder's prediction kernels (csrc/k_lj92.hip) at the shapes of tests/lj92_shape_cases.py, bit for bit against the oracle:
rows beyond the 8192 values k_lj_rows stages in LDS (worked on in place, block loops with a second trip and more), batches that mix
widths on both sides of 8192, widths around the 32-column block edges, one row, one column, 16-bit samples with predictors 4 to 7, and
the row limit of predictor 7.  tests/test_lj92_shape_cases.py shows on the CPU that the cases reach all that.

Every case goes to the batched entry point in ONE call (lj92.decode_frames where it has a video geometry, mlvfs_amd_lj92_decode_dev in
the decoder's own order where it has none); cases in the decoder's own order and the wide rows also go, stream by stream, through the
drop-in lj92_open / lj92_decode / lj92_close.  A frame's expected result is always the oracle's for that stream alone."""
import ctypes as C

import numpy as np
import pytest

import lj92_shape_cases as sc
from test_lj92 import dropin_decode, gpu_decode

pytestmark = pytest.mark.gpu

_want = {}


def want(oracle, stream):
    """The oracle's image of a stream, in the decoder's own order (once per stream)"""
    if stream not in _want:
        st, img = oracle.lj92_decode(stream)
        assert st == 0
        img.setflags(write=False)
        _want[stream] = img
    return _want[stream]


def decode_raw_batch(gpu, streams, shapes):
    """mlvfs_amd_lj92_decode_dev in the decoder's own order (xres = yres = 0): every stream's values, H x W of its own JPEG"""
    import torch
    n = len(streams)
    stride = max(h * w for h, w in shapes)
    out = torch.zeros((n, stride), dtype=torch.int16, device="cuda")
    bufs = [np.frombuffer(s, np.uint8) for s in streams]
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    sizes = (C.c_size_t * n)(*[b.size for b in bufs])
    rc = gpu.mlvfs_amd_lj92_decode_dev(ptrs, sizes, n, 0, 0, C.c_void_p(out.data_ptr()), stride * 2, None)
    assert rc == 0, gpu.mlvfs_amd_last_error()
    flat = out.cpu().numpy().view(np.uint16)
    return [flat[k, : h * w].reshape(h, w) for k, (h, w) in enumerate(shapes)]


@pytest.mark.parametrize("case", sc.CASES, ids=[c.name.replace(" ", "-") for c in sc.CASES])
def test_case_equals_oracle(gpu, oracle, reference, case):
    streams = sc.streams(case, reference)
    shapes = [(f.h, f.w) for f in case.frames]
    if case.video is not None:
        xres, yres = case.video
        got = gpu_decode(streams, xres, yres)                                  # one call, untiled
        for k, s in enumerate(streams):
            assert np.array_equal(got[k], oracle.lj92_untile(want(oracle, s), xres, yres)), (case.name, case.frames[k])
    else:
        got = decode_raw_batch(gpu, streams, shapes)                           # one call, the decoder's own order
        for k, s in enumerate(streams):
            assert np.array_equal(got[k], want(oracle, s)), (case.name, case.frames[k])
    if case.video is None or case.wide:
        for k, s in enumerate(streams):                                        # the drop-in symbols: a stream per call
            st, img, dims = dropin_decode(gpu, s)
            f = case.frames[k]
            assert st == 0 and dims == (f.w, f.h, f.bits), (case.name, f, st, dims)
            assert np.array_equal(img, want(oracle, s)), (case.name, f)


def test_every_block_edge_width_in_one_call(gpu, oracle, reference):
    """All the narrow shapes in one batch in the decoder's own order: twelve widths from 1 to 66 share one launch's LDS, in sub-batches
    of four"""
    frames = [f for c in sc.CASES if c.name.startswith("edge ") for f in c.frames]
    assert len(frames) == 4 * (len(sc.EDGE_WIDTHS) + 1)
    streams = [sc.stream(f, reference) for f in frames]
    got = decode_raw_batch(gpu, streams, [(f.h, f.w) for f in frames])
    for k, s in enumerate(streams):
        assert np.array_equal(got[k], want(oracle, s)), frames[k]


def test_wide_row_through_decode_untiled(gpu, oracle, reference):
    """mlvfs_amd_lj92_decode_untiled on rows of 9216 values: the 192 x 192 video frame of main.c:646-667"""
    case = next(c for c in sc.CASES if c.name == "wide 4x9216")
    xres, yres = case.video
    gpu.mlvfs_amd_lj92_decode_untiled.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    for f in case.frames:
        if f.pred not in (1, 6, 7):
            continue
        s = sc.stream(f, reference)
        buf = np.frombuffer(s, np.uint8).copy()
        hd = C.c_void_p()
        assert gpu.lj92_open(C.byref(hd), C.c_void_p(buf.ctypes.data), buf.size, None, None, None) == 0
        out = np.zeros((yres, xres), np.uint16)
        st = gpu.mlvfs_amd_lj92_decode_untiled(hd, C.c_void_p(out.ctypes.data), xres, yres)
        gpu.lj92_close(hd)
        assert st == 0 and np.array_equal(out, oracle.lj92_untile(want(oracle, s), xres, yres)), f


def test_predictor_7_beyond_its_row_limit_is_refused_before_any_kernel(gpu):
    """8193 rows: mlvfs_amd_lj92_decode_dev checks every stream's header -- predictor 7's row limit among the checks -- in its first
    loop, before it sizes a buffer, uploads a byte or launches a kernel (csrc/lj92.cpp), so the refusal leaves the output untouched;
    the refused stream is refused as well when a good one stands in front of it."""
    import torch
    from mlvfs_amd import lib, lj92
    f = sc.REFUSED_P7
    bad = sc.stream(f)
    st, img, _ = dropin_decode(gpu, bad)
    assert st != 0 and b"limited to 8192 rows" in gpu.mlvfs_amd_last_error()
    good = sc.stream(sc.Frame(8192, 2, 7, seed=300))
    for streams in ([bad], [good, bad]):
        out = torch.full((len(streams), 8193 * 2), 0x5A5A, dtype=torch.int16, device="cuda")
        bufs = [np.frombuffer(s, np.uint8) for s in streams]
        ptrs = (C.c_void_p * len(streams))(*[b.ctypes.data for b in bufs])
        sizes = (C.c_size_t * len(streams))(*[b.size for b in bufs])
        rc = gpu.mlvfs_amd_lj92_decode_dev(ptrs, sizes, len(streams), 0, 0, C.c_void_p(out.data_ptr()), 8193 * 2 * 2, None)
        assert rc == lib.ERR_ARG and b"limited to 8192 rows" in gpu.mlvfs_amd_last_error()
        assert bool((out == 0x5A5A).all())                                     # nothing ran
    with pytest.raises(lib.MlvfsAmdError, match="limited to"):
        lj92.decode_frames([bad], 2, 8193)


def test_an_ordinary_stream_decodes_after_all_that(gpu, oracle):
    """The thread's grow-only work buffers and the row kernel's LDS went through every size above: a plain 136 x 72 frame afterwards"""
    from test_lj92 import images
    from oracle import lj92_testenc as enc
    w, h = 136, 72
    s = enc.encode(images(w, h)["smooth"], 6, 14)
    st, img = oracle.lj92_decode(s)
    assert st == 0
    assert np.array_equal(gpu_decode([s], w, h)[0], oracle.lj92_untile(img, w, h))
    st, got, dims = dropin_decode(gpu, s)
    assert st == 0 and dims == (w, h, 14) and np.array_equal(got, img)

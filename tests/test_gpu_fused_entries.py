"""Every host-side door to the fused pass (csrc/fused_pass.cpp: run_fused_pass) gives the same bytes, and they are the oracle's.

One synthetic 14-bit clip of 5 frames goes through ClipStream.process (mlvfs_amd_process_frames_dev), process_unpacked on the unpacked
frames, process_host in chunks of 2 (a short last chunk, three slots of the pipeline) and, frame by frame, the drop-in symbols inside a
frame bracket (dropin.cpp: lazy_run).  The geometry is the smallest of tests/stream_shapes.py with a second tile column (tiles are 128
pixels wide); the 14-bit loader takes every geometry.  The pixel map is the bad-pixel map detected on frame 0 -- the only kind of map the
bracket joins to its launch (a focus-pixel map runs early there) -- with defects planted in a cell of the halo between the two tile
columns and in the halo between two tile rows; the stripes correction is set by hand."""
import ctypes as C

import numpy as np
import pytest

import stream_shapes as ss
from mlvfs_amd import abi, lib, synth

pytestmark = pytest.mark.gpu
BLACK, WHITE = synth.BLACK, synth.WHITE
CO = [65536, 65536, 65354, 65738, 65241, 65868, 65450, 65640]
N = 5
W, H = min((g for g in ss.GEOMETRIES if g[0] > 128), key=lambda g: g[0] * g[1])
PLANTED = [(126, 40), (129, 31)]                  # cell column 63: halo of tile column 1; cell row 15: first of tile row 1, halo of row 0
GUID = 0xF05ED0075
# what is switched on: (cs, pixel map, stripes)
CASES = [(0, True, True), (2, True, True), (5, True, True), (0, False, False)]


def _frames(shift=0):
    out = []
    for k in range(N):
        f = synth.normal_frame(W, H, seed=9, frame=k, hot=20, cold=20)
        for x, y in PLANTED:
            f[y, x] = 16000
        out.append((f >> shift).astype(np.uint16))
    return out


def _want(oracle, frames, pixels, black, white, cs, fix, stripes):
    out = []
    for f in frames:
        img = oracle.apply_bad_pixels(f, black, pixels) if fix else f
        if cs:
            img = oracle.chroma_smooth(img, black, cs)
        out.append(oracle.stripes_apply(img, black, white, 1, np.array(CO, np.int32)) if stripes else img)
    return out


@pytest.fixture(scope="module")
def clip(gpu, oracle):
    """The clip, its map, a ClipStream that carries map and correction, and the drop-in's map of the same clip (detected on frame 0)"""
    from mlvfs_amd.stream import ClipStream
    assert (W, H) == (504, 122) and W % 8 == 0 and -(-W // 128) >= 2
    frames = _frames()
    pixels = oracle.detect_bad_pixels(frames[0], BLACK, 0)
    have = {(int(x), int(y)) for x, y in np.asarray(pixels).reshape(-1, 2)}
    assert set(PLANTED) <= have, "the planted defects are not in the map"
    s = ClipStream(W, H, 14, BLACK, WHITE, device=0)
    s.set_pixel_map(pixels)
    s.set_stripes(1, CO)
    packed = [np.ascontiguousarray(synth.pack_bits(f), np.uint16) for f in frames]
    fh = abi.make_frame_headers(W, H, black=BLACK, white=WHITE, guid=GUID)
    img = frames[0].copy()                          # the clip's first frame detects (outside a bracket: at once)
    gpu.fix_bad_pixels(C.byref(fh), lib.ptr(img), 0, 0)
    assert np.array_equal(img, oracle.apply_bad_pixels(frames[0], BLACK, pixels))
    yield dict(frames=frames, pixels=pixels, s=s, packed=packed, dev=s.upload_packed(packed))
    s.close()
    gpu.stripes_free_corrections()


def _dropin(gpu, packed, cs, fix, stripes):
    """tests/test_gpu_resident.py's bracket sequence, one frame per bracket; every frame must run as one launch at the bracket's end"""
    fh = abi.make_frame_headers(W, H, black=BLACK, white=WHITE, guid=GUID)
    corr = gpu.stripes_new_correction(b"fused_entries.MLV")
    corr.contents.correction_needed = 1
    for k in range(8):
        corr.contents.coeffficients[k] = CO[k]
    stats0, stats = (C.c_longlong * 2)(), (C.c_longlong * 2)()
    gpu.mlvfs_amd_dropin_stats(stats0)
    out = []
    for p in packed:
        img = np.full((H, W), 0xABCD, np.uint16)
        assert gpu.mlvfs_amd_frame_begin() == 0
        assert gpu.dng_get_image_data(C.byref(fh), lib.ptr(p), lib.ptr(img), 0, img.nbytes) == img.nbytes
        if fix:
            gpu.fix_bad_pixels(C.byref(fh), lib.ptr(img), 0, 0)
        if cs:
            gpu.chroma_smooth(C.byref(fh), lib.ptr(img), cs)
        if stripes:
            gpu.stripes_apply_correction(C.byref(fh), corr, lib.ptr(img), 0, img.size)
        assert (img == 0xABCD).all(), "a stage wrote the host buffer"
        assert gpu.mlvfs_amd_frame_end() == 0
        out.append(img)
    gpu.mlvfs_amd_dropin_stats(stats)
    assert stats[0] - stats0[0] == len(packed) and stats[1] == stats0[1], (list(stats0), list(stats))
    return out


@pytest.mark.parametrize("cs,fix,stripes", CASES, ids=["cs0", "cs2", "cs5", "nothing"])
def test_every_door_gives_the_oracles_frames(gpu, oracle, clip, cs, fix, stripes):
    from mlvfs_amd.stream import to_numpy_u16
    s = clip["s"]
    want = _want(oracle, clip["frames"], clip["pixels"], BLACK, WHITE, cs, fix, stripes)
    doors = {
        "process": to_numpy_u16(s.process(clip["dev"], cs=cs, fix_pixels=fix, stripes=stripes)),
        "process_unpacked": to_numpy_u16(s.process_unpacked(s.unpack(clip["dev"]), cs=cs, fix_pixels=fix, stripes=stripes)),
        "process_host": to_numpy_u16(s.process_host(clip["dev"].cpu(), cs=cs, fix_pixels=fix, stripes=stripes, chunk=2)).reshape(N, H, W),
        "drop-in bracket": _dropin(gpu, clip["packed"], cs, fix, stripes),
    }
    for name, got in doors.items():
        for k in range(N):
            assert np.array_equal(got[k], want[k]), (name, k, int((got[k] != want[k]).sum()))


@pytest.mark.parametrize("bpp", [12, 10])
def test_other_bit_depths_through_process_and_process_host(gpu, oracle, bpp):
    """process_host's branch for other bit depths (chunks through the device entry point).  12 bits: the fused loader reads the stream
    itself; 10 bits: 504 is no multiple of 16, so the device entry point unpacks into the clip's buffer first (frame_kernel_takes)"""
    from mlvfs_amd.stream import ClipStream, to_numpy_u16
    shift = 14 - bpp
    black, white = BLACK >> shift, WHITE >> shift
    frames = _frames(shift)
    pixels = oracle.detect_bad_pixels(frames[0], black, 0)
    s = ClipStream(W, H, bpp, black, white, device=0)
    s.set_pixel_map(pixels)
    s.set_stripes(1, CO)
    dev = s.upload_packed([synth.pack_bits(f, bpp) for f in frames])
    want = _want(oracle, frames, pixels, black, white, 5, True, True)
    doors = {
        "process": to_numpy_u16(s.process(dev, cs=5, fix_pixels=True, stripes=True)),
        "process_host": to_numpy_u16(s.process_host(dev.cpu(), cs=5, fix_pixels=True, stripes=True, chunk=2)).reshape(N, H, W),
    }
    s.close()
    for name, got in doors.items():
        for k in range(N):
            assert np.array_equal(got[k], want[k]), (name, k, int((got[k] != want[k]).sum()))

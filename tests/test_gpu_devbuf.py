"""Device buffers that grow on demand (csrc/common.h, DevBuf): what a handle serves after its buffers grew, and after a
growth that failed -- mlvfs_amd_test_fail_next(3) fails the calling thread's next DevBuf / PinBuf growth as if the allocation had
failed: the old block is gone, nothing is allocated.  What is expected always comes from a fresh handle (or is the frame itself),
never from the handle under test.

The host pipeline's slots and the drop-in symbols' staging belong to the host thread; those two tests run on a thread of their own,
where both start empty whatever earlier tests of the process have grown -- the growth the hook waits for is then certain to come."""
import ctypes as C
import threading

import numpy as np
import pytest

from mlvfs_amd import abi, lib, mlvfile, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

pytestmark = pytest.mark.gpu
BLACK, WHITE = synth.BLACK, synth.WHITE
W, H, N = 64, 48, 5


def on_a_fresh_thread(fn):
    """fn() on a new host thread; its result, or its exception raised here"""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except BaseException as e:           # noqa: BLE001 (handed to the caller's thread)
            box["error"] = e

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("devbuf") / "M07-1234.MLV")
    frames = [synth.normal_frame(W, H, seed=3, frame=k) for k in range(N)]
    mlvfile.write_clip(path, [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in frames], W, H)
    return path


CALLS = [("dng", (0, 1), dict(batch=1)), ("dng", (0, 5), dict(batch=4)), ("dng_lossless", (0, 5), dict(batch=4)), ("rgb", (0, 5), dict(batch=4))]


def plain(result):
    """a call's result as something == compares: dng / rgb give an array, dng_lossless (files, flags)"""
    return result.tobytes() if isinstance(result, np.ndarray) else result


@pytest.fixture(scope="module")
def fresh(gpu, clip):
    """what a fresh handle gives for each of CALLS alone"""
    want = []
    for name, args, kw in CALLS:
        with mlvfile.MlvReader(clip) as r, Mount(r, MlvfsOptions()) as m:
            want.append(plain(getattr(m, name)(*args, **kw)))
    return want


def test_a_mount_grows(gpu, clip, fresh):
    with mlvfile.MlvReader(clip) as r, Mount(r, MlvfsOptions()) as m:
        for (name, args, kw), want in zip(CALLS, fresh):
            assert plain(getattr(m, name)(*args, **kw)) == want, f"{name}{args} {kw} on the handle that grew"


def test_a_mount_survives_a_failed_growth(gpu, clip, fresh):
    with mlvfile.MlvReader(clip) as r, Mount(r, MlvfsOptions()) as m:
        assert plain(m.dng(0, 1, batch=1)) == fresh[0]
        gpu.mlvfs_amd_test_fail_next(3)
        with pytest.raises(lib.MlvfsAmdError, match="injected failure"):
            m.dng(0, 5, batch=4)
        assert plain(m.dng(0, 5, batch=4)) == fresh[1]


def test_the_host_pipeline_survives_a_failed_growth(gpu):
    """Its slots grow one by one.  A growth that fails part-way leaves some slots empty: the next call, however small, has to allocate
    them again instead of trusting a capacity shared by all of them."""
    import torch
    from mlvfs_amd.stream import ClipStream

    def body():
        w, h, n = 256, 130, 5
        s = ClipStream(w, h, 14, BLACK, WHITE, device=0)
        frames = [synth.normal_frame(w, h, frame=k) for k in range(n)]
        packed = s.upload_packed([synth.pack_bits(f) for f in frames])
        s.analyse_first_frame(packed, cs=5, bad_pix=1, stripes=True, rand_mode=1)
        want = s.process(packed, cs=5, fix_pixels=True, stripes=True).cpu().contiguous().view(torch.uint8).reshape(n, -1)
        host_in = packed.cpu()
        run = lambda chunk: s.process_host(host_in, torch.zeros((n, s.out_stride), dtype=torch.uint8), cs=5, fix_pixels=True, stripes=True, chunk=chunk)
        first = run(1)
        out = torch.zeros((n, s.out_stride), dtype=torch.uint8)
        gpu.mlvfs_amd_test_fail_next(3)
        with pytest.raises(lib.MlvfsAmdError, match="injected failure"):
            s.process_host(host_in, out, cs=5, fix_pixels=True, stripes=True, chunk=4)
        after = [run(1), run(4)]
        s.close()
        return want, first, after

    want, first, after = on_a_fresh_thread(body)
    assert torch.equal(first, want)
    assert torch.equal(after[0], want), "chunk=1 after the failed growth"
    assert torch.equal(after[1], want), "chunk=4 after the failed growth"


def test_the_dropin_thread_context_survives_a_failed_growth(gpu, capfd):
    def unpack(w, h, seed):
        f = synth.normal_frame(w, h, seed=seed)
        fh = abi.make_frame_headers(w, h, black=BLACK, white=WHITE)
        p = np.ascontiguousarray(synth.pack_bits(f), np.uint16)
        img = np.full((h, w), 0xABCD, np.uint16)
        return f, img, lambda: gpu.dng_get_image_data(C.byref(fh), lib.ptr(p), lib.ptr(img), 0, img.nbytes)

    def body():
        assert gpu.mlvfs_amd_init(0) == 0
        f, img, call = unpack(64, 48, 5)
        assert call() == img.nbytes and np.array_equal(img, f)
        f, img, call = unpack(416, 264, 6)
        gpu.mlvfs_amd_test_fail_next(3)
        failed = call(), img.copy(), gpu.mlvfs_amd_last_error()
        again = call(), img.copy()
        return f, failed, again

    capfd.readouterr()
    f, (rc, img, err), (rc2, img2) = on_a_fresh_thread(body)
    assert rc == 0 and not img.any(), "the failed growth left the caller's bytes in the frame"
    assert b"served black" in capfd.readouterr().err.encode()
    assert b"injected failure" in err
    assert rc2 == img2.nbytes and np.array_equal(img2, f)

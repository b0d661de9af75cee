"""mlvfs_amd_mlv_transcode on a clip of N 3584x1320 frames (14 bits, two chunks), file I/O included: plain -> LJ92, then that
output -> plain; output bytes / input bytes; and, where oracle/_ref is present, the reference encoder's time per frame on one host
core (Reference.lj92_encode_tile of the tiled frame, the tiling not counted) as the baseline.

    python tools/mlv_transcode_bench.py [--frames 32] [--batch 8] [--dir DIR] [--loops 3]

For the time per frame of k_mlv_tile / k_mlv_pack beside k_unpack_x16<14> on the same frames run it under
`rocprofv3 --kernel-trace --stats -- python tools/mlv_transcode_bench.py --loops 1` (under a timeout)."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlvfs_amd import lib, mlvfile, synth

W, H = 3584, 1320


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--io-threads", type=int, default=0)
    ap.add_argument("--dir", default=None, help="where the clips go (default: a temporary directory)")
    a = ap.parse_args()
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    root = tempfile.mkdtemp(prefix="mlvtc_", dir=a.dir)
    try:
        # eight different frames, repeated: the encoder's work depends on the content, not on its novelty
        base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, a.frames))]
        packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
        src = os.path.join(root, "src")
        os.mkdir(src)
        mlvfile.write_clip(os.path.join(src, "B.MLV"), [packed[k % len(packed)] for k in range(a.frames)], W, H, chunks=2)
        res = {}
        for what, frm, lj92 in (("plain->lj92", src, True), ("lj92->plain", os.path.join(root, "lj92"), False)):
            best = None
            for loop in range(a.loops + 1):                          # the first pass warms the page cache, the code objects and the staging
                dst = os.path.join(root, "lj92" if lj92 else "plain")
                shutil.rmtree(dst, ignore_errors=True)
                os.mkdir(dst)
                with mlvfile.MlvReader(os.path.join(frm, "B.MLV")) as r:
                    t0 = time.perf_counter()
                    s = r.transcode(os.path.join(dst, "B.MLV"), lj92=lj92, batch=a.batch, io_threads=a.io_threads)
                    dt = time.perf_counter() - t0
                if loop and (best is None or dt < best):
                    best = dt
            res[what] = (s, best)
            print(f"{what}: {s['frames']} frames, best of {a.loops}: {best:.3f} s = {s['frames'] / best:.1f} frames/s, {best / s['frames'] * 1e3:.2f} ms/frame;"
                  f" payload bytes {s['bytes_in']} -> {s['bytes_out']} (x{s['bytes_out'] / s['bytes_in']:.3f})")
        back = res["lj92->plain"][0]["bytes_out"]
        print(f"round trip: {back} bytes of plain payload, the source had {res['plain->lj92'][0]['bytes_in']}")
        try:
            from oracle import bindings
            if bindings.have_ref():
                R = bindings.Reference()
                tiled = [np.ascontiguousarray(np.block([[f[0::2, 0::2], f[0::2, 1::2]], [f[1::2, 0::2], f[1::2, 1::2]]])) for f in base[:4]]
                t = []
                for img in tiled:
                    t0 = time.perf_counter(); R.lj92_encode_tile(img, W, H, 14); t.append(time.perf_counter() - t0)
                print(f"reference encoder, one host core: {np.median(t) * 1e3:.1f} ms/frame (median of {len(t)}), the tiling not counted")
            else:
                print("reference encoder: oracle/_ref not present")
        except Exception as e:  # noqa: BLE001
            print("reference not available:", e)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return 0


if __name__ == "__main__":
    # on a thread of its own: the library's per-thread stream is then given back when the thread ends, not while the process
    # exits -- under rocprofv3 the profiler's own state is gone by then and the run ends in an abort instead of a stats file
    import threading
    rc = [1]
    t = threading.Thread(target=lambda: rc.__setitem__(0, main()))
    t.start()
    t.join()
    sys.exit(rc[0])

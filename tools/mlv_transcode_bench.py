"""mlvfs_amd_mlv_transcode on a clip of N 3584x1320 frames (14 bits, two chunks), file I/O included: plain -> LJ92, then that
output -> plain; output bytes / input bytes; and, where oracle/_ref is present, the reference encoder's time per frame on one host
core (Reference.lj92_encode_tile of the tiled frame, the tiling not counted) as the baseline.

    python tools/mlv_transcode_bench.py [--frames 32] [--batch 8] [--dir DIR] [--loops 3] [--bits N [N ...]] [--skip-kernels]

For the time per frame of k_mlv_tile / k_mlv_pack beside k_unpack_x16<14> on the same frames run it under
`rocprofv3 --kernel-trace --stats -- python tools/mlv_transcode_bench.py --loops 1` (under a timeout).

--bits N (8..16; several may be given): the clip at another bit depth (mlvfs_amd_mlv_transcode_bits; the numbers of DESIGN.md 3.9).
1. Kernel times.  The tool starts ITSELF once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, the
   program behind `--`); that child rewrites the clip, in one process and twice each (the second round is the warm one),
       plain -> LJ92 at 14 bits                 k_unpack_x16<14>, k_mlv_tile_x<16, false>    (no conversion: the routes as they were)
       plain -> plain at the first N            k_mlv_repack_x16<14, N>                      (unpack, shift and pack in one pass)
       plain -> LJ92 at N                       k_mlv_unpack_shift_x16<14>, k_mlv_tile_x<16, false>
       that LJ92 clip (14 bits) -> plain at N   k_mlv_pack_x16<N, true>                      (the second of the two passes k_mlv_repack replaces)
       that LJ92 clip -> LJ92 at N              k_mlv_tile_x<16, true>
   and the parent prints every kernel's time per frame with the spread of its launches, and the fused pass beside the two it replaces.
2. Frames per second and payload bytes out / in, best of --loops, for plain -> LJ92 at 14 bits (no conversion) and, for every N,
   plain -> plain and plain -> LJ92 at N, all in this one call."""
import argparse
import csv
import glob
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlvfs_amd import lib, mlvfile, synth

W, H = 3584, 1320


def write_source(root, frames):
    """eight different frames, repeated: the encoder's work depends on the content, not on its novelty -> (directory, the frames)"""
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    src = os.path.join(root, "src")
    os.mkdir(src)
    mlvfile.write_clip(os.path.join(src, "B.MLV"), [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return src, base


def timed(a, frm, dst, lj92, bits=None, loops=None):
    """-> (stats, best seconds of `loops` calls after a first one that warms the page cache, the code objects and the staging)"""
    best = None
    for loop in range((a.loops if loops is None else loops) + 1):
        shutil.rmtree(dst, ignore_errors=True)
        os.mkdir(dst)
        with mlvfile.MlvReader(os.path.join(frm, "B.MLV")) as r:
            t0 = time.perf_counter()
            s = r.transcode(os.path.join(dst, "B.MLV"), lj92=lj92, batch=a.batch, io_threads=a.io_threads, bits=bits)
            dt = time.perf_counter() - t0
        if loop and (best is None or dt < best):
            best = dt
    return s, best


def report(what, s, best, loops):
    print(f"{what}: {s['frames']} frames, best of {loops}: {best:.3f} s = {s['frames'] / best:.1f} frames/s, {best / s['frames'] * 1e3:.2f} ms/frame;"
          f" payload bytes {s['bytes_in']} -> {s['bytes_out']} (x{s['bytes_out'] / s['bytes_in']:.3f})")


# ---- --bits: the profiled child and its report (the pattern of tools/dark_bench.py) ---------------------------------------------
def child(a) -> int:
    """what the profiler watches"""
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    src, n = os.path.join(a.dir, "src"), a.bits[0]
    lj = os.path.join(a.dir, "c_lj92")
    timed(a, src, lj, True, loops=1)
    timed(a, src, os.path.join(a.dir, "c_plain_n"), False, n, loops=1)
    timed(a, src, os.path.join(a.dir, "c_lj92_n"), True, n, loops=1)
    timed(a, lj, os.path.join(a.dir, "c_back_n"), False, n, loops=1)
    timed(a, lj, os.path.join(a.dir, "c_lj_lj_n"), True, n, loops=1)
    return 0


def kernel_report(a) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    n = a.bits[0]
    out = os.path.join(a.dir, "prof")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "bits", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--dir", a.dir, "--frames", str(a.frames), "--batch", str(a.batch),
           "--io-threads", str(a.io_threads), "--bits", str(n)]
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        so, se = p.communicate(timeout=a.child_limit + 30)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        so, se = p.communicate()
    if p.returncode != 0:
        print(f"the profiled run ended with status {p.returncode}; nothing more is run on the GPU:", so[-2000:], se[-2000:])
        return False
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        print("no kernel_stats.csv under", out, [os.path.relpath(f, out) for f in glob.glob(os.path.join(out, "**", "*"), recursive=True)][:20])
        return True
    rows = list(csv.DictReader(open(stats[0])))
    fused, second = f"k_mlv_repack_x16<14,{n}>", f"k_mlv_pack_x16<{n},true>"
    kernels = ["k_unpack_x16<14>", "k_mlv_tile_x<16,false>", fused, "k_mlv_unpack_shift_x16<14>", second, "k_mlv_tile_x<16,true>"]
    print(f"kernel times, {a.frames} frames in batches of {a.batch} (one launch = one batch; us per frame = launch / {a.batch}):")
    found = {}
    for want in kernels:
        for row in rows:
            if row["Name"].replace("mlv::", "").replace("void ", "").replace(" ", "").startswith(want + "("):
                found[want] = [float(row[k]) / 1e3 / a.batch for k in ("AverageNs", "MinNs", "MaxNs")] + [int(row["Calls"])]
                avg, lo, hi, calls = found[want]
                print(f"  {want:28s} {calls:3d} launches   avg {avg:7.2f}   min {lo:7.2f}   max {hi:7.2f}   spread {hi - lo:6.2f}")
    if all(k in found for k in ("k_unpack_x16<14>", fused, second)):
        u, f, s = found["k_unpack_x16<14>"], found[fused], found[second]
        print(f"  fused {f[0]:.2f} against two passes {u[0] + s[0]:.2f} us per frame: {u[0] + s[0] - f[0]:.2f} saved; the spread of k_unpack_x16<14>'s launches is {u[2] - u[1]:.2f}")
    return True


def bits_main(a, root) -> int:
    src, _ = write_source(root, a.frames)
    if not a.skip_kernels and not kernel_report(a):                         # before this process opens the GPU itself
        return 1
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    report("plain->lj92 at 14 bits (no conversion)", *timed(a, src, os.path.join(root, "lj92"), True), a.loops)
    for n in a.bits:
        report(f"plain->plain at {n} bits", *timed(a, src, os.path.join(root, "plain_n"), False, n), a.loops)
        report(f"plain->lj92 at {n} bits", *timed(a, src, os.path.join(root, "lj92_n"), True, n), a.loops)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--loops", type=int, default=3)
    ap.add_argument("--io-threads", type=int, default=0)
    ap.add_argument("--dir", default=None, help="where the clips go (default: a temporary directory)")
    ap.add_argument("--bits", type=int, nargs="+", metavar="N", help="rewrite at N bits per pixel (8..16) instead of the round trip")
    ap.add_argument("--skip-kernels", action="store_true", help="--bits: no profiled child run")
    ap.add_argument("--child-limit", type=int, default=300, help="--bits: seconds the profiled child run may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.bits and not all(8 <= n <= 16 for n in a.bits):
        ap.error("--bits takes 8 to 16")
    if a.child:
        return child(a)
    root = tempfile.mkdtemp(prefix="mlvtc_", dir=a.dir)
    if a.bits:
        a.dir = root
        try:
            return bits_main(a, root)
        finally:
            shutil.rmtree(root, ignore_errors=True)
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    try:
        src, base = write_source(root, a.frames)
        res = {}
        for what, frm, lj92 in (("plain->lj92", src, True), ("lj92->plain", os.path.join(root, "lj92"), False)):
            res[what] = timed(a, frm, os.path.join(root, "lj92" if lj92 else "plain"), lj92)
            report(what, *res[what], a.loops)
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

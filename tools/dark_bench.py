"""Dark frames at 3584x1320 (csrc/cal.cpp, csrc/k_cal.hip): the numbers of DESIGN.md 3.8.

    python tools/dark_bench.py [--frames 32] [--batch 8] [--reps 3] [--dir DIR] [--skip-kernels]

1. Kernel times.  The tool starts ITSELF once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, the
   program behind `--`); that child runs, on 32 frames in batches of 8 and in one process,
       the mount without options, without and with a dark frame    k_unpack_x16<14>  |  k_cal_unpack_x16<14, true, false> (the fused pass)
       mlvfs_amd_unpack_dev + mlvfs_amd_dark_subtract_dev          k_unpack_x16<14>, k_cal_apply_x16<true, false> (the two passes it replaces)
       mlvfs_amd_lj92_tile_dev                                     k_mlv_tile_x<16, false>
       mlvfs_amd_dark_from_clip                                    k_unpack_x16<14>, k_dark_accum_x16, k_dark_mean
   and the parent prints every kernel's time per frame side by side, with the spread of its launches.
2. The mount's frames per second with and without a dark frame for cs5x5 + bad pixels + stripes, in alternating repetitions.
3. mlvfs_amd_dark_from_clip: milliseconds for the clip's frames, file reads included."""
import argparse
import csv
import ctypes as C
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
from mlvfs_amd.dark import Dark
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

W, H = 3584, 1320
KERNELS = ["k_unpack_x16<14>", "k_mlv_tile_x<16, false>", "k_cal_unpack_x16<14, true, false>", "k_cal_apply_x16<true, false>", "k_dark_accum_x16", "k_dark_mean"]


def plane():
    """the pedestal, a column pattern and a little noise; no hot entries: they would become bad pixels of the subtracted clip, and the
    mount's two arms would differ in the size of the repair map, not in the subtraction"""
    rng = np.random.default_rng(3)
    p = synth.BLACK + rng.integers(-5, 6, (H, W)) + (np.arange(W) % 8 == 3) * 9
    return p.astype(np.uint16)


def write_clip(root, frames):
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    path = os.path.join(root, "B.MLV")
    mlvfile.write_clip(path, [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return path, packed


def child(a) -> int:
    """what the profiler watches"""
    import torch
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    path = os.path.join(a.dir, "B.MLV")
    n = a.batch
    with mlvfile.MlvReader(path) as r, Dark.from_plane(plane(), 14, synth.BLACK) as dark:
        for d in (None, dark, None, dark):                                   # the second round is the warm one; all launches are listed
            with Mount(r, MlvfsOptions(), basename="/B.MLV", dark=d) as m:
                m.dng(0, a.frames, batch=n)
        packed = r.read_frames(0, n, W * H * 14 // 8 + 16)
        dp = torch.from_numpy(packed).cuda()
        frames = torch.zeros((n, H, W), dtype=torch.int16, device="cuda")
        tiled = torch.zeros_like(frames)
        geom = lib.Geom(W, H, 14, synth.BLACK, synth.WHITE, 0, 0)
        for _ in range(a.frames // n):
            lib.check(L.mlvfs_amd_unpack_dev(C.byref(geom), C.c_void_p(dp.data_ptr()), packed.shape[1], C.c_void_p(frames.data_ptr()), W * H * 2, n, None))
            lib.check(L.mlvfs_amd_dark_subtract_dev(dark.h, C.byref(geom), C.c_void_p(frames.data_ptr()), W * H * 2, n, None))
            lib.check(L.mlvfs_amd_lj92_tile_dev(C.c_void_p(frames.data_ptr()), W * H * 2, C.c_void_p(tiled.data_ptr()), W * H * 2, W, H, n, None))
        torch.cuda.synchronize()
        Dark.from_clip(r, 0, a.frames, batch=n).close()
    return 0


def kernel_report(a) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    out = os.path.join(a.dir, "prof")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "dark", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--dir", a.dir, "--frames", str(a.frames), "--batch", str(a.batch)]
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
    print(f"kernel times, {a.frames} frames in batches of {a.batch} (one launch = one batch; us per frame = launch / {a.batch}; k_dark_mean: one plane):")
    found = {}
    for want in KERNELS:
        for row in rows:
            if row["Name"].replace("mlv::", "").replace("void ", "").startswith(want + "("):
                per = 1 if want == "k_dark_mean" else a.batch
                found[want] = [float(row[k]) / 1e3 / per for k in ("AverageNs", "MinNs", "MaxNs")] + [int(row["Calls"])]
                avg, lo, hi, calls = found[want]
                print(f"  {want:24s} {calls:3d} launches   avg {avg:7.2f}   min {lo:7.2f}   max {hi:7.2f}   spread {hi - lo:6.2f}")
    if all(k in found for k in KERNELS[:4] if k != "k_mlv_tile_x<16, false>"):
        u, f, s = found["k_unpack_x16<14>"], found["k_cal_unpack_x16<14, true, false>"], found["k_cal_apply_x16<true, false>"]
        print(f"  fused {f[0]:.2f} against two passes {u[0] + s[0]:.2f} us per frame: {u[0] + s[0] - f[0]:.2f} saved; the spread of k_unpack_x16<14>'s launches is {u[2] - u[1]:.2f}")
    return True


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the clip and the profile go (default: a temporary directory)")
    ap.add_argument("--skip-kernels", action="store_true", help="no profiled child run")
    ap.add_argument("--child-limit", type=int, default=300, help="seconds the profiled child run may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    root = tempfile.mkdtemp(prefix="darkbench_", dir=a.dir)
    a.dir = root
    try:
        path, _ = write_clip(root, a.frames)
        if not a.skip_kernels and not kernel_report(a):                     # before this process opens the GPU itself
            return 1
        L = lib.load()
        assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
        opt = MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)
        with mlvfile.MlvReader(path) as r, Dark.from_plane(plane(), 14, synth.BLACK) as dark:
            fps = {False: [], True: []}
            for rep in range(a.reps + 1):                                    # the first repetition warms page cache, code objects, staging
                for with_dark in (False, True):
                    L.free_focus_pixel_maps()
                    with Mount(r, opt, basename="/B.MLV", dark=dark if with_dark else None) as m:
                        t0 = time.perf_counter()
                        m.dng(0, a.frames, batch=a.batch)
                        dt = time.perf_counter() - t0
                    if rep:
                        fps[with_dark].append(a.frames / dt)
            for with_dark in (False, True):
                v = fps[with_dark]
                print(f"mount, cs5x5 + bad pixels + stripes, {'with a' if with_dark else 'without'} dark frame: {np.median(v):.1f} frames/s"
                      f" (median of {len(v)} alternating repetitions: {', '.join(f'{x:.1f}' for x in v)}), file reads and downloads included")
            print("  (one machine, one run: the difference is that of one box)")
            ms = []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                Dark.from_clip(r, 0, a.frames, batch=a.batch).close()
                if rep:
                    ms.append((time.perf_counter() - t0) * 1e3)
            print(f"mlvfs_amd_dark_from_clip, {a.frames} frames in batches of {a.batch}, file reads included: {np.median(ms):.1f} ms"
                  f" (median of {len(ms)}: {', '.join(f'{x:.1f}' for x in ms)})")
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

"""Resampled rendered frames demosaiced by AMaZE at 3584x1320 (csrc/k_amaze_resample.hip, csrc/amaze_render.cpp, csrc/mount.cpp): the
numbers of DESIGN.md 3.20.

    python tools/amaze_resample_bench.py [--frames 32] [--batch 8] [--reps 3] [--quality 90] [--dir DIR] [--skip-kernels]

1. Kernel times.  The tool starts ITSELF once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, the
   program behind `--`, under a time limit); that child serves the clip through the mount with cs5x5 + bad pixels + stripes as TIFF
   files through the AMaZE-resampled route at 1920x707 and 2560x943, the AMaZE full-size route and the linear resampled route at
   1920x707, and the parent prints, per frame, k_amz_resample_x16 at both sizes (told apart by their grids in the trace) beside
   k_amz_tone_x16 and k_resample_x16 of the same run.
2. The mount's frames per second, file reads and downloads included, for those four TIFF routes and the AMaZE-resampled JPEG route at
   1920x707, in alternating repetitions within one run, with the bytes per file of each."""
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
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

W, H = 3584, 1320
SMALL, LARGE = (1920, 707), (2560, 943)
# (label, kind, route, size): route "amaze" resamples the AMaZE rendering, "full" is the AMaZE full-size route, "linear" the linear resampled one
ROUTES = [(f"TIFF, AMaZE resampled {SMALL[0]}x{SMALL[1]}", "rgb", "amaze", SMALL), (f"TIFF, AMaZE resampled {LARGE[0]}x{LARGE[1]}", "rgb", "amaze", LARGE),
          ("TIFF, AMaZE full size", "rgb", "full", None), (f"TIFF, linear resampled {SMALL[0]}x{SMALL[1]}", "rgb", "linear", SMALL),
          (f"JPEG, AMaZE resampled {SMALL[0]}x{SMALL[1]}", "jpeg", "amaze", SMALL)]
PROFILED = ROUTES[:4]


def options():
    return MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)


def write_clip(root, frames):
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    path = os.path.join(root, "B.MLV")
    mlvfile.write_clip(path, [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return path


def serve(L, r, a, kind, route, size):
    """one fresh handle serves the clip -> (seconds, mean bytes per file)"""
    L.free_focus_pixel_maps()
    with Mount(r, options(), basename="/B.MLV") as m:
        if route == "amaze":
            m.set_resample_demosaic("amaze")
        if route == "full":
            m.set_demosaic("amaze")
        how = dict(full=True) if route == "full" else dict(size=size, resample=True)
        t0 = time.perf_counter()
        if kind == "jpeg":
            files, flags = m.jpeg(0, a.frames, quality=a.quality, batch=a.batch, **how)
            dt = time.perf_counter() - t0
            assert not any(flags), "a frame was served as its TIFF"
            return dt, sum(len(f) for f in files) / len(files)
        files = m.rgb(0, a.frames, batch=a.batch, **how)
        return time.perf_counter() - t0, files.shape[1]


def child(a) -> int:
    """what the profiler watches"""
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r:
        for _ in range(2):                                                   # the second round is the warm one; all launches are listed
            for _, kind, route, size in PROFILED:
                serve(L, r, a, kind, route, size)
    return 0


def workgroups(L, size, batch):
    """of one launch of k_amz_resample_x16 for a batch (host code: mlvfs_amd_test_amz_resample_plan)"""
    out = np.zeros(8, np.int32)
    lib.check(L.mlvfs_amd_test_amz_resample_plan(W, H, size[0], size[1], batch, lib.ptr(out)), "test_amz_resample_plan")
    assert out[0] == 1, "the size does not take the fast form"
    return int(out[3]) * int(out[5])


def kernel_report(a) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    out = os.path.join(a.dir, "prof")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "amaze_resample", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--dir", a.dir, "--frames", str(a.frames), "--batch", str(a.batch), "--quality", str(a.quality)]
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        so, se = p.communicate(timeout=a.child_limit + 30)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        so, se = p.communicate()
    if p.returncode != 0:
        print(f"the profiled run ended with status {p.returncode}; nothing more is run on the GPU:", so[-2000:], se[-2000:])
        return False
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        print("no kernel_trace.csv under", out, [os.path.relpath(f, out) for f in glob.glob(os.path.join(out, "**", "*"), recursive=True)][:20])
        return True
    rows = list(csv.DictReader(open(trace[0])))
    served = 2 * a.frames                                                    # two rounds of every profiled route
    total = {}                                                               # (kernel, workgroups of the launch in x) -> [ns, launches]
    for row in rows:
        name = row["Kernel_Name"].replace("mlv::", "").replace("void ", "").split("(")[0].split("<")[0]
        wg = int(row["Grid_Size_X"]) // max(int(row["Workgroup_Size_X"]), 1)
        t = total.setdefault((name, wg), [0, 0])
        t[0] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
        t[1] += 1
    L = lib.load()                                                           # host code alone: the plan
    per = {}
    print(f"kernel times, {a.frames} frames in batches of {a.batch} (us per frame = total time of the kernel in a route / frames that route served):")
    for size in (SMALL, LARGE):
        wg = workgroups(L, size, a.batch)
        hit = total.get(("k_amz_resample_x16", wg))
        if hit:
            per[size] = hit[0] / 1e3 / served
            moved = (12 * W * H + 3 * size[0] * size[1]) / 1e6
            print(f"  k_amz_resample_x16 {size[0]}x{size[1]}  {hit[1]:4d} launches of {wg} workgroups a frame  {per[size]:8.2f} us per frame,"
                  f" {moved:6.2f} MB per frame: {moved / per[size]:.2f} TB/s")
    for want, moved in (("k_amz_tone_x16", 15 * W * H / 1e6), ("k_resample_x16", (2 * W * H + 3 * SMALL[0] * SMALL[1]) / 1e6), ("k_amz_balance_x16", 6 * W * H / 1e6)):
        ns = sum(v[0] for (name, _), v in total.items() if name == want)
        n = sum(v[1] for (name, _), v in total.items() if name == want)
        routes = 3 if want == "k_amz_balance_x16" else 1                     # the balance pass runs in all three AMaZE routes
        if n:
            per[want] = ns / 1e3 / (served * routes)
            print(f"  {want:32s} {n:4d} launches                              {per[want]:8.2f} us per frame, {moved:6.2f} MB per frame: {moved / per[want]:.2f} TB/s")
    for want in ("k_amaze", "k_amaze_rows"):
        ns = sum(v[0] for (name, _), v in total.items() if name == want)
        if ns:
            print(f"  {want:32s}                                            {ns / 1e3 / (served * 3):8.2f} us per frame")
    if "k_amz_tone_x16" in per:
        for size in (SMALL, LARGE):
            if size in per:
                ratio = per[size] / per["k_amz_tone_x16"]
                print(f"  k_amz_resample_x16 at {size[0]}x{size[1]} takes {ratio:.2f} x k_amz_tone_x16's time (expected: at most 1.25): {'met' if ratio <= 1.25 else 'MISSED'}")
    missing = [k for k in (SMALL, LARGE, "k_amz_tone_x16", "k_resample_x16") if k not in per]
    if missing:
        print("  kernels missing from the trace:", missing, sorted({k for k in total})[:60])
    return True


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--dir", default=None, help="where the clip and the profile go (default: a temporary directory)")
    ap.add_argument("--skip-kernels", action="store_true", help="no profiled child run")
    ap.add_argument("--child-limit", type=int, default=300, help="seconds the profiled child run may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    root = tempfile.mkdtemp(prefix="amazersbench_", dir=a.dir)
    a.dir = root
    try:
        path = write_clip(root, a.frames)
        if not a.skip_kernels and not kernel_report(a):                     # before this process opens the GPU itself
            return 1
        L = lib.load()
        assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
        took = {label: [] for label, _, _, _ in ROUTES}
        size = {}
        with mlvfile.MlvReader(path) as r:
            for rep in range(a.reps + 1):                                    # the first repetition warms page cache, code objects and work memory
                for label, kind, route, sz in ROUTES:
                    dt, size[label] = serve(L, r, a, kind, route, sz)
                    if rep:
                        took[label].append(dt)
        print(f"mount, cs5x5 + bad pixels + stripes, {a.frames} frames of {W}x{H} in batches of {a.batch}, JPEG quality {a.quality}, file reads and downloads included:")
        med, scatter = {}, {}
        for label, v in took.items():
            fps = [a.frames / t for t in v]
            med[label], scatter[label] = float(np.median(fps)), max(fps) - min(fps)
            print(f"  {label:36s} {med[label]:7.1f} frames/s (median of {len(fps)} alternating repetitions: {', '.join(f'{x:.1f}' for x in fps)};"
                  f" scatter {scatter[label]:.1f}), {size[label]:9.0f} bytes per file")
        small, full = ROUTES[0][0], ROUTES[2][0]
        margin = max(scatter[small], scatter[full])
        print(f"  AMaZE resampled {SMALL[0]}x{SMALL[1]} / AMaZE full size = {med[small] / med[full]:.2f} (expected: no fewer frames per second, the repetitions'"
              f" scatter of {margin:.1f} frames/s the margin): {'met' if med[small] + margin >= med[full] else 'MISSED'}")
        print("  (one machine, one run: the differences are those of one box)")
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

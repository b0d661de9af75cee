"""Rendered frames resampled from the full-size rendering at 3584x1320 (csrc/k_resample.hip, csrc/mount.cpp): the numbers of
DESIGN.md 3.18.

    python tools/resample_bench.py [--frames 32] [--batch 8] [--reps 3] [--quality 90] [--dir DIR] [--skip-kernels]

1. Kernel times.  The tool starts ITSELF once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, the
   program behind `--`, under a time limit); that child serves the clip through the mount with cs5x5 + bad pixels + stripes on every
   route, and the parent prints k_resample_x16 per frame at each of the two sizes -- its launches told apart by their place in the
   child's order -- beside k_render1_x16 (and k_render2_x16, k_scale_x16) of the same run, with the ratio of the two times (the
   yardstick: 1.25).
2. The mount's frames per second, file reads and downloads included, for the routes -- full-size .dng, half-size TIFF, full-size TIFF
   and the resampled TIFF and JPEG at 1920x707 and 2560x943 -- in alternating repetitions within one run, with the bytes per file of
   each, and each resampled TIFF's rate over the full-size TIFF's (the yardstick: no fewer, within the scatter)."""
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
SIZES = [(1920, 707), (2560, 943)]
# (label, kind, full, size, resample)
ROUTES = [("full-size .dng", "dng", False, None, False), ("half-size TIFF", "rgb", False, None, False), ("full-size TIFF", "rgb", True, None, False),
          ("1280x472 scaled TIFF", "rgb", False, (1280, 472), False)]
ROUTES += [(f"{ow}x{oh} {kind}", route, False, (ow, oh), True) for ow, oh in SIZES for kind, route in (("TIFF", "rgb"), ("JPEG", "jpeg"))]


def options():
    return MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)


def write_clip(root, frames):
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    path = os.path.join(root, "B.MLV")
    mlvfile.write_clip(path, [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return path


def serve(L, r, a, kind, full, size, resample):
    """one fresh handle serves the clip -> (seconds, mean bytes per file)"""
    L.free_focus_pixel_maps()
    with Mount(r, options(), basename="/B.MLV") as m:
        t0 = time.perf_counter()
        if kind == "jpeg":
            files, flags = m.jpeg(0, a.frames, quality=a.quality, batch=a.batch, full=full, size=size, resample=resample)
            dt = time.perf_counter() - t0
            assert not any(flags), "a frame was served as its TIFF"
            return dt, sum(len(f) for f in files) / len(files)
        files = m.rgb(0, a.frames, batch=a.batch, full=full, size=size, resample=resample) if kind == "rgb" else m.dng(0, a.frames, batch=a.batch)
        return time.perf_counter() - t0, files.shape[1]


def child(a) -> int:
    """what the profiler watches"""
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r:
        for _ in range(2):                                                   # the second round is the warm one; all launches are listed
            for _, kind, full, size, resample in ROUTES:
                serve(L, r, a, kind, full, size, resample)
    return 0


def short(name):
    return name.replace("mlv::", "").replace("void ", "")


def kernel_report(a) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    out = os.path.join(a.dir, "prof")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "resample", "--",
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
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not stats:
        print("no kernel_stats.csv under", out, [os.path.relpath(f, out) for f in glob.glob(os.path.join(out, "**", "*"), recursive=True)][:20])
        return True
    rows = list(csv.DictReader(open(stats[0])))
    print(f"kernel times, {a.frames} frames in batches of {a.batch} (one launch = one batch; us per frame = launch / {a.batch}):")
    full = None
    for row in rows:
        for want in ("k_render1_x16", "k_render2_x16", "k_scale_x16", "k_resample_x16", "k_resample_generic"):
            if short(row["Name"]).startswith(want + "("):
                avg, lo, hi = (float(row[k]) / 1e3 / a.batch for k in ("AverageNs", "MinNs", "MaxNs"))
                note = " (both sizes together)" if want.startswith("k_resample") else ""
                print(f"  {want:20s} {int(row['Calls']):3d} launches   avg {avg:7.2f}   min {lo:7.2f}   max {hi:7.2f} us per frame{note}")
                if want == "k_render1_x16":
                    full = avg
    if not trace:
        print("  no kernel_trace.csv: the sizes cannot be told apart")
        return True
    launches = sorted((r for r in csv.DictReader(open(trace[0])) if short(r.get("Kernel_Name", "")).startswith("k_resample_x16(")),
                      key=lambda r: int(r["Start_Timestamp"]))
    # the child's order: two rounds; in each, per size the TIFF route and then the JPEG route, a launch per batch
    per = 2 * -(-a.frames // a.batch)
    if len(launches) != 2 * len(SIZES) * per:
        print(f"  the trace lists {len(launches)} launches of k_resample_x16, not {2 * len(SIZES) * per}: the sizes cannot be told apart")
        return True
    for k, size in enumerate(SIZES):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 / a.batch for n, r in enumerate(launches) if n % (len(SIZES) * per) // per == k]
        avg = float(np.mean(us))
        ratio = f", {avg / full:.2f} x k_render1_x16's time (yardstick: 1.25)" if full else ""
        print(f"  k_resample_x16 to {size[0]:4d}x{size[1]:<4d} {len(us):3d} launches   avg {avg:7.2f}   min {min(us):7.2f}   max {max(us):7.2f} us per frame{ratio}")
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
    root = tempfile.mkdtemp(prefix="resamplebench_", dir=a.dir)
    a.dir = root
    try:
        path = write_clip(root, a.frames)
        if not a.skip_kernels and not kernel_report(a):                     # before this process opens the GPU itself
            return 1
        L = lib.load()
        assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
        took = {route[0]: [] for route in ROUTES}
        nbytes = {}
        with mlvfile.MlvReader(path) as r:
            for rep in range(a.reps + 1):                                    # the first repetition warms page cache, code objects and staging
                for label, kind, full, size, resample in ROUTES:
                    dt, nbytes[label] = serve(L, r, a, kind, full, size, resample)
                    if rep:
                        took[label].append(dt)
        print(f"mount, cs5x5 + bad pixels + stripes, {a.frames} frames of {W}x{H} in batches of {a.batch}, JPEG quality {a.quality}, file reads and downloads included:")
        med = {}
        for label, v in took.items():
            fps = [a.frames / t for t in v]
            med[label] = float(np.median(fps))
            print(f"  {label:20s} {med[label]:7.1f} frames/s (median of {len(fps)} alternating repetitions: {', '.join(f'{x:.1f}' for x in fps)};"
                  f" scatter {max(fps) - min(fps):.1f}), {nbytes[label]:9.0f} bytes per file")
        for ow, oh in SIZES:
            print(f"  {ow}x{oh} TIFF / full-size TIFF = {med[f'{ow}x{oh} TIFF'] / med['full-size TIFF']:.2f} (yardstick: 1 or better, within the scatter)")
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

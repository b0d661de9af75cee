"""Rendered JPEG frames at 4:2:0, 4:2:2 and 4:4:4 chroma sampling at 3584x1320 (csrc/k_jpeg.hip, csrc/mount.cpp): the numbers of
DESIGN.md 3.21.

    python tools/jpeg_sampling_bench.py [--frames 32] [--batch 8] [--reps 3] [--quality 90] [--dir DIR] [--skip-kernels]

1. Kernel times.  The tool starts ITSELF under `rocprofv3 --kernel-trace` (runs of their own, no counters, the program behind `--`,
   under a time limit), once for the half-size and once for the full-size route; the child serves the clip through the mount with
   cs5x5 + bad pixels + stripes at the three samplings in turn, twice.  The parent sorts the launches by their start, gives the four
   kernels that all samplings share (k_jpg_rows, k_jpg_count_ff, k_jpg_place, k_jpg_stuff) to the sampling of the k_jpg_transform*
   launch in front of them, and prints each kernel's median per frame at each sampling, with the ratio to 4:2:0 beside the ratio of
   blocks per pixel (1.33 at 4:2:2, 2.0 at 4:4:4) that a stage whose work is per block would show.
2. The mount's frames per second, file reads and downloads included, of the half-size and the full-size JPEG route at the three
   samplings, in alternating repetitions within one run, with the bytes per file of each."""
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
SAMPLINGS = ["4:2:0", "4:2:2", "4:4:4"]
SUFFIX = {"4:2:0": "", "4:2:2": "_422", "4:4:4": "_444"}
BLOCKS = {"4:2:0": 1.0, "4:2:2": 4 / 3, "4:4:4": 2.0}          # blocks per pixel, relative to 4:2:0
PER_SAMPLING = ["k_jpg_transform", "k_jpg_scan_bits", "k_jpg_emit"]
SHARED = ["k_jpg_rows", "k_jpg_count_ff", "k_jpg_place", "k_jpg_stuff"]
ORDER = ["k_jpg_transform", "k_jpg_scan_bits", "k_jpg_rows", "k_jpg_emit", "k_jpg_count_ff", "k_jpg_place", "k_jpg_stuff"]
ROUTES = [("half size", False), ("full size", True)]


def options():
    return MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)


def write_clip(root, frames):
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    path = os.path.join(root, "B.MLV")
    mlvfile.write_clip(path, [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return path


def serve(L, r, a, full, sampling):
    """one fresh handle serves the clip as JPEG files -> (seconds, mean bytes per file, files served as their TIFF)"""
    L.free_focus_pixel_maps()
    with Mount(r, options(), basename="/B.MLV") as m:
        m.set_jpeg_sampling(sampling)
        t0 = time.perf_counter()
        files, flags = m.jpeg(0, a.frames, quality=a.quality, batch=a.batch, full=full)
        dt = time.perf_counter() - t0
        return dt, sum(len(f) for f in files) / len(files), sum(1 for f in flags if f)


def child(a) -> int:
    """what the profiler watches"""
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r:
        for _ in range(2):
            for sampling in SAMPLINGS:
                serve(L, r, a, a.child == "full", sampling)
    return 0


def short_name(name):
    return name.replace("void ", "").replace("mlv::", "").split("(")[0].strip()


def kernel_report(a, label, full) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    out = os.path.join(a.dir, "prof_full" if full else "prof_half")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "-f", "csv", "-d", out, "-o", "jpeg", "--",
           sys.executable, os.path.abspath(__file__), "--child", "full" if full else "half", "--dir", a.dir, "--frames", str(a.frames),
           "--batch", str(a.batch), "--quality", str(a.quality)]
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
    try:
        so, se = p.communicate(timeout=a.child_limit + 30)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        so, se = p.communicate()
    if p.returncode != 0:
        print(f"the profiled run ended with status {p.returncode}; nothing more is run on the GPU:", so[-2000:], se[-2000:])
        return False
    traces = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not traces:
        print("no kernel_trace.csv under", out, [os.path.relpath(f, out) for f in glob.glob(os.path.join(out, "**", "*"), recursive=True)][:20])
        return True
    rows = list(csv.DictReader(open(traces[0])))
    if not rows or not {"Kernel_Name", "Start_Timestamp", "End_Timestamp"} <= set(rows[0]):
        print("kernel_trace.csv has other columns than expected:", list(rows[0]) if rows else "none")
        return True
    rows.sort(key=lambda row: int(row["Start_Timestamp"]))
    times = {s: {} for s in SAMPLINGS}                       # sampling -> kernel -> [us per launch]
    current = None
    for row in rows:
        name, us = short_name(row["Kernel_Name"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
        for s in SAMPLINGS:
            for k in PER_SAMPLING:
                if name == k + SUFFIX[s]:
                    times[s].setdefault(k, []).append(us)
                    current = s
        if name in SHARED and current:
            times[current].setdefault(name, []).append(us)
    print(f"kernel times, {label} route, {a.frames} frames in batches of {a.batch}, quality {a.quality} (one launch = one batch; the median launch / {a.batch} = us per frame):")
    print(f"  {'kernel':18s}" + "".join(f"{s:>12s}" for s in SAMPLINGS) + "   4:2:2 / 4:2:0 (1.33)   4:4:4 / 4:2:0 (2.00)")
    total = {s: 0.0 for s in SAMPLINGS}
    for k in ORDER:
        med = {s: float(np.median(times[s][k])) / a.batch if times[s].get(k) else float("nan") for s in SAMPLINGS}
        for s in SAMPLINGS:
            total[s] += med[s]
        print(f"  {k:18s}" + "".join(f"{med[s]:12.2f}" for s in SAMPLINGS) + f"   {med['4:2:2'] / med['4:2:0']:20.2f}   {med['4:4:4'] / med['4:2:0']:20.2f}"
              f"   ({len(times['4:2:0'].get(k, []))} launches each)")
    print(f"  {'the seven together':18s}" + "".join(f"{total[s]:12.2f}" for s in SAMPLINGS)
          + f"   {total['4:2:2'] / total['4:2:0']:20.2f}   {total['4:4:4'] / total['4:2:0']:20.2f}")
    for s in SAMPLINGS[1:]:
        r = total[s] / total["4:2:0"]
        print(f"  {s}: {r:.2f} x the 4:2:0 kernels' time, expected {BLOCKS[s]:.2f} x from the blocks per pixel: {'met' if r <= 1.05 * BLOCKS[s] else 'missed'}")
    return True


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--dir", default=None, help="where the clip and the profiles go (default: a temporary directory)")
    ap.add_argument("--skip-kernels", action="store_true", help="no profiled child runs")
    ap.add_argument("--child-limit", type=int, default=240, help="seconds a profiled child run may take")
    ap.add_argument("--child", choices=("half", "full"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    root = tempfile.mkdtemp(prefix="jpegsampling_", dir=a.dir)
    a.dir = root
    try:
        path = write_clip(root, a.frames)
        if not a.skip_kernels:                                                # before this process opens the GPU itself
            for label, full in ROUTES:
                if not kernel_report(a, label, full):
                    return 1
        L = lib.load()
        assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
        cases = [(label, full, s) for label, full in ROUTES for s in SAMPLINGS]
        took = {c: [] for c in cases}
        size, tiffs = {}, {}
        with mlvfile.MlvReader(path) as r:
            for rep in range(a.reps + 1):                                    # the first repetition warms page cache, code objects and staging
                for c in cases:
                    dt, size[c], tiffs[c] = serve(L, r, a, c[1], c[2])
                    if rep:
                        took[c].append(dt)
        print(f"mount, cs5x5 + bad pixels + stripes, {a.frames} frames of {W}x{H} in batches of {a.batch}, JPEG quality {a.quality}, file reads and downloads included:")
        for c, v in took.items():
            fps = [a.frames / t for t in v]
            print(f"  {c[0]:10s} {c[2]}  {np.median(fps):7.1f} frames/s (median of {len(fps)} alternating repetitions: {', '.join(f'{x:.1f}' for x in fps)};"
                  f" scatter {max(fps) - min(fps):.1f}), {size[c]:9.0f} bytes per file" + (f", {tiffs[c]} served as TIFF" if tiffs[c] else ""))
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

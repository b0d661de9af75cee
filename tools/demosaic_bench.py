"""Rendered full-size sRGB frames at 3584x1320 (csrc/k_demosaic.hip, csrc/mount.cpp): the numbers of DESIGN.md 3.14.

    python tools/demosaic_bench.py [--frames 32] [--batch 8] [--reps 3] [--quality 90] [--dir DIR] [--skip-kernels]

1. Kernel times.  The tool starts ITSELF once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, the
   program behind `--`, under a time limit); that child serves the clip through the mount with cs5x5 + bad pixels + stripes on the
   five routes, and the parent prints k_render1_x16 per frame beside k_render2_x16 and k_unpack_x16<14> of the same run, with the
   bytes each moves, the time per output pixel of the two renderings and their ratio (the yardstick: 1.5), and the linear-copy floor
   for the full-size rendering's bytes at the rate tools/stream_floor.hip measured (6.2 TB/s).
2. The mount's frames per second, file reads and downloads included, for the five routes -- full-size .dng, half-size TIFF, full-size
   TIFF, half-size JPEG, full-size JPEG -- in alternating repetitions within one run, with the bytes per file of each, and the
   full-size TIFF's rate over the .dng's (the yardstick: 0.67, the ratio of the bytes that cross the link)."""
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
# bytes a kernel reads + writes per frame, and the pixels it writes (None: not a rendering)
KERNELS = {"k_unpack_x16<14>": (W * H * 3.75, None), "k_render2_x16": (W * H * 2 + (W // 2) * (H // 2) * 3, (W // 2) * (H // 2)),
           "k_render1_x16": (W * H * 2 + W * H * 3, W * H), "k_render1_generic": (W * H * 2 + W * H * 3, W * H)}
COPY_FLOOR_TBS = 6.2                     # tools/stream_floor.hip's linear copy
ROUTES = [("full-size .dng", "dng", False), ("half-size TIFF", "rgb", False), ("full-size TIFF", "rgb", True), ("half-size JPEG", "jpeg", False),
          ("full-size JPEG", "jpeg", True)]


def options():
    return MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)


def write_clip(root, frames):
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    path = os.path.join(root, "B.MLV")
    mlvfile.write_clip(path, [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return path


def serve(L, r, a, kind, full):
    """one fresh handle serves the clip -> (seconds, mean bytes per file)"""
    L.free_focus_pixel_maps()
    with Mount(r, options(), basename="/B.MLV") as m:
        t0 = time.perf_counter()
        if kind == "jpeg":
            files, flags = m.jpeg(0, a.frames, quality=a.quality, batch=a.batch, full=full)
            dt = time.perf_counter() - t0
            assert not any(flags), "a frame was served as its TIFF"
            return dt, sum(len(f) for f in files) / len(files)
        files = m.rgb(0, a.frames, batch=a.batch, full=full) if kind == "rgb" else m.dng(0, a.frames, batch=a.batch)
        return time.perf_counter() - t0, files.shape[1]


def child(a) -> int:
    """what the profiler watches"""
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r:
        for _ in range(2):                                                   # the second round is the warm one; all launches are listed
            for _, kind, full in ROUTES:
                serve(L, r, a, kind, full)
    return 0


def kernel_report(a) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    out = os.path.join(a.dir, "prof")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "demosaic", "--",
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
    if not stats:
        print("no kernel_stats.csv under", out, [os.path.relpath(f, out) for f in glob.glob(os.path.join(out, "**", "*"), recursive=True)][:20])
        return True
    rows = list(csv.DictReader(open(stats[0])))
    print(f"kernel times, {a.frames} frames in batches of {a.batch} (one launch = one batch; us per frame = launch / {a.batch}):")
    found = {}
    for want, (moved, pixels) in KERNELS.items():
        for row in rows:
            if row["Name"].replace("mlv::", "").replace("void ", "").startswith(want + "("):
                avg, lo, hi = (float(row[k]) / 1e3 / a.batch for k in ("AverageNs", "MinNs", "MaxNs"))
                found[want] = avg
                per_pixel = f", {avg * 1e6 / pixels:.3f} ps per output pixel" if pixels else ""
                print(f"  {want:20s} {int(row['Calls']):3d} launches   avg {avg:7.2f}   min {lo:7.2f}   max {hi:7.2f} us per frame,"
                      f" {moved / 1e6:6.2f} MB per frame: {moved / 1e6 / avg:.2f} TB/s{per_pixel}")          # MB per us = TB/s
    if "k_render1_x16" in found and "k_render2_x16" in found:
        ratio = (found["k_render1_x16"] / KERNELS["k_render1_x16"][1]) / (found["k_render2_x16"] / KERNELS["k_render2_x16"][1])
        floor = KERNELS["k_render1_x16"][0] / 1e6 / COPY_FLOOR_TBS
        print(f"  k_render1_x16 per output pixel = {ratio:.2f} x k_render2_x16's (yardstick: 1.5); the linear-copy floor for its"
              f" {KERNELS['k_render1_x16'][0] / 1e6:.2f} MB at {COPY_FLOOR_TBS} TB/s is {floor:.2f} us: {found['k_render1_x16'] / floor:.2f} x the floor")
    missing = [k for k in ("k_unpack_x16<14>", "k_render2_x16", "k_render1_x16") if k not in found]
    if missing:
        print("  kernels missing from the profile:", missing, sorted({r["Name"][:60] for r in rows})[:40])
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
    root = tempfile.mkdtemp(prefix="demosaicbench_", dir=a.dir)
    a.dir = root
    try:
        path = write_clip(root, a.frames)
        if not a.skip_kernels and not kernel_report(a):                     # before this process opens the GPU itself
            return 1
        L = lib.load()
        assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
        took = {label: [] for label, _, _ in ROUTES}
        size = {}
        with mlvfile.MlvReader(path) as r:
            for rep in range(a.reps + 1):                                    # the first repetition warms page cache, code objects and staging
                for label, kind, full in ROUTES:
                    dt, size[label] = serve(L, r, a, kind, full)
                    if rep:
                        took[label].append(dt)
        print(f"mount, cs5x5 + bad pixels + stripes, {a.frames} frames of {W}x{H} in batches of {a.batch}, JPEG quality {a.quality}, file reads and downloads included:")
        med = {}
        for label, v in took.items():
            fps = [a.frames / t for t in v]
            med[label] = float(np.median(fps))
            print(f"  {label:16s} {med[label]:7.1f} frames/s (median of {len(fps)} alternating repetitions: {', '.join(f'{x:.1f}' for x in fps)};"
                  f" scatter {max(fps) - min(fps):.1f}), {size[label]:9.0f} bytes per file")
        print(f"  full-size TIFF / full-size .dng = {med['full-size TIFF'] / med['full-size .dng']:.2f} (yardstick: 0.67 or better);"
              f" full-size JPEG / full-size .dng = {med['full-size JPEG'] / med['full-size .dng']:.2f} (expected above 1)")
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

"""Rendered full-size frames demosaiced by AMaZE at 3584x1320 (csrc/k_amaze_render.hip, csrc/amaze_render.cpp, csrc/mount.cpp): the
numbers of DESIGN.md 3.19.

    python tools/amaze_render_bench.py [--frames 32] [--batch 8] [--reps 3] [--quality 90] [--dir DIR] [--skip-kernels]

1. Kernel times.  The tool starts ITSELF once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, the
   program behind `--`, under a time limit); that child serves the clip through the mount with cs5x5 + bad pixels + stripes as
   full-size TIFF, JPEG and 16-bit TIFF files with the linear filter and with AMaZE, and the parent prints, per frame, the two
   element-wise kernels with the bytes each moves and the rate that makes, the two AMaZE kernels, and k_render1_x16 of the same run,
   whose rate is the yardstick for the element-wise kernels' traffic floor.
2. The mount's frames per second, file reads and downloads included, for the six routes in alternating repetitions within one run,
   with the bytes per file of each, and each AMaZE route's rate over the linear one's."""
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

from mlvfs_amd import lib, look, mlvfile, synth
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

W, H = 3584, 1320
NPIX = W * H
# bytes a kernel reads + writes per frame (None: not an element-wise pass)
KERNELS = {"k_render1_x16": NPIX * 5, "k_render1_deep_x16": NPIX * 8, "k_amz_balance_x16": NPIX * 6, "k_amaze_rows": None, "k_amaze": None,
           "k_amz_tone_x16": NPIX * 15, "k_amz_tone_deep_x16": NPIX * 18}
KINDS = [("TIFF", "rgb"), ("JPEG", "jpeg"), ("16-bit TIFF", "rgb16")]
ROUTES = [(f"{name}, {dm}", kind, dm) for name, kind in KINDS for dm in ("linear", "amaze")]


def options():
    return MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)


def write_clip(root, frames):
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    path = os.path.join(root, "B.MLV")
    mlvfile.write_clip(path, [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return path


def serve(L, r, a, kind, dm, lk16):
    """one fresh handle serves the clip at full size -> (seconds, mean bytes per file)"""
    L.free_focus_pixel_maps()
    with Mount(r, options(), basename="/B.MLV") as m:
        if dm != "linear":
            m.set_demosaic(dm)
        t0 = time.perf_counter()
        if kind == "jpeg":
            files, flags = m.jpeg(0, a.frames, quality=a.quality, batch=a.batch, full=True)
            dt = time.perf_counter() - t0
            assert not any(flags), "a frame was served as its TIFF"
            return dt, sum(len(f) for f in files) / len(files)
        files = m.rgb(0, a.frames, batch=a.batch, full=True, look16=lk16 if kind == "rgb16" else None)
        return time.perf_counter() - t0, files.shape[1]


def child(a) -> int:
    """what the profiler watches"""
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r, look.Look16(look.shaper16("srgb")) as lk16:
        for _ in range(2):                                                   # the second round is the warm one; all launches are listed
            for _, kind, dm in ROUTES:
                serve(L, r, a, kind, dm, lk16)
    return 0


def kernel_report(a) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    out = os.path.join(a.dir, "prof")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "amaze_render", "--",
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
    print(f"kernel times, {a.frames} frames in batches of {a.batch} (us per frame = total time of the kernel / frames it served):")
    found = {}
    for want, moved in KERNELS.items():
        for row in rows:
            if row["Name"].replace("mlv::", "").replace("void ", "").startswith((want + "(", want + "<")):    # k_amaze_rows is a template
                # k_amaze runs several launches per batch and k_amaze_rows one: per frame = the kernel's total over the frames rendered
                # with it (the 8-bit kernels serve the TIFF and the JPEG route, the balance and AMaZE all three, the deep ones one; two rounds)
                routes = 3 if want in ("k_amaze", "k_amaze_rows", "k_amz_balance_x16") else 1 if "deep" in want else 2
                per_frame = float(row["TotalDurationNs"]) / 1e3 / (2 * routes * a.frames)
                found[want] = per_frame
                rate = f", {moved / 1e6:6.2f} MB per frame: {moved / 1e6 / per_frame:.2f} TB/s" if moved else ""   # MB per us = TB/s
                print(f"  {want:22s} {int(row['Calls']):4d} launches   {per_frame:8.2f} us per frame{rate}")
    if "k_render1_x16" in found:
        rate = KERNELS["k_render1_x16"] / 1e6 / found["k_render1_x16"]
        for k in ("k_amz_balance_x16", "k_amz_tone_x16", "k_amz_tone_deep_x16"):
            if k in found:
                floor = KERNELS[k] / 1e6 / rate
                print(f"  {k}: its {KERNELS[k] / 1e6:.1f} MB at k_render1_x16's {rate:.2f} TB/s would take {floor:.2f} us; it takes {found[k] / floor:.2f} x that")
    if "k_amaze" in found and "k_amaze_rows" in found:
        print(f"  AMaZE's two kernels: {found['k_amaze'] + found['k_amaze_rows']:.0f} us per frame summed (they overlap on two streams);"
              f" the dual-ISO profile's figures for them: 573 + 646 us (DESIGN.md 3.3)")
    missing = [k for k in KERNELS if k not in found]
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
    root = tempfile.mkdtemp(prefix="amazebench_", dir=a.dir)
    a.dir = root
    try:
        path = write_clip(root, a.frames)
        if not a.skip_kernels and not kernel_report(a):                     # before this process opens the GPU itself
            return 1
        L = lib.load()
        assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
        took = {label: [] for label, _, _ in ROUTES}
        size = {}
        with mlvfile.MlvReader(path) as r, look.Look16(look.shaper16("srgb")) as lk16:
            for rep in range(a.reps + 1):                                    # the first repetition warms page cache, code objects and work memory
                for label, kind, dm in ROUTES:
                    dt, size[label] = serve(L, r, a, kind, dm, lk16)
                    if rep:
                        took[label].append(dt)
        print(f"mount, cs5x5 + bad pixels + stripes, {a.frames} frames of {W}x{H} in batches of {a.batch} at full size, JPEG quality {a.quality}, file reads and downloads included:")
        med = {}
        for label, v in took.items():
            fps = [a.frames / t for t in v]
            med[label] = float(np.median(fps))
            print(f"  {label:20s} {med[label]:7.1f} frames/s (median of {len(fps)} alternating repetitions: {', '.join(f'{x:.1f}' for x in fps)};"
                  f" scatter {max(fps) - min(fps):.1f}), {size[label]:9.0f} bytes per file")
        for name, _ in KINDS:
            print(f"  {name}: AMaZE / linear = {med[name + ', amaze'] / med[name + ', linear']:.2f}")
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

"""Flat fields at 3584x1320 (csrc/cal.cpp, csrc/k_cal.hip): the numbers of DESIGN.md 3.10.

    python tools/flat_bench.py [--frames 32] [--batch 8] [--reps 3] [--dir DIR] [--skip-kernels]

1. Kernel times.  The tool starts ITSELF once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, the
   program behind `--`); that child runs, on 32 frames in batches of 8 and in one process,
       the mount without options: plain, with a dark frame, with a flat field, with both
                                        k_unpack_x16<14> | k_cal_unpack_x16<14, DARK, FLAT> for (true, false), (false, true), (true, true)
       mlvfs_amd_unpack_dev + mlvfs_amd_flat_apply_dev without and with a dark frame
                                        k_unpack_x16<14>, k_cal_apply_x16<false | true, true> (the two passes the fused one replaces)
       mlvfs_amd_flat_from_clip         k_unpack_x16<14>, k_dark_accum_x16, k_dark_mean, k_flat_chan_sums, k_flat_gain
   and the parent prints every kernel's time per frame side by side, with the spread of its launches, and the keep rule's verdict.
2. The mount's frames per second with and without a flat field for cs5x5 + bad pixels + stripes, in alternating repetitions.
3. Plain -> plain at 12 bits (the route that pays one pass more than k_mlv_repack) with and without a flat field, alternating."""
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
from mlvfs_amd.flat import Flat
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions

W, H = 3584, 1320
# (what a kernel's name in the profile starts with, launches that are one plane and not one batch)
KERNELS = [("k_unpack_x16<14>", False), ("k_cal_unpack_x16<14, true, false>", False), ("k_cal_unpack_x16<14, false, true>", False), ("k_cal_unpack_x16<14, true, true>", False),
           ("k_cal_apply_x16<false, true>", False), ("k_cal_apply_x16<true, true>", False), ("k_flat_chan_sums", True), ("k_flat_gain", True)]


def dark_plane():
    """tools/dark_bench.py's: the pedestal, a column pattern and a little noise"""
    rng = np.random.default_rng(3)
    return (synth.BLACK + rng.integers(-5, 6, (H, W)) + (np.arange(W) % 8 == 3) * 9).astype(np.uint16)


def flat_plane():
    """an evenly lit target through vignetting (corners at 0.6), a column pattern, a tint per channel and a little noise; no dust: deep
    shadows would become bad pixels of the corrected clip, and the mount's two arms would differ in the size of the repair map"""
    rng = np.random.default_rng(4)
    yy, xx = np.indices((H, W))
    r2 = ((xx - (W - 1) / 2) / W) ** 2 + ((yy - (H - 1) / 2) / H) ** 2
    sig = 6000 * (1 - 0.8 * r2) * (1 + 0.03 * (xx % 8 == 3)) * np.array([1.0, 0.8, 0.8, 0.6])[(yy & 1) * 2 + (xx & 1)]
    return (synth.BLACK + sig + rng.integers(-6, 7, (H, W))).astype(np.uint16)


def write_clip(root, frames):
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    path = os.path.join(root, "B.MLV")
    mlvfile.write_clip(path, [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return path


def child(a) -> int:
    """what the profiler watches"""
    import torch
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    path = os.path.join(a.dir, "B.MLV")
    n = a.batch
    with mlvfile.MlvReader(path) as r, Dark.from_plane(dark_plane(), 14, synth.BLACK) as dark, Flat.from_plane(flat_plane(), 14, synth.BLACK) as flat:
        arms = [(None, None), (dark, None), (None, flat), (dark, flat)]
        for d, f in arms + arms:                                             # the second round is the warm one; all launches are listed
            with Mount(r, MlvfsOptions(), basename="/B.MLV", dark=d, flat=f) as m:
                m.dng(0, a.frames, batch=n)
        packed = r.read_frames(0, n, W * H * 14 // 8 + 16)
        dp = torch.from_numpy(packed).cuda()
        frames = torch.zeros((n, H, W), dtype=torch.int16, device="cuda")
        geom = lib.Geom(W, H, 14, synth.BLACK, synth.WHITE, 0, 0)
        for d in (None, dark):
            for _ in range(a.frames // n):
                lib.check(L.mlvfs_amd_unpack_dev(C.byref(geom), C.c_void_p(dp.data_ptr()), packed.shape[1], C.c_void_p(frames.data_ptr()), W * H * 2, n, None))
                lib.check(L.mlvfs_amd_flat_apply_dev(flat.h, d.h if d else None, C.byref(geom), C.c_void_p(frames.data_ptr()), W * H * 2, n, None))
        torch.cuda.synchronize()
        for _ in range(4):
            Flat.from_clip(r, 0, a.frames, batch=n).close()
    return 0


def kernel_report(a) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    out = os.path.join(a.dir, "prof")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "flat", "--",
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
    print(f"kernel times, {a.frames} frames in batches of {a.batch} (one launch = one batch; us per frame = launch / {a.batch}; the gain kernels: one plane):")
    found = {}
    for want, one_plane in KERNELS:
        for row in rows:
            if row["Name"].replace("mlv::", "").replace("void ", "").startswith(want + "("):
                per = 1 if one_plane else a.batch
                found[want] = [float(row[k]) / 1e3 / per for k in ("AverageNs", "MinNs", "MaxNs")] + [int(row["Calls"])]
                avg, lo, hi, calls = found[want]
                print(f"  {want:30s} {calls:3d} launches   avg {avg:7.2f}   min {lo:7.2f}   max {hi:7.2f}   spread {hi - lo:6.2f}")
    if all(k in found for k, _ in KERNELS[:6]):
        u = found["k_unpack_x16<14>"]
        for fused, apply in (("k_cal_unpack_x16<14, false, true>", "k_cal_apply_x16<false, true>"), ("k_cal_unpack_x16<14, true, true>", "k_cal_apply_x16<true, true>")):
            f, s = found[fused], found[apply]
            saved = u[0] + s[0] - f[0]
            print(f"  {fused} {f[0]:.2f} against k_unpack_x16<14> + {apply} {u[0] + s[0]:.2f} us per frame: {saved:.2f} saved;"
                  f" the spread of k_unpack_x16<14>'s launches is {u[2] - u[1]:.2f}: {'keep' if saved > u[2] - u[1] else 'DROP'} the fused pass")
    else:
        print("  kernels missing from the profile:", [k for k, _ in KERNELS if k not in found], sorted({r["Name"][:60] for r in rows})[:40])
    return True


def alternate(reps, arms, run):
    """arms: {label: argument}; run(argument) -> seconds; the first repetition warms page cache, code objects and staging"""
    took = {k: [] for k in arms}
    for rep in range(reps + 1):
        for k, v in arms.items():
            dt = run(v)
            if rep:
                took[k].append(dt)
    return took


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
    root = tempfile.mkdtemp(prefix="flatbench_", dir=a.dir)
    a.dir = root
    try:
        path = write_clip(root, a.frames)
        if not a.skip_kernels and not kernel_report(a):                     # before this process opens the GPU itself
            return 1
        L = lib.load()
        assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
        opt = MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)
        with mlvfile.MlvReader(path) as r, Flat.from_plane(flat_plane(), 14, synth.BLACK) as flat:
            def serve(f):
                L.free_focus_pixel_maps()
                with Mount(r, opt, basename="/B.MLV", flat=f) as m:
                    t0 = time.perf_counter()
                    m.dng(0, a.frames, batch=a.batch)
                    return time.perf_counter() - t0

            for k, v in alternate(a.reps, {"without": None, "with a": flat}, serve).items():
                fps = [a.frames / t for t in v]
                print(f"mount, cs5x5 + bad pixels + stripes, {k} flat field: {np.median(fps):.1f} frames/s"
                      f" (median of {len(fps)} alternating repetitions: {', '.join(f'{x:.1f}' for x in fps)}), file reads and downloads included")

            count = [0]

            def rewrite(f):
                count[0] += 1
                out = os.path.join(root, f"out{count[0]}")
                os.mkdir(out)
                t0 = time.perf_counter()
                r.transcode(os.path.join(out, "B.MLV"), lj92=False, batch=a.batch, bits=12, flat=f)
                dt = time.perf_counter() - t0
                shutil.rmtree(out)
                return dt

            for k, v in alternate(a.reps, {"without": None, "with a": flat}, rewrite).items():
                fps = [a.frames / t for t in v]
                print(f"plain -> plain at 12 bits, {k} flat field: {np.median(fps):.1f} frames/s"
                      f" (median of {len(fps)} alternating repetitions: {', '.join(f'{x:.1f}' for x in fps)}), file reads and writes included")
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

"""A look on the rendered routes at 3584x1320 (csrc/k_tone_dev.h, csrc/mount.cpp): the numbers of DESIGN.md 3.16.

    python tools/look_bench.py [--frames 32] [--batch 8] [--reps 3] [--dir DIR] [--skip-kernels]

1. Kernel times.  The tool starts ITSELF once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, the
   program behind `--`, under a time limit); that child serves the clip through the mount with cs5x5 + bad pixels + stripes as half-size,
   full-size and 1280x472 TIFF files without a look, with a 33^3 look and with a 65^3 look, and the parent prints us per frame of each
   look kernel beside its plain twin of the same run, and the ratio of the two (the yardstick is the twin, never the look kernel
   itself).  The launches of a look kernel at the two table sizes are told apart by their place in the child's order.
2. The mount's frames per second, file reads and downloads included, for the three TIFF routes with and without the 33^3 look, in
   alternating repetitions within one run (the yardstick: a route with a look within the repetitions' scatter of the same route
   without).
Every step that uses the GPU runs under a time limit of its own, and the tool ends at the first that fails."""
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
SIZE = (1280, 472)
ROUTES = [("half-size TIFF", dict()), ("full-size TIFF", dict(full=True)), ("1280x472 TIFF", dict(size=SIZE))]
TWINS = [("k_render2_x16", "k_render2_look_x16"), ("k_render1_x16", "k_render1_look_x16"), ("k_scale_x16", "k_scale_look_x16")]
TABLES = (33, 65)


def options():
    return MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)


def write_clip(root, frames):
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    path = os.path.join(root, "B.MLV")
    mlvfile.write_clip(path, [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return path


def make_look(n):
    """a table of n a side that is no identity -- a contrast curve with a colour twist -- behind the linear shaper"""
    T = look.identity(n).astype(np.float64) / 65535.0
    T = np.clip(0.5 + 1.25 * (T - 0.5) + 0.06 * (T[:, [1, 2, 0]] - T[:, [2, 0, 1]]), 0.0, 1.0)
    return look.Look(look.shaper_linear(), n, np.floor(T * 65535.0 + 0.5).astype(np.uint16))


def serve(L, r, a, args, lk):
    """one fresh handle serves the clip -> seconds"""
    L.free_focus_pixel_maps()
    with Mount(r, options(), basename="/B.MLV") as m:
        if lk is not None:
            m.set_look(lk)
        t0 = time.perf_counter()
        m.rgb(0, a.frames, batch=a.batch, **args)
        return time.perf_counter() - t0


def child(a) -> int:
    """what the profiler watches: per round, every route plain, then with the 33^3, then with the 65^3 table"""
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r, make_look(TABLES[0]) as l33, make_look(TABLES[1]) as l65:
        for _ in range(2):                                                   # the second round is the warm one; all launches are listed
            for lk in (None, l33, l65):
                for _, args in ROUTES:
                    serve(L, r, a, args, lk)
    return 0


def short(name):
    return name.replace("mlv::", "").replace("void ", "")


def kernel_report(a) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    out = os.path.join(a.dir, "prof")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "look", "--",
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
    trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
    if not trace:
        print("no kernel_trace.csv under", out, [os.path.relpath(f, out) for f in glob.glob(os.path.join(out, "**", "*"), recursive=True)][:20])
        return True
    rows = sorted(csv.DictReader(open(trace[0])), key=lambda r: int(r["Start_Timestamp"]))

    def launches(kernel):
        return [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 / a.batch for r in rows if short(r.get("Kernel_Name", "")).startswith(kernel + "(")]

    per = -(-a.frames // a.batch)                                            # launches of one route in one serve
    print(f"kernel times, {a.frames} frames of {W}x{H} in batches of {a.batch} (one launch = one batch; us per frame = launch / {a.batch}):")
    for plain, with_look in TWINS:
        us, lus = launches(plain), launches(with_look)
        if len(us) != 2 * per or len(lus) != 2 * len(TABLES) * per:
            print(f"  the trace lists {len(us)} launches of {plain} and {len(lus)} of {with_look}, not {2 * per} and {2 * len(TABLES) * per}")
            continue
        base = float(np.mean(us))
        print(f"  {plain:22s} {len(us):3d} launches   avg {base:7.2f}   min {min(us):7.2f}   max {max(us):7.2f} us per frame")
        for k, n in enumerate(TABLES):                                       # per round: the launches at 33, then those at 65
            part = [v for i, v in enumerate(lus) if i % (len(TABLES) * per) // per == k]
            avg = float(np.mean(part))
            print(f"  {with_look:22s} {len(part):3d} launches   avg {avg:7.2f}   min {min(part):7.2f}   max {max(part):7.2f} us per frame"
                  f" at N = {n} ({look.SHAPER_BYTES + 8 * n ** 3} bytes of image): {avg / base:.2f} x its plain twin")
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
    ap.add_argument("--routes", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.routes:
        return routes(a)
    root = tempfile.mkdtemp(prefix="lookbench_", dir=a.dir)
    a.dir = root
    try:
        write_clip(root, a.frames)
        if not a.skip_kernels and not kernel_report(a):
            return 1
        # the routes: a process of its own under a time limit of its own, as the profiled run has one
        cmd = ["timeout", "-k", "10", str(a.child_limit), sys.executable, os.path.abspath(__file__), "--routes", "--dir", root, "--frames", str(a.frames),
               "--batch", str(a.batch), "--reps", str(a.reps)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"the run of the routes ended with status {rc}")
            return 1
    finally:
        shutil.rmtree(root, ignore_errors=True)
    return 0


def routes(a) -> int:
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    took = {(label, with_look): [] for label, _ in ROUTES for with_look in (False, True)}
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r, make_look(TABLES[0]) as lk:
        for rep in range(a.reps + 1):                                        # the first repetition warms page cache, code objects and staging
            for label, args in ROUTES:
                for with_look in (False, True):
                    dt = serve(L, r, a, args, lk if with_look else None)
                    if rep:
                        took[(label, with_look)].append(dt)
    print(f"mount, cs5x5 + bad pixels + stripes, {a.frames} frames of {W}x{H} in batches of {a.batch}, file reads and downloads included:")
    for label, _ in ROUTES:
        fps = {k: [a.frames / t for t in took[(label, k)]] for k in (False, True)}
        med = {k: float(np.median(v)) for k, v in fps.items()}
        for k in (False, True):
            print(f"  {label:16s} {'with a 33^3 look' if k else 'plain           '} {med[k]:7.1f} frames/s (median of {len(fps[k])} alternating repetitions:"
                  f" {', '.join(f'{x:.1f}' for x in fps[k])}; scatter {max(fps[k]) - min(fps[k]):.1f})")
        scatter = max(max(v) - min(v) for v in fps.values())
        print(f"  {label:16s} look / plain = {med[True] / med[False]:.3f}; the medians differ by {abs(med[True] - med[False]):.1f} frames/s, the repetitions scatter by {scatter:.1f}")
    print("  (one machine, one run: the differences are those of one box)")
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

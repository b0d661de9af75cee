"""The 16-bit TIFF routes at 3584x1320 (csrc/k_tone_dev.h, csrc/mount.cpp): the numbers of DESIGN.md 3.17.

    python tools/deep_bench.py [--frames 32] [--batch 8] [--reps 3] [--dir DIR] [--skip-kernels]

1. Kernel times.  The tool starts ITSELF once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, the
   program behind `--`, under a time limit); that child serves the clip through the mount with cs5x5 + bad pixels + stripes as half-size,
   full-size and 1280x472 TIFF files at 8 bits plain, at 8 bits with a 33^3 look, at 16 bits with N = 0 and at 16 bits with N = 33, and
   the parent prints us per frame of each deep kernel beside its plain and its look twin of the same run (the yardstick: the look
   kernel's time plus the extra store traffic).  The launches of a deep kernel at the two N are told apart by their place in the
   child's order.
2. The mount's frames per second, file reads and downloads included, for the three 16-bit TIFF routes beside their 8-bit twins -- N = 0
   beside the plain route, N = 33 beside the route with the 33^3 look -- in alternating repetitions within one run (the yardstick: the
   8-bit routes are bound by the link, so a 16-bit route should fall towards the ratio of bytes per file, about 0.5).
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
TWINS = [("k_render2_x16", "k_render2_look_x16", "k_render2_deep_x16"), ("k_render1_x16", "k_render1_look_x16", "k_render1_deep_x16"),
         ("k_scale_x16", "k_scale_look_x16", "k_scale_deep_x16")]
TABLES = (0, 33)                         # of the deep look
PIXELS = {"half-size TIFF": (W // 2) * (H // 2), "full-size TIFF": W * H, "1280x472 TIFF": SIZE[0] * SIZE[1]}


def options():
    return MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)


def write_clip(root, frames):
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    path = os.path.join(root, "B.MLV")
    mlvfile.write_clip(path, [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return path


def table(n):
    """a table of n a side that is no identity -- a contrast curve with a colour twist (tools/look_bench.py's)"""
    T = look.identity(n).astype(np.float64) / 65535.0
    T = np.clip(0.5 + 1.25 * (T - 0.5) + 0.06 * (T[:, [1, 2, 0]] - T[:, [2, 0, 1]]), 0.0, 1.0)
    return np.floor(T * 65535.0 + 0.5).astype(np.uint16)


def make_look(n):
    """the 8-bit twin: that table behind the linear shaper"""
    return look.Look(look.shaper_linear(), n, table(n))


def make_deep(n):
    """a 12-stop log curve, and behind it that table where n is not 0"""
    return look.Look16(look.shaper16_log2(12), n, table(n) if n else None)


def serve(L, r, a, args, lk=None, deep=None):
    """one fresh handle serves the clip -> seconds"""
    L.free_focus_pixel_maps()
    with Mount(r, options(), basename="/B.MLV") as m:
        if lk is not None:
            m.set_look(lk)
        t0 = time.perf_counter()
        m.rgb(0, a.frames, batch=a.batch, look16=deep, **args)
        return time.perf_counter() - t0


def child(a) -> int:
    """what the profiler watches: per round, every route at 8 bits plain, at 8 bits with the 33^3 look, at 16 bits with N = 0, at 16
    bits with N = 33"""
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r, make_look(33) as l33, make_deep(TABLES[0]) as d0, make_deep(TABLES[1]) as d33:
        for _ in range(2):                                                   # the second round is the warm one; all launches are listed
            for lk, deep in ((None, None), (l33, None), (None, d0), (None, d33)):
                for _, args in ROUTES:
                    serve(L, r, a, args, lk, deep)
    return 0


def short(name):
    return name.replace("mlv::", "").replace("void ", "")


def kernel_report(a) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    out = os.path.join(a.dir, "prof")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "deep", "--",
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
    for (plain, with_look, deep), (label, _) in zip(TWINS, ROUTES):
        us, lus, dus = launches(plain), launches(with_look), launches(deep)
        if len(us) != 2 * per or len(lus) != 2 * per or len(dus) != 2 * len(TABLES) * per:
            print(f"  the trace lists {len(us)} launches of {plain}, {len(lus)} of {with_look} and {len(dus)} of {deep}, not {2 * per}, {2 * per} and {2 * len(TABLES) * per}")
            continue
        base, lbase = float(np.mean(us)), float(np.mean(lus))
        for name, v in ((plain, us), (with_look, lus)):
            print(f"  {name:22s} {len(v):3d} launches   avg {float(np.mean(v)):7.2f}   min {min(v):7.2f}   max {max(v):7.2f} us per frame")
        for k, n in enumerate(TABLES):                                       # per round: the launches at N = 0, then those at N = 33
            part = [v for i, v in enumerate(dus) if i % (len(TABLES) * per) // per == k]
            avg = float(np.mean(part))
            print(f"  {deep:22s} {len(part):3d} launches   avg {avg:7.2f}   min {min(part):7.2f}   max {max(part):7.2f} us per frame"
                  f" at N = {n}: {avg / base:.2f} x its plain twin, {avg / lbase:.2f} x its look twin; it stores {3 * PIXELS[label] / 1e6:.2f} MB more than either")
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
    root = tempfile.mkdtemp(prefix="deepbench_", dir=a.dir)
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
    kinds = ("8 bits, plain", "16 bits, N = 0", "8 bits, 33^3 look", "16 bits, N = 33")
    took = {(label, kind): [] for label, _ in ROUTES for kind in kinds}
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r, make_look(33) as l33, make_deep(0) as d0, make_deep(33) as d33:
        how = dict(zip(kinds, ((None, None), (None, d0), (l33, None), (None, d33))))
        for rep in range(a.reps + 1):                                        # the first repetition warms page cache, code objects and staging
            for label, args in ROUTES:
                for kind in kinds:
                    dt = serve(L, r, a, args, *how[kind])
                    if rep:
                        took[(label, kind)].append(dt)
    print(f"mount, cs5x5 + bad pixels + stripes, {a.frames} frames of {W}x{H} in batches of {a.batch}, file reads and downloads included:")
    for label, _ in ROUTES:
        fps = {k: [a.frames / t for t in took[(label, k)]] for k in kinds}
        med = {k: float(np.median(v)) for k, v in fps.items()}
        for k in kinds:
            size = 256 + (6 if k.startswith("16") else 3) * PIXELS[label]
            print(f"  {label:16s} {k:18s} {med[k]:7.1f} frames/s, {size / 1e6:6.2f} MB per file (median of {len(fps[k])} alternating repetitions:"
                  f" {', '.join(f'{x:.1f}' for x in fps[k])}; scatter {max(fps[k]) - min(fps[k]):.1f})")
        bytes_ratio = (256 + 3 * PIXELS[label]) / (256 + 6 * PIXELS[label])
        for k8, k16 in ((kinds[0], kinds[1]), (kinds[2], kinds[3])):
            print(f"  {label:16s} {k16} / {k8} = {med[k16] / med[k8]:.3f}; the bytes per file say {bytes_ratio:.3f}")
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

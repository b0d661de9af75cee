"""A clip's frames as device-resident tensors at 3584x1320 (csrc/k_tensor.hip, csrc/mount.cpp): the numbers of DESIGN.md 3.24.

    python tools/tensor_bench.py [--frames 32] [--batch 8] [--reps 3] [--dir DIR] [--skip-kernels] [--skip-floor]

Conditions: 14 bits, cs5x5 + bad pixels + stripes, frames in batches, alternating repetitions within one run, the median of them.
1. The linear-copy floor: tools/stream_floor (built from tools/stream_floor.hip if it is not there) in this run; its best read + write
   rate is what the same bytes take when nothing is computed.
2. Kernel times.  The tool starts ITSELF once more under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, the program
   behind `--`, under a time limit); that child serves the four tensor cases, and the parent prints each tensor kernel per frame beside
   the rendering pass in front of it (k_render2_x16, k_render1_x16, k_render1_deep_x16), with the bytes each moves, the TB/s that makes
   and the tensor kernel's time over the floor of its bytes.  Stated beforehand: each _x8 kernel stays within 1.5 x that floor.
3. Frames per second of the four tensor cases, each beside the TIFF or .dng route of the same frames.  Stated beforehand: a tensor route
   serves no fewer frames per second than its file route, beyond the repetitions' scatter, because it moves no file over the link.
The tensors are written into one buffer per case that is allocated before the clock starts, as a consumer that reuses its batch would."""
import argparse
import csv
import glob
import os
import re
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

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 3584, 1320
FULL, HALF = W * H, (W // 2) * (H // 2)
# label, Mount.tensor's arguments, the file route of the same frames, the tensor kernel, bytes it reads + writes per frame, the pass in
# front of it and that pass's bytes (None: the fused pass, which this tool does not report)
CASES = [("half size, F16 NCHW", dict(dtype="float16"), ("rgb", dict()), "k_tensor_rgb_x8<8, 1, 0>", HALF * 9, "k_render2_x16", FULL * 2 + HALF * 3),
         ("full size, F16 NCHW", dict(dtype="float16", full=True), ("rgb", dict(full=True)), "k_tensor_rgb_x8<8, 1, 0>", FULL * 9, "k_render1_x16", FULL * 5),
         ("full size, 16 bits to F32 NCHW", dict(dtype="float32", full=True, deep=True), ("rgb", dict(full=True, deep=True)), "k_tensor_rgb_x8<16, 0, 0>",
          FULL * 18, "k_render1_deep_x16", FULL * 8),
         ("Bayer, F16 NCHW", dict(kind="bayer", dtype="float16"), ("dng", dict()), "k_tensor_bayer_x8<1, 0>", FULL * 4, None, 0)]
BOUND = 1.5


def options():
    return MlvfsOptions(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)


def write_clip(root, frames):
    base = [synth.normal_frame(W, H, seed=9, frame=k) for k in range(min(8, frames))]
    packed = [np.ascontiguousarray(synth.pack_bits(f), "<u2").tobytes() for f in base]
    path = os.path.join(root, "B.MLV")
    mlvfile.write_clip(path, [packed[k % len(packed)] for k in range(frames)], W, H, chunks=2)
    return path


def serve_tensor(L, r, a, args, deep, out=None):
    """one fresh handle leaves the clip's tensors in `out` -> (seconds, the tensor)"""
    args = dict(args)
    lk = deep if args.pop("deep", False) else None
    L.free_focus_pixel_maps()
    with Mount(r, options(), basename="/B.MLV") as m:
        t0 = time.perf_counter()
        out = m.tensor(0, a.frames, batch=a.batch, out=out, look16=lk, **args)
        return time.perf_counter() - t0, out


def serve_file(L, r, a, kind, args, deep):
    """one fresh handle serves the same frames as files -> (seconds, bytes per file)"""
    args = dict(args)
    lk = deep if args.pop("deep", False) else None
    L.free_focus_pixel_maps()
    with Mount(r, options(), basename="/B.MLV") as m:
        t0 = time.perf_counter()
        files = m.rgb(0, a.frames, batch=a.batch, look16=lk, **args) if kind == "rgb" else m.dng(0, a.frames, batch=a.batch)
        return time.perf_counter() - t0, files.shape[1]


def linear_deep():
    return look.Look16(look.shaper16_linear(), 0, None)


def child(a) -> int:
    """what the profiler watches: two rounds of the four tensor cases, in CASES' order; the second round is the warm one"""
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r, linear_deep() as deep:
        for _ in range(2):
            for _, args, _, _, _, _, _ in CASES:
                serve_tensor(L, r, a, args, deep)
    return 0


def short(name):
    return name.replace("mlv::", "").replace("(anonymous namespace)::", "").replace("void ", "")


def copy_floor(a):
    """TB/s of a linear read + write copy on this machine, now; None: not measured"""
    exe = os.path.join(HERE, "stream_floor")
    if not os.path.exists(exe):
        b = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", os.path.join(HERE, "stream_floor.hip"), "-o", exe], capture_output=True, text=True)
        if b.returncode != 0:
            print("tools/stream_floor does not build:", b.stderr[-1000:])
            return None
    p = subprocess.run(["timeout", "-k", "10", "120", exe, "100"], capture_output=True, text=True)
    if p.returncode != 0:
        print(f"tools/stream_floor ended with status {p.returncode}; nothing more is run on the GPU:", p.stdout[-1000:], p.stderr[-1000:])
        return False
    rates = [float(m.group(1)) for m in re.finditer(r"mode 0 \(read\+write\).*?([0-9.]+) TB/s", p.stdout)]
    if not rates:
        print("tools/stream_floor printed no read + write rate:", p.stdout[-500:])
        return None
    print(f"linear copy, read + write, nothing computed (tools/stream_floor, 100 frames): {max(rates):.2f} TB/s (its three forms: {', '.join(f'{x:.2f}' for x in rates)})")
    return max(rates)


def kernel_report(a, floor) -> bool:
    """False: the profiled child did not end well.  The caller then ends without opening the GPU: nothing is started on a card
    after a program has failed on it."""
    out = os.path.join(a.dir, "prof")
    # under timeout(1), a process group of its own: at the limit the profiler AND the program behind `--` are ended, not the profiler alone
    cmd = ["timeout", "-k", "10", str(a.child_limit), "rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", out, "-o", "tensor", "--",
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

    per = -(-a.frames // a.batch)                                            # launches of one kernel in one serve
    print(f"kernel times, {a.frames} frames of {W}x{H} in batches of {a.batch} (one launch = one batch; us per frame = launch / {a.batch}):")

    def line(name, v, moved):
        avg = float(np.mean(v))
        print(f"  {name:28s} {len(v):3d} launches   avg {avg:7.2f}   min {min(v):7.2f}   max {max(v):7.2f} us per frame, {moved / 1e6:6.2f} MB per frame:"
              f" {moved / 1e6 / avg:.2f} TB/s")                                # MB per us = TB/s
        return avg

    for label, _, _, kernel, moved, before, moved_before in CASES:
        sharing = [c for c in CASES if c[3] == kernel]                       # one instantiation may serve two sizes: told apart by their order
        v = launches(kernel)
        if len(v) != 2 * per * len(sharing):
            print(f"  {label}: the trace lists {len(v)} launches of {kernel}, not {2 * per * len(sharing)}:", sorted({short(r.get('Kernel_Name', ''))[:50] for r in rows})[:60])
            continue
        at = [c[0] for c in sharing].index(label)
        v = [x for i, x in enumerate(v) if (i // per) % len(sharing) == at]
        print(f" {label}:")
        if before:
            vb = launches(before)
            if vb:
                line(before, vb, moved_before)
        avg = line(kernel, v, moved)
        if floor:
            least = moved / 1e6 / floor
            print(f"  {'':28s} the same bytes as a linear copy at {floor:.2f} TB/s: {least:.2f} us; the kernel takes {avg / least:.2f} x that"
                  f" ({'within' if avg <= BOUND * least else 'MISSES'} the {BOUND} x stated beforehand)")
    return True


def routes(a) -> int:
    import torch
    L = lib.load()
    assert L.mlvfs_amd_init(0) == 0, L.mlvfs_amd_last_error()
    took = {label: ([], []) for label, *_ in CASES}
    size, outs = {}, {}
    with mlvfile.MlvReader(os.path.join(a.dir, "B.MLV")) as r, linear_deep() as deep:
        for rep in range(a.reps + 1):                                    # the first repetition warms page cache, code objects and staging
            for label, args, (kind, fargs), *_ in CASES:
                dt, outs[label] = serve_tensor(L, r, a, args, deep, outs.get(label))
                df, size[label] = serve_file(L, r, a, kind, fargs, deep)
                if rep:
                    took[label][0].append(dt)
                    took[label][1].append(df)
    torch.cuda.synchronize()
    print(f"mount, cs5x5 + bad pixels + stripes, {a.frames} frames of {W}x{H} in batches of {a.batch}, file reads included; the file routes download, the tensor routes do not:")
    for label, (vt, vf) in took.items():
        ft, ff = [a.frames / t for t in vt], [a.frames / t for t in vf]
        t = outs[label]
        scatter = max(max(ft) - min(ft), max(ff) - min(ff))
        verdict = "no fewer" if np.median(ft) >= np.median(ff) - scatter else "FEWER"
        print(f"  {label:32s} tensor {np.median(ft):7.1f} frames/s ({', '.join(f'{x:.1f}' for x in ft)}), {t[0].numel() * t.element_size():9d} bytes per frame left on the GPU")
        print(f"  {'':32s} file   {np.median(ff):7.1f} frames/s ({', '.join(f'{x:.1f}' for x in ff)}), {size[label]:9.0f} bytes per file over the link"
              f" -- the tensor route serves {verdict} (scatter {scatter:.1f})")
    print("  (medians of alternating repetitions in one run on one machine)")
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the clip and the profile go (default: a temporary directory)")
    ap.add_argument("--skip-kernels", action="store_true", help="no profiled child run")
    ap.add_argument("--skip-floor", action="store_true", help="no run of tools/stream_floor")
    ap.add_argument("--child-limit", type=int, default=300, help="seconds the profiled child run and the run of the routes may each take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--routes", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.routes:
        return routes(a)
    root = tempfile.mkdtemp(prefix="tensorbench_", dir=a.dir)
    a.dir = root
    try:
        write_clip(root, a.frames)
        floor = None if a.skip_floor else copy_floor(a)
        if floor is False:
            return 1
        if not a.skip_kernels and not kernel_report(a, floor):
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


if __name__ == "__main__":
    # on a thread of its own: the library's per-thread stream is then given back when the thread ends, not while the process
    # exits -- under rocprofv3 the profiler's own state is gone by then and the run ends in an abort instead of a stats file
    import threading
    rc = [1]
    t = threading.Thread(target=lambda: rc.__setitem__(0, main()))
    t.start()
    t.join()
    sys.exit(rc[0])

#!/usr/bin/env python3
"""tools/p5_loop_counts.py [extra hipcc flags] -- k_frame_p5<false,1> from the compiler's own assembly, no GPU needed: the resource
lines (registers, spills, scratch, LDS, occupancy) and static instruction counts of the whole kernel and of its largest loops (a loop =
a backward branch and everything between it and its target; the task loop comes first, the main loop of pair steps second).  Compiles
mlvfs_amd/csrc/k_frame_p.hip with the production flags into a temporary directory.  DESIGN.md §3.1's table of the step loop is made
with it."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlvfs_amd", "csrc")
KERNEL = "_ZN3mlv10k_frame_p5ILb0ELi1EEEvNS_9FrameArgsEiiiii"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-Wno-unused-function", "-I" + os.path.join(ROOT, "include"),
         "-mllvm", "--amdgpu-sched-strategy=max-ilp", "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "--save-temps=obj"]


def stats(ins):
    c = collections.Counter(m for m, _ in ins)
    some = lambda p: sum(v for k, v in c.items() if k.startswith(p))
    return dict(all=len(ins), valu=some("v_"), v_mov=c["v_mov_b32_e32"] + c["v_mov_b32_e64"], dpp=c["v_mov_b32_dpp"], pk_minmax=some("v_pk_m"),
                waits=c["s_waitcnt"], lds=some("ds_"), stores=some("buffer_store"), loads=some("buffer_load"),
                lane_moves=c["v_readlane_b32"] + c["v_writelane_b32"])


def main():
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + sys.argv[1:] + ["-c", os.path.join(CSRC, "k_frame_p.hip"), "-o", os.path.join(d, "kfp.o")],
                           cwd=CSRC, stderr=subprocess.PIPE, text=True)
        if r.returncode:
            sys.exit(r.stderr)
        keep = False
        for ln in r.stderr.splitlines():
            if "Function Name:" in ln:
                keep = KERNEL in ln
            m = re.search(r"remark: [^ ]+ +(.*) \[-Rpass", ln)
            if keep and m and "Function Name" not in m.group(1):
                print(m.group(1).strip())
        txt = open(os.path.join(d, "k_frame_p-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    a = txt.index("\n" + KERNEL + ":")
    ins, labels = [], {}
    for ln in txt[a:txt.index("s_endpgm", a)].splitlines():
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        m = re.match(r"^\t([a-z][a-z0-9_]+)\b(.*)", ln)
        if m:
            ins.append((m.group(1), m.group(2)))
    print("kernel", stats(ins))
    loops = {}
    for i, (mn, ops) in enumerate(ins):
        if mn.startswith("s_cbranch") or mn == "s_branch":
            t = ops.split()[0]
            if labels.get(t, i + 1) <= i:
                loops[t] = max(loops.get(t, 0), i + 1)
    for t, hi in sorted(loops.items(), key=lambda x: labels[x[0]] - x[1])[:4]:
        print("loop at", t, stats(ins[labels[t]:hi]))


if __name__ == "__main__":
    main()

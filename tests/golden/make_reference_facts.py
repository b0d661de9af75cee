#!/usr/bin/env python3
"""tests/golden/reference_facts.json FROM THE REFERENCE (run in the build container only): facts about the reference tree that
three CPU tests check the repository against, recorded as data so that the tests run without the tree.

    abi_layout              tests/abi_probe.c compiled with -DUSE_REFERENCE against the reference's own mlvfs.h: size and field
                            offsets of `struct frame_headers` (tests/test_abi.py)
    called_from_callers     every global function of the objects the library replaces (mlvfs/Makefile:24,34-38) that the rest of
                            MLVFS calls -- main.c, gif.c, webgui.c, resource_manager.c, ... (tests/test_cabi.py)
    process_frame_calls     the calls of process_frame (main.c) that bracket and make up the pixel path, in the order of their
                            first appearance in its text (tests/test_cabi.py)
    gif_c_calls             which chunk loader gif.c calls (tests/test_cabi.py)
    fpm_sha256              per mlvfs/data/*.fpm: SHA-256 of its coordinates as little-endian int64 (n, 2), file order
                            (tests/test_focus_maps.py)

    python tests/golden/make_reference_facts.py
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/mlvfs"
REPLACED = ["dng.c", "cs.c", "stripes.c", "hdr.c", "amaze_demosaic_RT.c", "histogram.c", "patternnoise.c"]
PIXEL_PATH = ["mlvfs_load_chunks(", "get_image_data(", "fix_pattern_noise(", "cr2hdr20_convert_data(", "fix_bad_pixels(",
              "chroma_smooth(", "stripes_apply_correction(", "mlvfs_close_chunks("]


def abi_layout(tmp):
    exe = os.path.join(tmp, "abi_probe")
    subprocess.run(["gcc", "-std=gnu99", "-DUSE_REFERENCE", "-I", REF, os.path.join(ROOT, "tests", "abi_probe.c"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}


def called_from_callers(tmp):
    defined = set()
    for src in REPLACED:
        obj = os.path.join(tmp, src + ".o")
        subprocess.run(["gcc", "-c", "-O0", "-w", "-std=gnu99", "-D_FILE_OFFSET_BITS=64", "-I", REF, os.path.join(REF, src), "-o", obj], check=True)
        out = subprocess.run(["nm", "--defined-only", obj], capture_output=True, text=True, check=True).stdout
        defined |= {l.split()[-1] for l in out.splitlines() if " T " in l}
    needed = set()
    for f in os.listdir(REF):
        if f.endswith(".c") and f not in REPLACED:
            text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(REF, f), errors="replace").read(), flags=re.S)
            needed |= {s for s in defined if re.search(r"\b" + re.escape(s) + r"\s*\(", text)}
    return sorted(needed)


def process_frame_calls():
    main_c = open(os.path.join(REF, "main.c"), errors="replace").read()
    body = main_c[main_c.index("static int process_frame("):main_c.index("int create_preview(")]
    return [c[:-1] for c in sorted(PIXEL_PATH, key=body.index)]


def gif_c_calls():
    gif_c = open(os.path.join(REF, "gif.c"), errors="replace").read()
    return {"mlvfs_load_chunks": "mlvfs_load_chunks" in gif_c, "mlvfs_close_chunks": "mlvfs_close_chunks" in gif_c,
            "load_chunks(path": "load_chunks(path" in gif_c}


def fpm_sha256():
    data = os.path.join(REF, "data")
    return {f[:-4]: hashlib.sha256(np.loadtxt(os.path.join(data, f), dtype="<i8").reshape(-1, 2).tobytes()).hexdigest()
            for f in sorted(os.listdir(data)) if f.endswith(".fpm")}


def main():
    with tempfile.TemporaryDirectory() as tmp:
        facts = {"generator": "tests/golden/make_reference_facts.py", "abi_layout": abi_layout(tmp),
                 "called_from_callers": called_from_callers(tmp), "process_frame_calls": process_frame_calls(),
                 "gif_c_calls": gif_c_calls(), "fpm_sha256": fpm_sha256()}
    with open(os.path.join(HERE, "reference_facts.json"), "w") as f:
        json.dump(facts, f, indent=1)
        f.write("\n")
    print("wrote", os.path.join(HERE, "reference_facts.json"))


if __name__ == "__main__":
    sys.exit(main())

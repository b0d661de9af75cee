"""Write a clip's tensors as .npy files, in order to look at them: every frame as the mount serves it with these options, left on the GPU
as a tensor (mlvfs_amd_mount_tensor; include/mlvfs_amd.h, "a clip's frames as device-resident tensors"; mlvfs_amd/tensor.py is the
definition) and copied to the host here, one file per frame.  A consumer on the GPU calls Mount.tensor() itself and copies nothing.

    python tools/mlv_tensor.py SRC.MLV OUTDIR [--kind rgb|bayer] [--dtype float16|float32|bfloat16|uint8|uint16] [--layout NCHW|NHWC]
                                             [--mean M[,M,M]] [--std S[,S,S]] [--gain G] [--full | --size WxH] [--resample] [--bits 16]
                                             [--cs N] [--bad-pix N] [--stripes] [--dual-iso N] [--hdr-interp N] [--first A] [--count N] [--batch N]

OUTDIR/<clip>_000000.npy ... hold arrays of shape (C, h, w) or (h, w, C).  bfloat16, which numpy does not have, is written as the
uint16 of its bits.  --bits 16 renders through a linear deep look: the 16-bit samples are linear light.  Nothing is overwritten."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlvfs_amd import look, mlvfile
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions


def wxh(text: str) -> tuple[int, int]:
    w, x, h = text.lower().partition("x")
    if not (x and w.isdigit() and h.isdigit() and int(w) >= 1 and int(h) >= 1):
        raise argparse.ArgumentTypeError(f"{text!r} is not WxH")
    return int(w), int(h)


def floats(text: str):
    try:
        v = [float(t) for t in text.split(",")]
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r} is not a number or a list of numbers")
    return v[0] if len(v) == 1 else v


def to_numpy(t):
    """a tensor on the GPU -> a numpy array on the host (bfloat16 as the uint16 of its bits)"""
    import torch
    t = t.cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("outdir")
    ap.add_argument("--kind", default="rgb", choices=("rgb", "bayer"))
    ap.add_argument("--dtype", default="float16", choices=("float16", "float32", "bfloat16", "uint8", "uint16"))
    ap.add_argument("--layout", default="NCHW", choices=("NCHW", "NHWC"))
    ap.add_argument("--mean", type=floats, default=None, help="subtracted per channel after the sample was scaled to 0 .. 1")
    ap.add_argument("--std", type=floats, default=None, help="divided by per channel")
    ap.add_argument("--gain", type=float, default=1.0, help="exposure factor of an rgb tensor, in steps of 1 / 256")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--full", action="store_true", help="the full-size rendering instead of the half-size one")
    how.add_argument("--size", type=wxh, metavar="WxH", help="the rendering at W x H")
    ap.add_argument("--resample", action="store_true", help="with --size: resampled from the full-size rendering, any size up to the frame's own")
    ap.add_argument("--bits", type=int, default=8, choices=(8, 16), help="16: the rendering at 16 bits, linear light")
    ap.add_argument("--cs", type=int, default=0, choices=(0, 2, 3, 5), help="chroma smoothing")
    ap.add_argument("--bad-pix", type=int, default=0, choices=(0, 1, 2), help="bad-pixel repair (2: aggressive)")
    ap.add_argument("--stripes", action="store_true", help="vertical stripes correction")
    ap.add_argument("--dual-iso", type=int, default=0, choices=(0, 1, 2), help="1 preview, 2 full conversion")
    ap.add_argument("--hdr-interp", type=int, default=0, choices=(0, 1), help="0 AMaZE + edge-directed, 1 mean23")
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--count", type=int, default=0, help="frames to write (default: to the end of the clip)")
    ap.add_argument("--batch", type=int, default=8, help="frames per GPU batch")
    a = ap.parse_args()
    if a.resample and (a.full or not a.size):
        ap.error("--resample takes --size, and no --full")
    if a.kind == "bayer" and (a.full or a.size or a.bits == 16):
        ap.error("--kind bayer takes none of --full, --size and --bits: the tensor is the frame itself")
    stem = os.path.splitext(os.path.basename(a.src))[0]
    opt = MlvfsOptions(chroma_smooth=a.cs, fix_bad_pixels=a.bad_pix, fix_stripes=int(a.stripes), dual_iso=a.dual_iso, hdr_interpolation_method=a.hdr_interp)
    with mlvfile.MlvReader(a.src) as r:
        count = a.count or r.frame_count - a.first
        if a.first < 0 or count <= 0 or a.first + count > r.frame_count:
            ap.error(f"frames {a.first} .. {a.first + count - 1} outside the clip ({r.frame_count} frames)")
        names = [os.path.join(a.outdir, f"{stem}_{k:06d}.npy") for k in range(a.first, a.first + count)]
        taken = [n for n in names if os.path.exists(n)]
        if taken:
            print(f"{taken[0]} exists ({len(taken)} of {count} files): nothing is overwritten", file=sys.stderr)
            return 1
        os.makedirs(a.outdir, exist_ok=True)
        lk16 = look.Look16(look.shaper16_linear(), 0, None) if a.bits == 16 else None
        try:
            with Mount(r, opt, basename="/" + os.path.basename(a.src)) as m:
                spec = dict(kind=a.kind, dtype=a.dtype, layout=a.layout, mean=a.mean, std=a.std)
                if a.kind == "rgb":
                    spec.update(gain=a.gain, full=a.full, size=a.size, resample=a.resample, look16=lk16)
                k = 0
                for t in m.tensors(a.first, count, batch=a.batch, **spec):
                    for frame in to_numpy(t):
                        np.save(names[k], frame)
                        k += 1
        finally:
            if lk16 is not None:
                lk16.close()
    print(f"{count} tensors of shape {tuple(frame.shape)} ({a.dtype}) written to {a.outdir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Rewrite a clip with lossless-JPEG payloads (what `mlv_dump -c` writes) or plain packed ones (--plain, `mlv_dump -d`) on the GPU:
mlvfs_amd_mlv_transcode (csrc/mlvwriter.cpp).

    python tools/mlv_transcode.py SRC.MLV DST.MLV [--plain] [--bits N] [--batch N] [--io-threads N] [--dark DARK.MLV [--dark-frames A:B]]
                                                 [--flat FLAT.MLV]

Source chunks SRC.M00 ... become DST.M00 ...; blocks keep the source's file order, NULL and XREF blocks are dropped, nothing is
overwritten and no .IDX is written.  Plain output of a plain or LZMA clip needs no GPU.  --dark: the clip DARK.MLV (its frames A .. B - 1,
default all) is averaged into a dark frame first, which is then subtracted from every frame (mlvfs_amd_dark_from_clip,
mlvfs_amd_mlv_transcode_dark; what `mlv_dump -a` and `-s` do).  --bits N: the clip at N bits per pixel, 8..16 (what `mlv_dump -b` does:
pixels and levels shifted without rounding, after the dark frame; RAWI rewritten; mlvfs_amd_mlv_transcode_bits).  --flat: the clip
FLAT.MLV of an evenly lit target is averaged into a flat field (with --dark, the dark frame is subtracted from it too) whose gain
corrects every frame after the dark frame and before --bits (mlvfs_amd_flat_from_clip, mlvfs_amd_mlv_transcode_cal; what `mlv_dump -t`
does)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlvfs_amd import mlvfile
from mlvfs_amd.dark import Dark
from mlvfs_amd.flat import Flat


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--plain", action="store_true", help="plain packed payloads instead of LJ92")
    ap.add_argument("--bits", type=int, default=0, metavar="N", help="bits per pixel of the output, 8..16 (default: the clip's)")
    ap.add_argument("--batch", type=int, default=0, help="frames per GPU batch (default 8)")
    ap.add_argument("--io-threads", type=int, default=0)
    ap.add_argument("--dark", metavar="PATH", help="a clip of dark frames: averaged, then subtracted from every frame")
    ap.add_argument("--dark-frames", metavar="A:B", help="the frames of --dark to average (default: all)")
    ap.add_argument("--flat", metavar="PATH", help="a clip of an evenly lit target: averaged into a gain plane that corrects every frame")
    a = ap.parse_args()
    if a.dark_frames and not a.dark:
        ap.error("--dark-frames needs --dark")
    if a.bits and not 8 <= a.bits <= 16:
        ap.error("--bits takes 8 to 16")
    dark = None
    if a.dark:
        with mlvfile.MlvReader(a.dark) as dr:
            lo, _, hi = (a.dark_frames or ":").partition(":")
            first = int(lo) if lo else 0
            count = (int(hi) if hi else dr.frame_count) - first
            t0 = time.perf_counter()
            dark = Dark.from_clip(dr, first, count, batch=a.batch, io_threads=a.io_threads)
            print(f"dark frame: the mean of {count} frame(s) of {a.dark} in {time.perf_counter() - t0:.3f} s, pedestal {dark.info()['black']}")
    flat = None
    if a.flat:
        with mlvfile.MlvReader(a.flat) as fr:
            t0 = time.perf_counter()
            # a dark frame of another geometry than the flat clip's is refused there, as it is for the clip itself
            flat = Flat.from_clip(fr, dark=dark, batch=a.batch, io_threads=a.io_threads)
            i = flat.info()
            print(f"flat field: the mean of {i['frames_averaged']} frame(s) of {a.flat} in {time.perf_counter() - t0:.3f} s, channel means {i['means']}")
    with mlvfile.MlvReader(a.src) as r:
        t0 = time.perf_counter()
        s = r.transcode(a.dst, lj92=not a.plain, batch=a.batch, io_threads=a.io_threads, dark=dark, bits=a.bits or None, flat=flat)
        dt = time.perf_counter() - t0
    if flat is not None:
        flat.close()
    if dark is not None:
        dark.close()
    print(f"{s['frames']} frames in {s['files']} file(s), {dt:.3f} s ({s['frames'] / dt:.1f} frames/s): payload bytes {s['bytes_in']} -> {s['bytes_out']}"
          f" ({s['bytes_out'] / max(s['bytes_in'], 1):.3f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Write a clip as a sequence of rendered half-size sRGB TIFF frames: every frame as the mount serves it with these options, developed
to 8-bit RGB at half size on the GPU (mlvfs_amd_mount_rgb; include/mlvfs_amd.h, "rendered half-size sRGB frames") -- or, with --jpeg,
as baseline JPEG files encoded on the GPU (mlvfs_amd_mount_jpeg; "rendered frames as baseline JPEG files").  --full renders at the size
the clip was shot, demosaiced on the GPU (mlvfs_amd_mount_rgb_full, mlvfs_amd_mount_jpeg_full; "rendered full-size sRGB frames");
--size WxH at any size up to the half size, and --fit WxH at the largest such size inside that box at the frame's aspect, area-averaged in
linear light on the GPU (mlvfs_amd_mount_rgb_scaled, mlvfs_amd_mount_jpeg_scaled; "rendered frames at any smaller size").
--resample makes --size and --fit mean the frame's own W x H grid: any size up to the full size, area-averaged from the full-size
rendering's demosaiced channels (mlvfs_amd_mount_rgb_resampled, mlvfs_amd_mount_jpeg_resampled; "rendered frames resampled from the
full-size rendering") -- 3584 x 1320 --resample --fit 1920x1080 writes 1920 x 707.
--lut FILE.cube puts a 3D table, interpolated tetrahedrally on the GPU, in the place of the sRGB curve of every one of these routes
(mlvfs_amd_mount_set_look; "a look for the rendered frames"); --lut-input says what the table's input axis means: the sRGB value the
plain rendering would write (the default), linear light, or log2:STOPS -- a pure log curve over that many stops below white.
--full --demosaic amaze demosaics with AMaZE instead of the linear filter (mlvfs_amd_mount_set_demosaic; "rendered full-size frames
demosaiced by AMaZE"), with TIFF, --jpeg, --bits 16 and --lut alike.  --resample (--size WxH | --fit WxH) --demosaic amaze resamples
that AMaZE rendering instead of the linear one (mlvfs_amd_mount_set_resample_demosaic; "resampled rendered frames demosaiced by AMaZE").
--bits 16 writes 16-bit TIFF files toned from 16-bit linear light (mlvfs_amd_mount_rgb16 and its forms; "rendered frames at 16 bits"):
--lut-input's curve on the 16-bit index (linear: the file holds linear light itself), --lut's table behind it if one is given.

    python tools/mlv_render.py SRC.MLV OUTDIR [--gain G] [--full | --size WxH | --fit WxH] [--resample] [--demosaic amaze] [--jpeg [QUALITY]] [--sampling 444|422|420] [--bits 16] [--lut FILE.cube] [--lut-input srgb|linear|log2:STOPS] [--cs N] [--bad-pix N] [--stripes] [--dual-iso N] [--hdr-interp N]
                                             [--pattern-noise] [--deflicker T] [--dark DARK.MLV] [--flat FLAT.MLV]
                                             [--first A] [--count N] [--batch N] [--io-threads N]

OUTDIR/<clip>_000000.tif ... hold (W // 2) x (H // 2) RGB pixels (W x H with --full, the size asked for with --size or --fit) behind a 256-byte baseline TIFF header: any viewer opens them, any
editing program takes the sequence as an offline proxy.  --gain is the only exposure control (the deflicker's bias is not applied: it
only shapes the frame through the stages in front).  Frames are served in order, as one MLVFS process would serve them.  Nothing is
overwritten: an existing file of the sequence ends the run before any frame is served.  --jpeg writes OUTDIR/<clip>_000000.jpg ...
(quality 1 .. 100, 90 if none is given); a frame whose JPEG file would be larger than its TIFF is written as the .tif.  --sampling
chooses their chroma sampling (mlvfs_amd_mount_set_jpeg_sampling; "the chroma sampling of the JPEG files"): 420, the default, halves
chroma both ways, 422 along the row only, 444 keeps it whole."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mlvfs_amd import amaze_resample, look, mlvfile, resample, scale
from mlvfs_amd.dark import Dark
from mlvfs_amd.flat import Flat
from mlvfs_amd.mount import Mount
from mlvfs_amd.pipeline import MlvfsOptions


def wxh(text: str) -> tuple[int, int]:
    w, x, h = text.lower().partition("x")
    if not (x and w.isdigit() and h.isdigit() and int(w) >= 1 and int(h) >= 1):
        raise argparse.ArgumentTypeError(f"{text!r} is not WxH")
    return int(w), int(h)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("src")
    ap.add_argument("outdir")
    ap.add_argument("--gain", type=float, default=1.0, help="exposure factor, in steps of 1 / 256 (1 / 256 .. 255.996)")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--full", action="store_true", help="render at full size (a fixed 5x5 linear demosaic) instead of half size")
    how.add_argument("--size", type=wxh, metavar="WxH", help="render at W x H, at most half the frame's size a side (an area average in linear light)")
    how.add_argument("--fit", type=wxh, metavar="WxH", help="render at the largest size inside a box of W x H at the frame's aspect")
    ap.add_argument("--demosaic", default="linear", choices=("linear", "amaze"), help="with --full or --resample: the demosaic -- the fixed 5x5 "
                    "linear filter (default) or AMaZE (frames of 36x36 and more whose width is a multiple of 4)")
    ap.add_argument("--resample", action="store_true", help="with --size or --fit: any size up to the frame's own, resampled from the full-size "
                    "rendering (not with --full)")
    ap.add_argument("--jpeg", type=int, nargs="?", const=90, default=0, metavar="QUALITY", help="write baseline JPEG files (default quality 90)")
    ap.add_argument("--sampling", default=None, choices=("444", "422", "420"), help="with --jpeg: the chroma sampling, 4:4:4, 4:2:2 or 4:2:0 (default)")
    ap.add_argument("--bits", type=int, default=8, choices=(8, 16), help="16: 16-bit TIFF files toned from 16-bit linear light through --lut-input's "
                    "curve (and --lut's table behind it, if given); not with --jpeg")
    ap.add_argument("--lut", metavar="FILE.cube", help="a 3D .cube table (domain 0 .. 1, up to 65 a side) applied to every rendering")
    ap.add_argument("--lut-input", default="srgb", metavar="srgb|linear|log2:STOPS", help="what the table's input axis means (default srgb); "
                    "with --bits 16 and no --lut: the curve the files carry")
    ap.add_argument("--cs", type=int, default=0, choices=(0, 2, 3, 5), help="chroma smoothing")
    ap.add_argument("--bad-pix", type=int, default=0, choices=(0, 1, 2), help="bad-pixel repair (2: aggressive)")
    ap.add_argument("--stripes", action="store_true", help="vertical stripes correction")
    ap.add_argument("--dual-iso", type=int, default=0, choices=(0, 1, 2), help="1 preview, 2 full conversion")
    ap.add_argument("--hdr-interp", type=int, default=0, choices=(0, 1), help="0 AMaZE + edge-directed, 1 mean23")
    ap.add_argument("--pattern-noise", action="store_true")
    ap.add_argument("--deflicker", type=int, default=0, metavar="T", help="target level, 0 = off")
    ap.add_argument("--dark", metavar="PATH", help="a clip of dark frames: averaged, then subtracted from every frame")
    ap.add_argument("--flat", metavar="PATH", help="a clip of an evenly lit target: averaged into a gain plane that corrects every frame")
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--count", type=int, default=0, help="frames to write (default: to the end of the clip)")
    ap.add_argument("--batch", type=int, default=8, help="frames per GPU batch")
    ap.add_argument("--io-threads", type=int, default=0)
    a = ap.parse_args()
    if not 1 <= round(256 * a.gain) <= 65535:
        ap.error(f"--gain {a.gain} outside 1 / 256 .. 65535 / 256")
    if a.jpeg and not 1 <= a.jpeg <= 100:
        ap.error(f"--jpeg {a.jpeg} outside 1 .. 100")
    if a.sampling and not a.jpeg:
        ap.error("--sampling takes --jpeg: only JPEG files have a chroma sampling")
    if a.bits == 16 and a.jpeg:
        ap.error("--bits 16 --jpeg: there are no 16-bit JPEG files")
    if a.resample and (a.full or not (a.size or a.fit)):
        ap.error("--resample takes --size or --fit, and no --full")
    if a.demosaic != "linear" and not (a.full or a.resample):
        ap.error("--demosaic amaze takes --full or --resample: only the full-size rendering and what is resampled from it have a demosaic to choose")
    cube = deep = None
    if a.lut or a.bits == 16:
        try:
            table = look.read_cube(a.lut) if a.lut else (0, None)
            if a.bits == 16:
                deep = (look.shaper16(a.lut_input),) + table
            else:
                cube = (look.shaper(a.lut_input),) + table
        except (OSError, ValueError) as e:
            ap.error(f"--lut {a.lut}: {e}" if a.lut else f"--lut-input: {e}")
    stem = os.path.splitext(os.path.basename(a.src))[0]
    opt = MlvfsOptions(chroma_smooth=a.cs, fix_bad_pixels=a.bad_pix, fix_stripes=int(a.stripes), dual_iso=a.dual_iso,
                       hdr_interpolation_method=a.hdr_interp, fix_pattern_noise=int(a.pattern_noise))
    dark = flat = lk = lk16 = None
    with mlvfile.MlvReader(a.src) as r:
        count = a.count or r.frame_count - a.first
        if a.first < 0 or count <= 0 or a.first + count > r.frame_count:
            ap.error(f"frames {a.first} .. {a.first + count - 1} outside the clip ({r.frame_count} frames)")
        size = a.size
        if a.size or a.fit:
            ok, fh = r.frame_headers(a.first)
            if not ok:
                ap.error(f"frame {a.first} has no usable headers")
            try:
                route = (amaze_resample if a.demosaic == "amaze" else resample) if a.resample else scale
                if a.fit:
                    size = route.fit(fh.rawi_hdr.xRes, fh.rawi_hdr.yRes, *a.fit)
                route.geom(fh.rawi_hdr.xRes, fh.rawi_hdr.yRes, *size)
            except ValueError as e:
                ap.error(str(e))
        names = [os.path.join(a.outdir, f"{stem}_{k:06d}.tif") for k in range(a.first, a.first + count)]
        jpgs = [n[:-4] + ".jpg" for n in names]
        taken = [n for n in names + (jpgs if a.jpeg else []) if os.path.exists(n)]
        if taken:
            print(f"{taken[0]} exists ({len(taken)} of {count} files): nothing is overwritten", file=sys.stderr)
            return 1
        os.makedirs(a.outdir, exist_ok=True)
        try:
            if a.dark:
                with mlvfile.MlvReader(a.dark) as dr:
                    dark = Dark.from_clip(dr, 0, dr.frame_count, batch=a.batch, io_threads=a.io_threads)
            if a.flat:
                with mlvfile.MlvReader(a.flat) as fr:
                    flat = Flat.from_clip(fr, dark=dark, batch=a.batch, io_threads=a.io_threads)
            if cube:
                lk = look.Look(*cube)
            if deep:
                lk16 = look.Look16(*deep)
            t0, total = time.perf_counter(), 0
            with Mount(r, opt, deflicker=a.deflicker, basename="/" + os.path.basename(a.src), dark=dark, flat=flat) as m:
                if lk is not None:
                    m.set_look(lk)
                if a.demosaic != "linear" and a.resample:
                    m.set_resample_demosaic(a.demosaic)
                elif a.demosaic != "linear":
                    m.set_demosaic(a.demosaic)
                if a.sampling:
                    m.set_jpeg_sampling(":".join(a.sampling))
                for f0 in range(0, count, a.batch):
                    n = min(a.batch, count - f0)
                    if a.jpeg:
                        files, flags = m.jpeg(a.first + f0, n, gain=a.gain, quality=a.jpeg, batch=a.batch, io_threads=a.io_threads, full=a.full,
                                              size=size, resample=a.resample)
                        targets = [names[f0 + k] if flags[k] & 1 else jpgs[f0 + k] for k in range(n)]
                    else:
                        files = [f.tobytes() for f in m.rgb(a.first + f0, n, gain=a.gain, batch=a.batch, io_threads=a.io_threads, full=a.full,
                                                            size=size, look16=lk16, resample=a.resample)]
                        targets = names[f0:f0 + n]
                    for name, data in zip(targets, files):
                        with open(name, "xb") as out:                       # "x": never over a file that appeared meanwhile
                            out.write(data)
                        total += len(data)
            dt = time.perf_counter() - t0
        finally:
            if lk is not None:
                lk.close()
            if lk16 is not None:
                lk16.close()
            if flat is not None:
                flat.close()
            if dark is not None:
                dark.close()
    print(f"{count} rendered file(s) in {a.outdir}, {dt:.3f} s ({count / dt:.1f} frames/s), {total / count:.0f} bytes per file")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Frames/s of a 3584x1320 clip served as .dng files through the mount (mlvfs_amd_mount_dng: batches, every stage on the GPU)
against the same frames through the drop-in sequence from one thread (payload read, pipeline.process_frame, main.c's deflicker
on the library's hist_* symbols, dng_get_header_data), and against the same option sets served as losslessly compressed files
(mlvfs_amd_mount_dng_lossless: fps and bytes per file), alternating the three in one process.  File-read- and PCIe-inclusive.

usage: python tools/mount_bench.py [frames] [dir]
       python tools/mount_bench.py --pn-kernels batch|single     pattern noise only, for a rocprofv3 --kernel-trace --stats run
       python tools/mount_bench.py --pn-stats kernel_stats.csv FRAMES    k_pn_* kernel time per frame from such a run
       python tools/mount_bench.py --enc-kernels batch|single    the LJ92 encoder only (frames in HBM in batches of 8 | lj92_encode per
                                                                 frame from host memory), 7168x660 at 16 bits as the mount encodes
       python tools/mount_bench.py --enc-stats kernel_stats.csv FRAMES   k_lje_* kernel time per frame from such a run"""
import ctypes as C
import csv
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlvfs_amd import lib, mlvfile, pipeline, synth            # noqa: E402
from mlvfs_amd.mount import Mount                              # noqa: E402
from mlvfs_amd.pipeline import MlvfsOptions                    # noqa: E402

W, H = 3584, 1320
PN_FRAMES = 32


def pn_kernels(mode):
    import torch
    L = lib.load()
    lib.check(L.mlvfs_amd_init(0), "init")
    f = synth.normal_frame(W, H, seed=1)
    geom = lib.Geom(W, H, 14, synth.BLACK, synth.WHITE, 0, 0)
    if mode == "batch":
        d = torch.from_numpy(np.ascontiguousarray(np.stack([f] * 8)).view(np.int16)).cuda()
        for _ in range(PN_FRAMES // 8):
            lib.check(L.mlvfs_amd_fix_pattern_noise_dev(C.byref(geom), C.c_void_p(d.data_ptr()), W * H * 2, 8, None), "pn batch")
    else:
        for _ in range(PN_FRAMES):
            g = f.copy()
            L.fix_pattern_noise(lib.ptr(g), W, H, synth.WHITE, 0)
    print(f"pattern noise ({mode}): {PN_FRAMES} frames of {W}x{H}")


def pn_stats(path, frames):
    tot = 0.0
    for r in csv.DictReader(open(path)):
        if "k_pn_" in r["Name"]:
            tot += float(r["TotalDurationNs"])
    print(f"k_pn_* kernels: {tot / 1e6:.2f} ms for {frames} frames = {tot / 1e6 / frames:.3f} ms per frame")


def enc_kernels(mode):
    import torch
    from mlvfs_amd import lj92
    L = lib.load()
    lib.check(L.mlvfs_amd_init(0), "init")
    frames = [synth.normal_frame(W, H, seed=1, frame=k).reshape(H // 2, 2 * W) for k in range(8)]
    total = 0
    if mode == "batch":
        d = torch.from_numpy(np.ascontiguousarray(np.stack(frames)).view(np.int16)).cuda()
        for _ in range(PN_FRAMES // 8):
            streams, _, status = lj92.encode_batch(d, bits=16)
            assert status == [0] * 8
            total += sum(len(s) for s in streams)
    else:
        for k in range(PN_FRAMES):
            total += len(lj92.encode(frames[k % 8], 2 * W, H // 2, 16))
    print(f"lj92 encoder ({mode}): {PN_FRAMES} frames of {2 * W}x{H // 2}, {total / PN_FRAMES:.0f} bytes per stream")


def enc_stats(path, frames):
    tot, parts = 0.0, []
    for r in csv.DictReader(open(path)):
        if "k_lje_" in r["Name"]:
            tot += float(r["TotalDurationNs"])
            parts.append((r["Name"].split("(")[0], float(r["TotalDurationNs"]) / 1e3 / frames))
    for name, us in sorted(parts, key=lambda p: -p[1]):
        print(f"  {name:40s} {us:8.2f} us per frame")
    print(f"k_lje_* kernels: {tot / 1e6:.2f} ms for {frames} frames = {tot / 1e3 / frames:.1f} us per frame")


def lossless_call(m, count, out, sizes, flags, res):
    lib.check(m.L.mlvfs_amd_mount_dng_lossless(m.h, 0, count, lib.ptr(out), out.shape[1], lib.ptr(sizes), lib.ptr(flags), 8, 0, lib.ptr(res)),
              "mount_dng_lossless")


def dropin_frames(r, opt, deflicker, first, count, mlv_name):
    """main.c:908-1005 per frame on the drop-in symbols (one thread); returns the .dng bytes"""
    L = lib.load()
    out = []
    for k in range(first, first + count):
        ok, fh = r.frame_headers(k)
        packed = r.read_frames(k, 1, (W * H * 14 // 8 + 2 + 15) // 16 * 16, io_threads=1)[0].view(np.uint16)
        img = pipeline.get_image_data(fh, packed).reshape(H, W)
        if deflicker:                                                    # main.c:895-906
            black, white = fh.rawi_hdr.raw_info.black_level, (1 << fh.rawi_hdr.raw_info.bits_per_pixel) + 1
            hist = L.hist_create(white)
            L.hist_add(hist, C.c_void_p(img.ctypes.data + 2), (img.nbytes - 1) // 2, 1)
            med = L.hist_median(hist)
            L.hist_destroy(hist)
            corr = np.log2(np.float64(deflicker - black) / np.float64(med - black))
            fh.rawi_hdr.raw_info.exposure_bias[0] = int(corr * 10000)
            fh.rawi_hdr.raw_info.exposure_bias[1] = 10000
        hdr = np.zeros(65536, np.uint8)
        L.dng_get_header_data(C.byref(fh), lib.ptr(hdr), 0, 65536, 0.0, b"/BENCH.MLV")
        img = pipeline.process_frame(packed, fh, opt, mlv_name)
        if fh.rawi_hdr.raw_info.black_level != synth.BLACK:              # converted: the header again
            L.dng_get_header_data(C.byref(fh), lib.ptr(hdr), 0, img.nbytes, 0.0, b"/BENCH.MLV")
        out.append((hdr, img))
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    d = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="mountbench")
    L = lib.load()
    lib.check(L.mlvfs_amd_init(0), "init")
    normal = [synth.normal_frame(W, H, seed=1, frame=k) for k in range(8)]
    dual = [synth.dual_iso_frame(W, H, frame=k) for k in range(4)]
    clips = {}
    for name, frames, count in (("NORMAL", normal, n), ("DUAL", dual, max(8, n // 3))):
        pl = [np.ascontiguousarray(synth.pack_bits(frames[k % len(frames)]), "<u2").tobytes() for k in range(count)]
        clips[name] = (mlvfile.write_clip(os.path.join(d, name + ".MLV"), pl, W, H, chunks=2), count)
    base = dict(chroma_smooth=5, fix_bad_pixels=1, fix_stripes=1)
    sets = [
        ("cs5+badpix+stripes", "NORMAL", MlvfsOptions(**base), 0),
        ("+pattern noise", "NORMAL", MlvfsOptions(**base, fix_pattern_noise=1), 0),
        ("+pattern noise+deflicker", "NORMAL", MlvfsOptions(**base, fix_pattern_noise=1), 3000),
        ("dual_iso=1", "DUAL", MlvfsOptions(dual_iso=1), 0),
        ("dual_iso=2 (amaze-edge)", "DUAL", MlvfsOptions(dual_iso=2), 0),
    ]
    print(f"{W}x{H}, clips of {clips['NORMAL'][1]} / {clips['DUAL'][1]} frames; best of 2 alternating runs each", flush=True)
    for label, clip, opt, defl in sets:
        names, count = clips[clip]
        best_m = best_d = best_l = 0.0
        sizes, flags, res = np.zeros(count, np.uintp), np.zeros(count, np.int32), np.zeros(count, np.int32)
        with mlvfile.MlvReader(names[0]) as r:
            for rep in range(3):                                         # rep 0 warms both (allocations, tables, page cache)
                with Mount(r, opt, deflicker=defl, basename="/BENCH.MLV") as m:
                    t0 = time.perf_counter()
                    m.dng(0, count, batch=8)
                    fm = count / (time.perf_counter() - t0)
                with Mount(r, opt, deflicker=defl, basename="/BENCH.MLV") as m:
                    t0 = time.perf_counter()
                    out = np.zeros((count, m.dng_size(0)), np.uint8)         # what m.dng allocates inside its time
                    lossless_call(m, count, out, sizes, flags, res)
                    fl = count / (time.perf_counter() - t0)
                t0 = time.perf_counter()
                dropin_frames(r, opt, defl, 0, count, names[0])
                fd = count / (time.perf_counter() - t0)
                if rep:
                    best_m, best_d, best_l = max(best_m, fm), max(best_d, fd), max(best_l, fl)
        print(f"{label:28s} mount {best_m:7.1f} fps   drop-in sequence (1 thread) {best_d:7.1f} fps   x{best_m / best_d:.2f}   "
              f"lossless {best_l:7.1f} fps, {sizes.mean():9.0f} of {out.shape[1]} bytes per file ({sizes.mean() / out.shape[1]:.3f}), "
              f"{int((flags & 1).sum())} uncompressed", flush=True)
    for names, _ in clips.values():
        for p in names:
            os.remove(p)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--pn-kernels":
        pn_kernels(sys.argv[2])
    elif len(sys.argv) > 3 and sys.argv[1] == "--pn-stats":
        pn_stats(sys.argv[2], int(sys.argv[3]))
    elif len(sys.argv) > 2 and sys.argv[1] == "--enc-kernels":
        enc_kernels(sys.argv[2])
    elif len(sys.argv) > 3 and sys.argv[1] == "--enc-stats":
        enc_stats(sys.argv[2], int(sys.argv[3]))
    else:
        main()

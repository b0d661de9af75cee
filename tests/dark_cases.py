"""Cases and the numpy oracle of dark-frame subtraction and averaging (csrc/cal.cpp, csrc/k_cal.hip), shared by
tests/test_dark_cases.py (CPU: the cases really test something) and tests/test_gpu_dark.py.

    out     = clamp(px - dark + black_d, 0, 2^bpp - 1)
    dark[p] = (sum over n frames of px_f[p] + n // 2) // n

The reference has no dark-frame code.  The tests tie the definition back to it so: a clip served or rewritten WITH a dark frame must
equal what the reference's own process_frame text gives for a clip whose payloads were subtracted beforehand with subtract() below."""
import struct

import numpy as np

from mlvfs_amd import mlvfile, synth

NAME = "M07-1234.MLV"
W, H = 416, 264
BLACK = synth.BLACK
# where clip_case forces a clamp, away from the borders and from pixel 0 (a first pixel of 0 is a case of its own for the encoders)
TOP_AT = [(20, 30), (21, 31), (100, 200), (101, 203)]            # (y, x): frame pixel near the top over a dark entry below black_d
ZERO_AT = [(40, 50), (41, 53), (150, 300), (151, 301)]           # frame pixel near 0 under a hot dark entry


def subtract(frame, dark, black_d, bpp):
    v = frame.astype(np.int64) - dark.astype(np.int64) + int(black_d)
    return np.clip(v, 0, (1 << bpp) - 1).astype(np.uint16)


def mean(frames):
    n = len(frames)
    total = np.zeros(frames[0].shape, np.uint32)
    for f in frames:
        total += f.astype(np.uint32)                                      # 32-bit unsigned sums: the library's
    return ((total + np.uint32(n // 2)) // np.uint32(n)).astype(np.uint16)


def clamp_classes(frame, dark, black_d, bpp):
    """-> (pixels that clamp at 0, pixels that clamp at the top, pixels that do neither)"""
    v = frame.astype(np.int64) - dark.astype(np.int64) + int(black_d)
    top = (1 << bpp) - 1
    return int((v < 0).sum()), int((v > top).sum()), int(((v >= 0) & (v <= top)).sum())


def clip_black(bpp):
    return BLACK >> (14 - bpp) if bpp <= 14 else BLACK << (bpp - 14)


def sub_case(w, h, bpp, n, black_d, seed=0):
    """n frames of w x h at bpp bits and a dark plane with pedestal black_d -> (frames, dark, wanted frames).  The plane is the
    pedestal with a little fixed pattern; its first entries are "hot" (near white, under frame pixels near 0: the result clamps at 0)
    and its last ones lie below the pedestal (under frame pixels near the top: the result clamps at 2^bpp - 1)."""
    rng = np.random.default_rng(1000 * w + 10 * h + bpp + n + seed)
    top, black = (1 << bpp) - 1, clip_black(bpp)
    npix = w * h
    frames = [rng.integers(max(black - 8, 0), top * 9 // 10, npix).astype(np.uint16) for _ in range(n)]
    dark = np.clip(black_d + rng.integers(-6, 7, npix), 0, top).astype(np.uint16)
    k = max(1, min(4, npix // 4))
    dark[:k] = top - 5
    dark[-k:] = black_d // 4
    for f in frames:
        f[:k] = rng.integers(0, 4, k)
        f[-k:] = top - rng.integers(0, 3, k)
    frames = [f.reshape(h, w) for f in frames]
    dark = dark.reshape(h, w)
    return frames, dark, [subtract(f, dark, black_d, bpp) for f in frames]


SUB_GEOMETRIES = [(16, 2), (48, 6), (2, 2), (30, 10), (416, 264)]
SUB_CASES = [(w, h, bpp, n, off) for (w, h) in SUB_GEOMETRIES for bpp in (10, 12, 14, 16) for n in (1, 3) for off in (0, -37)]


def avg_case(w, h, n, seed=0):
    """n 14-bit frames of w x h -> (frames, their rounded mean).  Pixel 0's sum is n * v + n // 2 (for an even n exactly half way: the
    mean rounds up to v + 1), pixel 1's is one below that (rounds down to v), pixel 2's one above."""
    rng = np.random.default_rng(77 * w + 5 * h + n + seed)
    frames = [rng.integers(BLACK - 40, BLACK + 400, (h, w)).astype(np.uint16) for _ in range(n)]
    v = BLACK + 13
    for f in frames:
        f[0, :3] = v
    for px, extra in ((0, n // 2), (1, n // 2 - 1), (2, n // 2 + 1)):
        for k in range(max(extra, 0)):
            frames[k % n][0, px] += 1
    return frames, mean(frames)


# the 16-pixel form and the pixel-per-lane form (w * h a multiple of 8, not of 16: a 14-bit payload then ends on a whole word, which
# a clip's frame_size = w * h * bpp / 8 bytes must do for the file to hold the last pixel at all)
AVG_GEOMETRIES = [(64, 48), (30, 12)]
AVG_COUNTS = [1, 2, 7]


def dark_plane(w=W, h=H, black_d=BLACK, seed=3):
    """A plane as a camera's dark clip averages to: the pedestal, a column pattern, a little noise, hot entries, and entries below the
    pedestal; TOP_AT and ZERO_AT hold the entries that force the two clamps of clip_case."""
    rng = np.random.default_rng(seed)
    plane = black_d + rng.integers(-5, 6, (h, w)) + (np.arange(w) % 8 == 3) * 9
    hot = rng.integers(0, w * h, 40)
    plane.reshape(-1)[hot] = rng.integers(3000, 16000, 40)
    scale_y, scale_x = h / H, w / W
    for (y, x) in TOP_AT:
        plane[int(y * scale_y), int(x * scale_x)] = black_d // 2
    for (y, x) in ZERO_AT:
        plane[int(y * scale_y), int(x * scale_x)] = 16000
    return np.clip(plane, 0, 16383).astype(np.uint16)


def clip_frames(kind="plain", n=5, w=W, h=H):
    """The frames of the clips the mount and transcoder tests serve (14 bits): test_gpu_ref_host.make_clip's material with pixels near
    the top over the plane's low entries and pixels near 0 under its hot ones."""
    frames = []
    scale_y, scale_x = h / H, w / W
    for k in range(n):
        f = synth.dual_iso_frame(w, h, frame=k) if kind == "dual_iso" else synth.normal_frame(w, h, seed=9, frame=k, hot=60, cold=60)
        f = np.ascontiguousarray(f, np.uint16).copy()
        for i, (y, x) in enumerate(TOP_AT):
            f[int(y * scale_y), int(x * scale_x)] = 16383 - (i + k) % 3
        for i, (y, x) in enumerate(ZERO_AT):
            f[int(y * scale_y), int(x * scale_x)] = (i + k) % 4
        frames.append(f)
    return frames


def clip_case(kind="plain", n=5, w=W, h=H, black_d=BLACK):
    """-> (frames, dark plane, the frames subtracted beforehand)"""
    frames, dark = clip_frames(kind, n, w, h), dark_plane(w, h, black_d)
    return frames, dark, [subtract(f, dark, black_d, 14) for f in frames]


# Other bit depths and a size that is no multiple of 16 pixels, through the reader's load (mount, transcoder): 12 and 10 bits take
# k_cal_unpack_x16<12 | 10, true, false>; 16 bits and 30 x 12 take the two-pass fallback of launch_cal_unpack (k_unpack_generic, then k_cal_apply)
DEPTH_CASES = [(W, H, 12), (W, H, 10), (64, 48, 16), (30, 12, 14), (30, 12, 12)]


def depth_case(w, h, bpp, n=3):
    """clip_case's material at bpp bits -> (frames, dark plane, pedestal, the frames subtracted beforehand)"""
    frames, dark = clip_frames("plain", n, w, h), dark_plane(w, h)
    if bpp < 14:
        frames, dark = [f >> (14 - bpp) for f in frames], dark >> (14 - bpp)
    else:
        frames, dark = [f << (bpp - 14) for f in frames], dark << (bpp - 14)
    black_d = clip_black(bpp)
    return frames, dark, black_d, [subtract(f, dark, black_d, bpp) for f in frames]


def write_clip(d, frames, payload="plain", reference=None, bpp=14, name=NAME):
    """frames -> a two-chunk clip in directory d (made here), payloads plain, LZMA (the reference's compressor) or LJ92; black and
    white level are those of 14 bits scaled to bpp"""
    d.mkdir()
    h, w = frames[0].shape
    vc = 1
    if payload == "lj92":
        from oracle import lj92_testenc as enc
        from test_lj92 import quadrants
        pl, vc = [struct.pack("<I", w * h * 2) + enc.encode(quadrants(f), 6, bpp) for f in frames], 1 | 0x100
    elif payload == "lzma":
        pl, vc = [reference.lzma_payload(synth.pack_bits(f, bpp).tobytes()) for f in frames], 1 | 0x80
    else:
        pl = [np.ascontiguousarray(synth.pack_bits(f, bpp), "<u2").tobytes() for f in frames]
    shift = 14 - bpp
    black, white = (BLACK >> shift, synth.WHITE >> shift) if shift >= 0 else (BLACK << -shift, synth.WHITE << -shift)
    mlvfile.write_clip(str(d / name), pl, w, h, bpp=bpp, black=black, white=white, chunks=2, frame_space=32, shuffle=True, video_class=vc)
    return d

"""Cases and the numpy oracle of a clip rewritten at another bit depth (mlvfs_amd_mlv_transcode_bits, mlvfs_amd_repack_dev,
mlvfs_amd_rawi_set_bits: csrc/mlvwriter.cpp, csrc/k_mlvpack.hip), shared by tests/test_bits_cases.py (CPU: the rule
for RAWI, the refusals, and that the cases really test something) and tests/test_gpu_bits.py.

    d = out_bpp - bpp        out = px >> -d  (d < 0: truncation)        out = px << d  (d > 0)        out = px  (d = 0)

black_level and white_level shift like pixels, pitch = raw_info.width * out_bpp / 8, frame_size = xRes * yRes * out_bpp / 8.  The
reference has no such code.  The tests tie the definition back to it so: a clip rewritten at out_bpp must be served by the
reference's own reader and process_frame text exactly as the EXPECTED clip is -- mlvfile.write_clip of the frames converted with
convert() below, at out_bpp, with the shifted levels.  The expected clip is written with the source's block layout, so
test_mlv_transcode.check_container compares an output against it block by block: its RAWI block is the one the rule asks for, every
other block is the source's (sources_other_blocks_are_the_expected_clips says so)."""
import struct

import numpy as np

from mlvfs_amd import mlvfile, synth

NAME = "M07-1234.MLV"
W, H = 416, 264
# the levels of a 14-bit source: odd, so that narrowing truncates them (2047 >> 2 = 511 where rounding gives 512; 15001 >> 2 = 3750)
BLACK14, WHITE14 = 2047, 15001
# where source_frames puts the top of the range and 0, away from the borders and from pixel 0 (a first pixel of 0 is a case of its own
# for the encoders)
TOP_AT = [(20, 30), (21, 31), (100, 200), (101, 203)]
ZERO_AT = [(40, 50), (41, 53), (150, 300), (151, 301)]


def shift(v, d):
    return v << d if d >= 0 else v >> -d


def convert(frame, bpp, out_bpp):
    """The definition."""
    f = np.asarray(frame).astype(np.uint32)
    return (shift(f, out_bpp - bpp) & 0xFFFF).astype(np.uint16)


def levels(bpp):
    """(black, white) of a source clip at bpp bits: BLACK14 / WHITE14 at 14 bits' scale"""
    return shift(BLACK14, bpp - 14), shift(WHITE14, bpp - 14)


def out_levels(bpp, out_bpp):
    b, w = levels(bpp)
    return shift(b, out_bpp - bpp), shift(w, out_bpp - bpp)


def source_frames(bpp=14, n=5, w=W, h=H):
    """test_gpu_ref_host.make_clip's material at bpp bits, with pixels at 2^bpp - 1 and at 0"""
    frames = []
    sy, sx = h / H, w / W
    for k in range(n):
        f = np.ascontiguousarray(synth.normal_frame(w, h, seed=9, frame=k, hot=60, cold=60), np.uint16).copy()
        f = convert(f, 14, bpp)
        for y, x in TOP_AT:
            f[int(y * sy), int(x * sx)] = (1 << bpp) - 1
        for y, x in ZERO_AT:
            f[int(y * sy), int(x * sx)] = 0
        frames.append(f)
    return frames


_lj92 = {}


def payloads(frames, bpp, kind="plain", reference=None):
    """-> (payload bytes per frame, video class)"""
    h, w = frames[0].shape
    if kind == "lj92":
        from oracle import lj92_testenc as enc
        from test_lj92 import quadrants
        key = (bpp, len(frames), hash(b"".join(f.tobytes() for f in frames)))          # (the test encoder is Python: once per material)
        if key not in _lj92:
            _lj92[key] = [struct.pack("<I", w * h * 2) + enc.encode(quadrants(f), 6, bpp) for f in frames]
        return _lj92[key], 1 | 0x100
    if kind == "lzma":
        return [reference.lzma_payload(synth.pack_bits(f, bpp).tobytes()) for f in frames], 1 | 0x80
    return [np.ascontiguousarray(synth.pack_bits(f, bpp), "<u2").tobytes() for f in frames], 1


def write_clip(d, frames, bpp, kind="plain", reference=None, black=None, white=None, name=NAME):
    """frames -> a two-chunk clip in directory d (made here) with plain, LZMA (the reference's compressor) or LJ92 payloads"""
    d.mkdir()
    h, w = frames[0].shape
    pl, vc = payloads(frames, bpp, kind, reference)
    b, wh = levels(bpp)
    mlvfile.write_clip(str(d / name), pl, w, h, bpp=bpp, black=b if black is None else black, white=wh if white is None else white,
                       chunks=2, frame_space=32, shuffle=True, video_class=vc)
    return d


def expected_clip(d, frames, bpp, out_bpp, name=NAME):
    """The clip a conversion of `frames` (bpp bits) to out_bpp must be served like: numpy's conversion, write_clip's RAWI at out_bpp."""
    b, wh = out_levels(bpp, out_bpp)
    return write_clip(d, [convert(f, bpp, out_bpp) for f in frames], out_bpp, black=b, white=wh, name=name)


def rawi_of(path):
    """the first chunk's RAWI block"""
    data, pos = open(path, "rb").read(), 0
    while pos + 16 <= len(data):
        size = struct.unpack_from("<I", data, pos + 4)[0]
        if data[pos:pos + 4] == b"RAWI":
            return data[pos:pos + size]
        pos += size
    raise AssertionError("no RAWI block in " + path)


# mlvfs_amd_repack_dev: (w, h): one group of 16 pixels, less than a wave, more than one block per frame; 2 x 2 and 30 x 10 take the
# word-per-lane kernel at any depth
REPACK_GEOMETRIES = [(16, 2), (48, 6), (416, 264), (2, 2), (30, 10)]
FAST_DEPTHS = [(i, o) for i in (14, 12, 10) for o in (14, 12, 10) if i != o]
GENERIC_DEPTHS = [(14, 16), (16, 12)]
REPACK_CASES = [(w, h, i, o, n) for (w, h) in REPACK_GEOMETRIES for (i, o) in FAST_DEPTHS + GENERIC_DEPTHS for n in (1, 3)]
# the clips test_gpu_bits.py rewrites: (source depth, out_bpp)
CLIP_DEPTHS = [(14, 12), (14, 10), (12, 14)]


def repack_frames(w, h, bpp, n, seed=0):
    """n frames over the whole range of bpp bits; the first pixels are the top of the range and 0"""
    rng = np.random.default_rng(1000 * w + 10 * h + bpp + n + seed)
    frames = [rng.integers(0, 1 << bpp, w * h).astype(np.uint16) for _ in range(n)]
    for f in frames:
        f[0], f[1] = (1 << bpp) - 1, 0
    return [f.reshape(h, w) for f in frames]


def small_frames(bpp=14, n=3, w=30, h=12):
    """30 x 12: no multiple of 16 pixels (w * h a multiple of 8: a 14-, 12- or 10-bit payload ends on a whole word).
    40 x 12 (SMALL_X8): whole groups of 16 pixels in rows of 8k + 8 -- the tiling's 8-pixel form and the other passes' 16-pixel forms."""
    return source_frames(bpp, n, w, h)


SMALL_X8 = (40, 12)
# the 40 x 12 clips test_gpu_bits.py rewrites to LJ92: (payload kind, source depth, out_bpp) -- an LJ92 source narrowed and widened
# (the tiling shifts, d < 0 and d > 0), and a 10-bit plain source (the one source depth CLIP_DEPTHS does not have)
SMALL_X8_CLIPS = [("lj92", 14, 12), ("lj92", 12, 14), ("plain", 10, 12)]


def full_size_frames():
    return source_frames(14, 2, 3584, 1320)


def hot16_frames(w=64, h=48):
    """Three quiet 14-bit frames; the middle one has a pixel at the top of the range beside a pixel of its colour at 0.  At 14 bits
    every frame encodes; widened to 16 bits the difference between the two is one of class 16."""
    frames = [np.ascontiguousarray(synth.normal_frame(w, h, seed=2, frame=k) >> 4, np.uint16) for k in range(3)]
    frames[1][10, 10], frames[1][10, 12] = 16383, 0
    return frames


def dark_case():
    """dark_cases.clip_case: (frames, dark plane, the frames subtracted beforehand with numpy), 14 bits, pedestal 2048"""
    import dark_cases as dc
    return dc.clip_case("plain")

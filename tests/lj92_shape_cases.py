"""The JPEG shapes the LJ92 decoder's prediction kernels are tested at (csrc/k_lj92.hip: k_lj_rows, k_lj_vhalve, k_lj_diagonals,
k_lj_wavefront, k_lj_column_sums, k_lj_columns), shared by tests/test_lj92_shape_cases.py (CPU: the reference's decoder, the oracle and
the source image agree on every stream; the LDS rule of k_lj_rows holds; the list reaches what it is there to reach) and
tests/test_gpu_lj92_shapes.py (GPU: every case against the oracle, bit for bit).

A CASE is a list of streams that go to the decoder in ONE call, and the video geometry the values are re-read as (main.c:646-667) or
None: the decoder's own order, for shapes whose value count has no even x even factorisation.  Shapes are written H x W, the JPEG's
own rows x values per row.  What the list is there for:

  wide rows     k_lj_rows stages a row of up to 8192 values in LDS and works on a longer one in place in global memory; its loops over
                the row's blocks of 32 columns are `for (b = threadIdx.x; b < nblk; b += 256)`, so only rows beyond 8192 values take
                a second trip.  4 x 8192 is the widest staged row, 4 x 8194 the narrowest even one that is not (257 blocks: one block
                on the second trip), 2 x 65534 / 2 x 65535 the widest a stream's header can say.
  mixed         frames on both sides of 8192 in one call: the launch's LDS is sized once, from the widest frame, and every frame
                finds its place in it by the same rule (csrc/lj92.h: lj_row_plan, seen here through mlvfs_amd_test_lj92_row_plan).
                Nine frames: sub-batches of four on alternating streams.  Every frame's expected result is the oracle's for that
                stream ALONE.
  block edges   widths around the edges of the 32-column blocks (the last block's length feeds a shift), a single column.
  single row    H = 1: every column segment of k_lj_column_sums / k_lj_columns is empty.
  16 bits       predictors 4 to 7 on 16-bit samples, staged and in place.
  predictor 7   LJ_WAVE_MAX_H = 8192 rows decode, 8193 are refused before any kernel runs.

Streams come from oracle/lj92_testenc.py (every predictor); a predictor-6 stream at 14 bits comes from the reference's own encoder
where the caller hands in the `reference` fixture.

THE REFERENCE AT H = 1, PREDICTOR 6: lj92.c's predictor-6 loop returns LJ92_ERROR_CORRUPT as soon as the read position has reached
the end of the data when the first row is done (lj92.c:442, 456) -- which is where a one-row image ends.  The oracle (and the
library) decode such a stream; the reference refuses it.  Predictor 6 is therefore left out of the single-row case, and
test_lj92_shape_cases.py pins both sides (REF_REFUSES), so that a change of either gets noticed."""
import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np

from mlvfs_amd import lib, synth
from oracle import lj92_testenc as enc


class Frame(NamedTuple):
    h: int
    w: int
    pred: int
    bits: int = 14
    image: str = "noise"         # "noise": 14-bit noise; "normal16": synth.normal_frame(256, 130, seed=9) << 2, its first h * w values
    seed: int = 0
    ramp: bool = False           # lj92_testenc's fixed code lengths 2..15


class Case(NamedTuple):
    name: str
    frames: Tuple[Frame, ...]
    video: Optional[Tuple[int, int]]     # (xres, yres), or None: the decoder's own order
    wide: bool = False                   # wide rows go through the batched entry point AND the drop-in symbols


def _wide():
    out = []
    for (h, w), video in (((4, 8192), (8192, 4)), ((4, 8194), (8194, 4)), ((4, 9216), (192, 192)), ((2, 65534), (65534, 2)),
                          ((3, 8193), None), ((2, 65535), None)):
        frames = [Frame(h, w, p, seed=w + p) for p in range(8)]
        if (h, w) == (4, 9216):
            frames.append(Frame(h, w, 6, seed=w + 8, ramp=True))
        out.append(Case(f"wide {h}x{w}", tuple(frames), video, wide=True))
    return out


MIXED_SHAPES = [(192, 192), (4, 9216), (9, 4096), (72, 512)]
MIXED_VIDEO = (192, 192)


def _mixed():
    wide, narrow = (4, 9216), (72, 512)
    out = []
    for p in (6, 1):
        out.append(Case(f"mixed wide-narrow p{p}", (Frame(*wide, p, seed=1), Frame(*narrow, p, seed=2)), MIXED_VIDEO))
        out.append(Case(f"mixed narrow-wide p{p}", (Frame(*narrow, p, seed=3), Frame(*wide, p, seed=4)), MIXED_VIDEO))
    out.append(Case("mixed four shapes", tuple(Frame(h, w, p, seed=10 + k) for k, ((h, w), p) in enumerate(zip(MIXED_SHAPES, (6, 6, 1, 6)))), MIXED_VIDEO))
    preds = (1, 4, 5, 6, 7)                             # (7 where H <= 8192: every shape here)
    out.append(Case("mixed nine frames", tuple(Frame(*MIXED_SHAPES[k % 4], preds[k % 5], seed=20 + k) for k in range(9)), MIXED_VIDEO))
    return out


EDGE_WIDTHS = (1, 2, 3, 31, 32, 33, 34, 63, 64, 65, 66)


def _edges():
    out = [Case(f"edge 6x{w}", tuple(Frame(6, w, p, seed=100 + w) for p in (1, 4, 5, 6)), None) for w in EDGE_WIDTHS]
    out.append(Case("edge 64x1", tuple(Frame(64, 1, p, seed=99) for p in (1, 4, 5, 6)), None))
    return out


def _rest():
    return [
        Case("single row 1x36864", tuple(Frame(1, 36864, p, seed=200 + p) for p in (0, 1, 2, 3, 4, 5, 7)), (192, 192)),
        Case("16 bits 130x256", tuple(Frame(130, 256, p, bits=16, image="normal16") for p in range(8)), (256, 130)),
        Case("16 bits 2x9216", tuple(Frame(2, 9216, p, bits=16, image="normal16") for p in (4, 5, 6, 7)), None),
        Case("predictor 7 at 8192 rows", (Frame(8192, 2, 7, seed=300),), (128, 128)),
    ]


CASES = _wide() + _mixed() + _edges() + _rest()
# one row more than k_lj_wavefront keeps in LDS: refused ("limited to"), in the decoder's own order
REFUSED_P7 = Frame(8193, 2, 7, seed=301)
# the one stream the reference's decoder refuses and the oracle decodes (the module's docstring)
REF_REFUSES = Frame(1, 36864, 6, seed=206)


def image(f: Frame) -> np.ndarray:
    if f.image == "normal16":
        full = ((synth.normal_frame(256, 130, seed=9).astype(np.uint32) << 2) & 0xFFFF).astype(np.uint16).reshape(-1)
        return np.ascontiguousarray(full[: f.h * f.w].reshape(f.h, f.w))
    assert f.image == "noise"
    return np.random.default_rng(1000 + f.seed).integers(0, 1 << 14, (f.h, f.w)).astype(np.uint16)


_streams = {}


def stream(f: Frame, reference=None) -> bytes:
    """The frame's JPEG stream (made once per session: the test encoder is Python)"""
    by_ref = reference is not None and f.pred == 6 and f.bits == 14 and not f.ramp
    key = (f, by_ref)
    if key not in _streams:
        img = image(f)
        _streams[key] = reference.lj92_encode(img, 14) if by_ref else enc.encode(img, f.pred, f.bits, ramp=f.ramp)
    return _streams[key]


def streams(case: Case, reference=None):
    return [stream(f, reference) for f in case.frames]


# ------------------------------------------------------------------ k_lj_rows' LDS, as the library itself cuts it
def row_plan(w: int, max_w: int) -> dict:
    """mlvfs_amd_test_lj92_row_plan: a row of w values in a launch whose widest frame has max_w"""
    out = (C.c_longlong * 4)()
    rc = lib.load().mlvfs_amd_test_lj92_row_plan(w, max_w, out)
    assert rc == 0, (w, max_w)
    return dict(staged=bool(out[0]), stage_off=int(out[1]), stage_end=int(out[2]), lds_bytes=int(out[3]))


def blocks(w: int) -> int:
    """Blocks of 32 columns in a row of w values (nblk of the first row's prefix sum), counted from the carries the launch reserves: one
    per block and two spare, 8 bytes each, in front of the staged row"""
    return row_plan(w, w)["stage_off"] // 8 - 2


def trips(w: int) -> int:
    """Trips of k_lj_rows' block loops (256 threads)"""
    return -(-blocks(w) // 256)


def calls(case: Case):
    """The (w, max_w) of every launch of k_lj_rows a case makes: the whole list in one call, and -- through the drop-in symbols, for
    cases in the decoder's own order and for wide rows -- every stream alone"""
    out = []
    max_w = max(f.w for f in case.frames)
    out += [(f.w, max_w) for f in case.frames]
    if case.video is None or case.wide:
        out += [(f.w, f.w) for f in case.frames]
    return out


def describe(case: Case) -> str:
    """One line per case for a summary: shape, predictor, path through k_lj_rows and the trips of its block loops"""
    max_w = max(f.w for f in case.frames)
    parts = []
    for f in case.frames:
        p = row_plan(f.w, max_w)
        parts.append(f"{f.h}x{f.w} p{f.pred}/{f.bits}b {'staged' if p['staged'] else 'in place'} {blocks(f.w)} blocks {trips(f.w)} trip(s)")
    return f"{case.name} [{'raw order' if case.video is None else '%dx%d' % case.video}, LDS {row_plan(max_w, max_w)['lds_bytes']}]: " + "; ".join(parts)

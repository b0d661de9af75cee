"""tests/mount_harness.py on the CPU: its checks of a served TIFF and JPEG file accept the definition's files and refuse each of them
with one thing wrong, so the one copy asserts what the copies it replaced asserted; and its table of routes gives, for a synthetic
.dng file, what a direct call of each route's definition gives, plain, with a look and with a deep look, at the size the route's
geometry rule gives."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import abi, amaze_render, amaze_resample, demosaic, jpeg, lib, render, resample, scale, synth

import deep_cases as dp
import look_cases as lc
import mount_harness as mh

W, H, Q = 24, 16, 85
SIZE = (W, H)
RNG = np.random.default_rng(5)
PX = np.kron(RNG.integers(0, 256, (2, 3, 3)), np.ones((8, 8, 1), np.int64)).astype(np.uint8)       # 24 x 16 in flat blocks: a short stream
PX16 = RNG.integers(0, 65536, (H, W, 3)).astype(np.uint16)
NOISE = RNG.integers(0, 256, (8, 8, 3)).astype(np.uint8)                                          # at quality 100 the TIFF is the smaller


def tiff(px, bits=8):
    return render.tiff_header(px.shape[1], px.shape[0], bits) + np.ascontiguousarray(px, "<u2" if bits == 16 else np.uint8).tobytes()


def jpg(px, q=Q, sampling=420):
    return jpeg.header(px.shape[1], px.shape[0], q, sampling) + jpeg.encode(px, q, None, sampling)


def flip(file, at):
    return file[:at] + bytes([file[at] ^ 1]) + file[at + 1:]


def test_the_checks_accept_the_definitions_files():
    mh.check_tiffs([PX, PX[::-1]], [tiff(PX), tiff(PX[::-1])], SIZE, "tiff")
    mh.check_tiffs([PX16], [tiff(PX16, 16)], SIZE, "tiff16", bits=16)
    for sampling in (420, 422, 444):
        assert len(jpg(PX, Q, sampling)) < len(tiff(PX))
        mh.check_jpegs([PX], [jpg(PX, Q, sampling)], [0], SIZE, "jpeg", Q, sampling)
    mh.check_jpegs([PX, PX], [jpg(PX, 90), jpg(PX, 50)], [0, 0], SIZE, "a quality per file", [90, 50])
    assert len(jpg(NOISE, 100)) > len(tiff(NOISE)), "the case does not reach the fallback"
    mh.check_jpegs([NOISE], [tiff(NOISE)], [1], (8, 8), "fallback", 100)


T8, T16, J, FB = tiff(PX), tiff(PX16, 16), jpg(PX), tiff(NOISE)
WRONG = {
    "tiff: a pixel byte": lambda: mh.check_tiffs([PX], [flip(T8, mh.HDR + 5)], SIZE, ""),
    "tiff: a header byte": lambda: mh.check_tiffs([PX], [flip(T8, 30)], SIZE, ""),
    "tiff: a byte short": lambda: mh.check_tiffs([PX], [T8[:-1]], SIZE, ""),
    "tiff: a byte long": lambda: mh.check_tiffs([PX], [T8 + b"\0"], SIZE, ""),
    "tiff: a file short": lambda: mh.check_tiffs([PX, PX], [T8], SIZE, ""),
    "tiff: width and height swapped": lambda: mh.check_tiffs([PX], [T8], (H, W), ""),
    "tiff16: a sample byte": lambda: mh.check_tiffs([PX16], [flip(T16, mh.HDR + 5)], SIZE, "", bits=16),
    "tiff16: a header byte": lambda: mh.check_tiffs([PX16], [flip(T16, 30)], SIZE, "", bits=16),
    "tiff16: a byte short": lambda: mh.check_tiffs([PX16], [T16[:-1]], SIZE, "", bits=16),
    "tiff16: a byte long": lambda: mh.check_tiffs([PX16], [T16 + b"\0"], SIZE, "", bits=16),
    "tiff16: a file short": lambda: mh.check_tiffs([PX16, PX16], [T16], SIZE, "", bits=16),
    "tiff16: an 8-bit file": lambda: mh.check_tiffs([PX16], [T8], SIZE, "", bits=16),
    "tiff16: width and height swapped": lambda: mh.check_tiffs([PX16], [T16], (H, W), "", bits=16),
    "jpeg: a stream byte": lambda: mh.check_jpegs([PX], [flip(J, len(J) - 3)], [0], SIZE, "", Q),
    "jpeg: a header byte": lambda: mh.check_jpegs([PX], [flip(J, 30)], [0], SIZE, "", Q),
    "jpeg: a byte short": lambda: mh.check_jpegs([PX], [J[:-1]], [0], SIZE, "", Q),
    "jpeg: a byte long": lambda: mh.check_jpegs([PX], [J + b"\0"], [0], SIZE, "", Q),
    "jpeg: a file short": lambda: mh.check_jpegs([PX, PX], [J], [0, 0], SIZE, "", Q),
    "jpeg: a flag short": lambda: mh.check_jpegs([PX, PX], [J, J], [0], SIZE, "", Q),
    "jpeg: flag 1 without a fallback": lambda: mh.check_jpegs([PX], [J], [1], SIZE, "", Q),
    "jpeg: flag 0 on the fallback": lambda: mh.check_jpegs([NOISE], [FB], [0], (8, 8), "", 100),
    "jpeg: the JPEG file where the fallback is due": lambda: mh.check_jpegs([NOISE], [jpg(NOISE, 100)], [0], (8, 8), "", 100),
    "jpeg: the TIFF where the JPEG file is smaller": lambda: mh.check_jpegs([PX], [T8], [1], SIZE, "", Q),
    "jpeg: the TIFF where the JPEG file is smaller, flag 0": lambda: mh.check_jpegs([PX], [T8], [0], SIZE, "", Q),
    "jpeg: 4:2:0 where 4:4:4 is asked for": lambda: mh.check_jpegs([PX], [J], [0], SIZE, "", Q, 444),
    "jpeg: another quality": lambda: mh.check_jpegs([PX], [J], [0], SIZE, "", 84),
    "jpeg: width and height swapped": lambda: mh.check_jpegs([PX], [J], [0], (H, W), "", Q),
    "jpeg: a pixel byte of the fallback": lambda: mh.check_jpegs([NOISE], [flip(FB, mh.HDR + 5)], [1], (8, 8), "", 100),
}


@pytest.mark.parametrize("what", list(WRONG))
def test_the_checks_refuse(what):
    with pytest.raises(AssertionError):
        WRONG[what]()


# ------------------------------------------------------------------ the routes
FW, FH, GAIN = 40, 36, 1.5                            # a frame every route takes: AMaZE wants 36 x 36 and a width that is a multiple of 4
SIZES = {"scaled": (13, 11), "resampled": (33, 25), "resampled+amaze": (39, 20)}
OUT = {"half": (20, 18), "full": (40, 36), "full+amaze": (40, 36), **SIZES}
TONES = {"plain": {}, "look": dict(look=lc.look_of("random17")), "look16": dict(look16=dp.look_of("random3"))}


@pytest.fixture(scope="module")
def dng(amd):
    """a .dng file as the mount serves it: the header writer's 65536 bytes and a frame's pixels"""
    fh, fps, base = synth.header_case(0)
    header = np.zeros(65536, np.uint8)
    assert amd.dng_get_header_data(C.byref(abi.FrameHeaders.from_buffer_copy(bytes(fh))), lib.ptr(header), 0, 65536, float(fps), base) == 65536
    frame = synth.normal_frame(FW, FH, seed=3)
    return header.tobytes() + np.ascontiguousarray(frame, "<u2").tobytes(), frame


def direct(route, frame, p, amaze, **tone):
    size = SIZES.get(route, ())
    if route.endswith("+amaze"):
        return (amaze_resample if size else amaze_render).render(frame, p, amaze, *size, **tone)
    return {"half": render, "full": demosaic, "scaled": scale, "resampled": resample}[route].render(frame, p, *size, **tone)


@pytest.mark.parametrize("tone", list(TONES))
@pytest.mark.parametrize("route", list(mh.ROUTES))
def test_renderings_are_the_routes_definition(dng, oracle, route, tone):
    file, frame = dng
    p = render.params_from_header(file[:65536], int(round(256 * GAIN)))
    got = mh.renderings([file, file], [GAIN, 1.0], FW, FH, route, SIZES.get(route), oracle.amaze_demosaic, **TONES[tone])
    want = direct(route, frame, p, oracle.amaze_demosaic, **TONES[tone])
    assert len(got) == 2 and got[0].dtype == (np.uint16 if tone == "look16" else np.uint8) and np.array_equal(got[0], want)
    assert not np.array_equal(got[1], want), "the gain did not reach the parameters"
    assert len(np.unique(want)) > 16, "the frame renders to next to nothing: the case shows little"
    ow, oh = mh.out_size(route, FW, FH, SIZES.get(route))
    assert (ow, oh) == OUT[route] == mh.out_size(mh.route_args(route, SIZES.get(route)), FW, FH) and want.shape == (oh, ow, 3)
    with pytest.raises(AssertionError):
        mh.renderings([file[:-2]], [GAIN], FW, FH, route, SIZES.get(route), oracle.amaze_demosaic)        # the length of each .dng is held


def test_the_routes_sizes_are_the_geometry_rules():
    assert render.geom(FW, FH) == OUT["half"] and demosaic.geom(FW, FH) == OUT["full"] and amaze_render.geom(FW, FH) == OUT["full+amaze"]
    for route, geom in (("scaled", scale.geom), ("resampled", resample.geom), ("resampled+amaze", amaze_resample.geom)):
        geom(FW, FH, *SIZES[route])                  # a size the route gives
        assert mh.route_args(route, SIZES[route])["size"] == OUT[route]
    assert mh.route_args("half") == {} and mh.route_args("full") == mh.route_args("full+amaze") == dict(full=True)
    assert mh.route_args("resampled", (3, 2)) == mh.route_args("resampled+amaze", (3, 2)) == dict(size=(3, 2), resample=True)

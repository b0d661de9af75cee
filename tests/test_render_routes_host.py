"""The six rendering routes' geometry rules, the library's host code (no GPU): for the smallest shapes on either side of every limit, the
Python yardstick's geom() of a route, the exported mlvfs_amd_rgb*_geom, the fits with a 1x1 box and the route's three device calls
(plain, look, deep) give one answer -- taken or refused, and the same W' x H' where one comes out -- and the three tones of one route
refuse a shape in the same words.  Only refused shapes reach the device calls: a refusal happens before any device work, a shape that
is taken would go on to the device.  No frame is allocated."""
import ctypes as C

import numpy as np
import pytest

from mlvfs_amd import amaze_render, amaze_resample, demosaic, lib, render, resample, scale

FRAMES = [(1, 1), (2, 2), (3, 3), (4, 4), (3, 8), (8, 3), (35, 36), (36, 35), (36, 36), (38, 36), (40, 36),
          (65535, 4), (65536, 4),                                  # a side of the full-size grid
          (131070, 2), (131071, 2), (131072, 2),                   # a side of the half-size grid
          (8192, 4095), (8192, 4096),                              # 2^25 pixels
          (16384, 8191), (16384, 8192)]                            # 2^27 pixels
SIZED = [(64, 48), (36, 36)]                                       # the frames the output sizes are held against


def half_geom(w, h):
    """render.geom gives W' x H' of any frame; the route's own limits are 2x2 and 2^27 pixels (include/mlvfs_amd.h)"""
    if w < 2 or h < 2 or w * h >= 1 << 27:
        raise ValueError(f"{w}x{h}")
    return render.geom(w, h)


# route: the yardstick's geom, whether it takes an output size, the frame's largest output size
ROUTES = {
    "render2": (half_geom, False, None),
    "render1": (demosaic.geom, False, None),
    "render_scaled": (scale.geom, True, lambda w, h: (w // 2, h // 2)),
    "render_resampled": (resample.geom, True, lambda w, h: (w, h)),
    "render1_amaze": (amaze_render.geom, False, None),
    "render_resampled_amaze": (amaze_resample.geom, True, lambda w, h: (w, h)),
}


def shapes(route):
    """[(w, h, ow, oh)]; ow = oh = None on a route that takes no output size"""
    _, sized, largest = ROUTES[route]
    if not sized:
        return [(w, h, None, None) for w, h in FRAMES + SIZED]
    out = [(w, h, 1, 1) for w, h in FRAMES]
    for w, h in SIZED:
        mw, mh = largest(w, h)
        out += [(w, h, ow, oh) for ow in (0, 1, mw, mw + 1, -1) for oh in (0, 1, mh, mh + 1, -1)]
    return out


def yardstick(route, w, h, ow, oh):
    """W' x H' of the rendering, or None where the yardstick refuses"""
    geom, sized, _ = ROUTES[route]
    try:
        size = geom(w, h, ow, oh) if sized else geom(w, h)
    except ValueError:
        return None
    return (ow, oh) if sized else size


def exported(amd, name, w, h):
    pw, ph = C.c_int(-7), C.c_int(-7)
    rc = getattr(amd, name)(w, h, C.byref(pw), C.byref(ph))
    assert rc in (0, lib.ERR_ARG), (name, w, h, rc)
    if rc:
        assert b"not supported" in amd.mlvfs_amd_last_error() and (pw.value, ph.value) == (-7, -7), (name, w, h)
        return None
    return pw.value, ph.value


@pytest.mark.parametrize("route,name", [("render2", "mlvfs_amd_rgb_geom"), ("render1", "mlvfs_amd_rgb_full_geom"), ("render1_amaze", "mlvfs_amd_rgb_amaze_geom")])
def test_the_exported_geometry_is_the_yardsticks(amd, route, name):
    for w, h, ow, oh in shapes(route):
        assert exported(amd, name, w, h) == yardstick(route, w, h, ow, oh), (name, w, h)


def test_the_exported_amaze_resample_geometry_is_the_yardsticks(amd):
    for w, h, ow, oh in shapes("render_resampled_amaze"):
        rc = amd.mlvfs_amd_rgb_amaze_resample_geom(w, h, ow, oh)
        want = yardstick("render_resampled_amaze", w, h, ow, oh)
        assert rc == (0 if want else lib.ERR_ARG), (w, h, ow, oh)
        if rc:
            assert b"not supported" in amd.mlvfs_amd_last_error()


@pytest.mark.parametrize("route,name,fit", [("render_scaled", "mlvfs_amd_rgb_fit", scale.fit), ("render_resampled", "mlvfs_amd_rgb_fit_full", resample.fit)])
def test_a_fit_with_a_1x1_box_takes_the_frames_the_route_takes(amd, route, name, fit):
    for w, h in FRAMES + SIZED:
        ow, oh = C.c_int(-7), C.c_int(-7)
        rc = getattr(amd, name)(w, h, 1, 1, C.byref(ow), C.byref(oh))
        if yardstick(route, w, h, 1, 1) is None:
            assert rc == lib.ERR_ARG and (ow.value, oh.value) == (-7, -7), (name, w, h)
            with pytest.raises(ValueError):
                fit(w, h, 1, 1)
        else:
            assert rc == 0 and (ow.value, oh.value) == fit(w, h, 1, 1) == (1, 1), (name, w, h)


@pytest.mark.parametrize("route", list(ROUTES))
def test_the_device_calls_refuse_what_the_yardstick_refuses(amd, route):
    """the refused shapes through mlvfs_amd_<route>_dev, _look_dev and _deep_dev: ERR_ARG, "not supported", one message for the three
    tones.  The pointers are host memory that no check follows; nothing is written"""
    src, dst, par = np.full(64, 0x0707, np.uint16), np.full(64, 9, np.uint8), np.zeros(16, np.int32)
    s, d, p = (C.c_void_p(a.ctypes.data) for a in (src, dst, par))
    sized = ROUTES[route][1]
    refused = [sh for sh in shapes(route) if yardstick(route, *sh) is None]
    taken = [sh for sh in shapes(route) if yardstick(route, *sh) is not None]
    assert refused and taken, route
    for w, h, ow, oh in refused:
        size = (ow, oh) if sized else ()
        messages = []
        for tone, look in (("", ()), ("_look", (s,)), ("_deep", (s,))):
            call = getattr(amd, f"mlvfs_amd_{route}{tone}_dev")
            assert call(s, 128, w, h, p, *size, d, 64, 1, *look, None) == lib.ERR_ARG, (route, tone, w, h, ow, oh)
            messages.append(amd.mlvfs_amd_last_error())
            assert b"not supported" in messages[-1] and messages[-1].startswith(route.encode() + b":"), (route, tone, messages[-1])
        assert messages[0] == messages[1] == messages[2], (route, w, h, ow, oh, messages)
    assert (src == 0x0707).all() and (dst == 9).all() and not par.any()


def test_the_routes_nest():
    """what the yardsticks say of one another, on the same shapes: an AMaZE route takes no frame its linear route refuses, a resampled
    route none its full-size route refuses, the scaled route none the half-size route refuses"""
    for w, h in FRAMES + SIZED:
        took = {r: yardstick(r, w, h, 1, 1) is not None for r in ROUTES}
        for inner, outer in (("render1_amaze", "render1"), ("render_resampled_amaze", "render_resampled"), ("render_resampled_amaze", "render1_amaze"),
                             ("render_resampled", "render1"), ("render_scaled", "render2")):
            assert not took[inner] or took[outer], (inner, outer, w, h)

"""The fused pass across black levels, white levels and stripe gains (the cases of tests/level_cases.py, proven non-vacuous on the CPU by
tests/test_level_cases.py), bit-exact against the `oracle` fixture, through every kernel the pass has:

  levels     12 blacks (0, 1, 63, 64, 65, 1023, 2047, 4095, 8191, 16000, 16319, 16384) in 32 pairs with the whites black + 65, black + 64,
             15000, 16383 and 60000; cs 0 / 2 / 3 / 5, a pixel map of either detection mode, realistic stripes -- k_frame_s and k_frame
             (cs2x2 / cs3x3), k_frame_p5, k_frame_p and k_frame (cs5x5), k_frame (no smoothing), forced with MLVFS_AMD_KF_S / _KF_P /
             _KF_P5 on 608x250 (two columns, the last folded in four, five segments, layout 1) and 264x62 (layout 2).
  families   unit, the packed form's last coefficients 65536 +- 32767 (phases 2..7; all; one unit column per dword and its mirror),
             one step beyond (65536 + 32768, 65536 - 32768, 0) and the clamp (gains 1.25 and 65536 + 32767 at white 15000), each at
             blacks 0, 2047 and 8191 through the same kernels.
  edges of the admission rule (csrc/k_frame.hip: launch_frame, coef_pk)
             white = black + 65 / black + 64 at eight blacks, black 16384, |coef - 65536| = 32767 / 32768, coef 0.  After every
             launch the plan it took is read back (mlvfs_amd_test_last_frame_plan): inside the rule the streaming kernel ran, on the
             other side it declined and k_frame_p / k_frame gave the oracle's bytes -- the form is proven by the plan, the rule is
             not restated here.
  depths     12- and 10-bit streams straight into the loader at four blacks and two whites each.
  16 bits    black 8192 / white 60000 with chroma smoothing, map and stripes, and stripes alone over 0 .. 65535 (black 0, pixels of
             65535, d = 32767: the largest product of the 32-bit epilogue); the stage API gives the fused bytes.
  cache      11 black levels in turn and three of them again, cs2x2 and then cs5x5, with a clip of a twelfth level in use between
             them: in a fresh process 6 + 11 evictions from the per-device cache of 8 output tables, 16 parked tables released,
             every level rebuilt at least once.
  lone greens  frames without a pixel at most 64 (or less than 256) above black whose SMOOTHED pixels land there.

What the sweep found: k_frame_p, k_frame_p5 and k_frame_s ran the stripes epilogue without its `a > 64` mask wherever no LOADED pixel
lay at most 64 above black; a smoothed red or blue can (a cell of dim greens among bright ones), stripes.c:261 leaves it alone, and the
kernels moved it -- by one level with realistic gains, by half its height above black at the form's edge.  Single pixels of the
low-light frames at blacks 65, 1023 and 4095 and of the edge families at black 0 showed it; the lone-green frames are
its reduction (csrc/k_frame_dev.h: smoothed_low)."""
import numpy as np
import pytest

import level_cases as LC
import stream_shapes as S
from mlvfs_amd import synth
from stream_shapes import P_NONE, P_P5, P_S, P_TILES

pytestmark = pytest.mark.gpu

POISON = 0x5A5A
SWITCHES = ("MLVFS_AMD_KF_P", "MLVFS_AMD_KF_P5", "MLVFS_AMD_KF_S")
# (switches, the first kernel inside the packed form, the first kernel beyond it, rows per task of the streaming kernel)
S_RUNS = (({"MLVFS_AMD_KF_S": "2"}, P_S, P_NONE, 60), ({"MLVFS_AMD_KF_S": "0"}, P_NONE, P_NONE, 0))
P_RUNS = (({"MLVFS_AMD_KF_P": "2", "MLVFS_AMD_KF_P5": "2"}, P_P5, P_TILES, 30),
          ({"MLVFS_AMD_KF_P": "2", "MLVFS_AMD_KF_P5": "0"}, P_TILES, P_TILES, 0),
          ({"MLVFS_AMD_KF_P": "0"}, P_NONE, P_NONE, 0))
NO_RUNS = (({}, P_NONE, P_NONE, 0),)


@pytest.fixture(scope="module")
def torch_cuda(gpu):
    import torch
    assert torch.cuda.is_available()
    return torch


def switch(monkeypatch, env):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check(got, want, what):
    for k in range(len(want)):
        if not np.array_equal(got[k], want[k]):
            ys, xs = np.nonzero(got[k] != want[k])
            y, x = int(ys[0]), int(xs[0])
            raise AssertionError(f"{what} frame {k}: {len(ys)} px differ, x {xs.min()}..{xs.max()}, y {ys.min()}..{ys.max()}; "
                                 f"at ({x}, {y}) {got[k][y, x]} for {want[k][y, x]}, phases {sorted(set((xs % 8).tolist()))}")


def upload16(torch, frames):
    return torch.from_numpy(np.stack(frames).view(np.int16)).cuda()


def launch(s, src, out, cs, fix, stripes, unpacked=False):
    from mlvfs_amd.stream import to_numpy_u16
    out.fill_(POISON)
    (s.process_unpacked if unpacked else s.process)(src, out, cs=cs, fix_pixels=fix, stripes=stripes)
    return to_numpy_u16(out)


def sweep_kernels(oracle, monkeypatch, w, h, black, white, form, coeffs, methods, mode, quarters=4):
    """One level pair and coefficient set through every kernel of the methods given: cs 0 and 5 with the pixel map, cs 2 / 3 without
    (k_frame_s takes none) and, through k_frame, with it.  Each launch against the oracle, and its plan against the form."""
    from mlvfs_amd.stream import ClipStream
    packed_form = form == "packed"
    clips = {}
    for cs in methods:
        kinds = LC.KINDS[cs]
        if kinds not in clips:
            frames = LC.footage(kinds, w, h, black, quarters)
            clips[kinds] = (frames, oracle.detect_bad_pixels(frames[0], black, mode))
        frames, pixels = clips[kinds]
        s = ClipStream(w, h, 14, black, white, device=0)
        s.set_pixel_map(pixels)
        s.set_stripes(1, coeffs)
        assert S.stripes_form(s, True) == (1 if packed_form else 2), "stream_shapes.stripes_form and the case disagree"
        src = s.upload_packed([synth.pack_bits(f) for f in frames])
        out = s.alloc_out(len(frames))
        with_map = LC.oracle_pass(oracle, frames, black, white, cs, pixels, coeffs)
        mapped = len(pixels) > 0
        if cs in (2, 3):
            without = LC.oracle_pass(oracle, frames, black, white, cs, None, coeffs)
            plan = [(env, False, without, a, b, rows) for env, a, b, rows in S_RUNS]
            plan.append(({"MLVFS_AMD_KF_S": "2"}, True, with_map, P_NONE if mapped else P_S, P_NONE, 60))
        else:
            plan = [(env, True, with_map, a, b, rows) for env, a, b, rows in (P_RUNS if cs == 5 else NO_RUNS)]
        for env, fix, want, inside, beyond, rows in plan:
            switch(monkeypatch, env)
            what = f"{w}x{h} black {black} white {white} cs {cs} map {int(fix)} {env}"
            got = launch(s, src, out, cs, fix, True)
            S.assert_took(inside if packed_form else beyond, w, h, rows, what)
            check(got, want, what)
        s.close()


# ------------------------------------------------------------------ levels x kernels
@pytest.mark.parametrize("case", LC.LEVELS, ids=LC.level_id)
def test_levels_through_every_kernel(torch_cuda, oracle, case, monkeypatch):
    """A level pair with the realistic coefficients, cs 0 / 2 / 3 / 5, through every kernel; at white = black + 64 the streaming kernels
    decline (the plan says so) and the others still give the oracle's bytes"""
    black, kind, form = case
    i = LC.LEVELS.index(case)
    w, h = LC.level_geometry(i)
    sweep_kernels(oracle, monkeypatch, w, h, black, LC.white_of(black, kind), form, LC.REALISTIC, (0, 2, 3, 5), (i // 2) % 2)


# ------------------------------------------------------------------ coefficient families x kernels
@pytest.mark.parametrize("case", LC.FAMILY_CASES, ids=LC.family_id)
def test_coefficient_families_through_every_kernel(torch_cuda, oracle, case, monkeypatch):
    """Coefficients at and one step beyond the packed form's edge, dwords of one unit column, a zero coefficient, gains that clamp: cs
    0, 5 and one of 2 / 3 through every kernel.  Family d: the streaming kernels declined, k_frame_p / k_frame equal the oracle."""
    name, black, white, form, quarters = case
    i = LC.FAMILY_CASES.index(case)
    w, h = LC.family_geometry(i)
    sweep_kernels(oracle, monkeypatch, w, h, black, white, form, LC.FAMILIES[name], (0, 2 + i % 2, 5), i % 2, quarters)


# ------------------------------------------------------------------ smoothed pixels within 64 of black, none loaded there
@pytest.mark.parametrize("black", LC.FAMILY_BLACKS)
@pytest.mark.parametrize("green,dim", LC.LONE_GREEN, ids=["no-pixel-within-64", "no-pixel-within-255"])
def test_smoothed_pixels_within_64_of_black(torch_cuda, oracle, black, green, dim, monkeypatch):
    """level_cases.lone_green_frame: the kernels that choose the output stage's variant from the pixels they load see none at most 64
    (none less than 256) above black, chroma smoothing writes hundreds there, and the stripes epilogue must leave those alone
    (stripes.c:261) -- cs 2 / 3 / 5 with the realistic coefficients through every kernel"""
    from mlvfs_amd.stream import ClipStream
    w, h = LC.GEOMETRIES[0]
    frames = [LC.lone_green_frame(w, h, black, green, dim, 1 + k) for k in range(LC.NFRAMES)]
    s = ClipStream(w, h, 14, black, 16383, device=0)
    s.set_stripes(1, LC.REALISTIC)
    src = s.upload_packed([synth.pack_bits(f) for f in frames])
    out = s.alloc_out(len(frames))
    for cs in (2, 3, 5):
        want = LC.oracle_pass(oracle, frames, black, 16383, cs, None, LC.REALISTIC)
        for env, first, _, rows in (P_RUNS if cs == 5 else S_RUNS):
            switch(monkeypatch, env)
            what = f"lone greens, black {black}, {dim} / {green} above, cs {cs} {env}"
            got = launch(s, src, out, cs, False, True)
            S.assert_took(first, w, h, rows, what)
            check(got, want, what)
    s.close()


# ------------------------------------------------------------------ 12- and 10-bit streams
@pytest.mark.parametrize("bpp,black,white", LC.REDUCED, ids=[f"{b}bit-black{k}-white{w}" for b, k, w in LC.REDUCED])
def test_reduced_depths_at_their_levels(torch_cuda, oracle, bpp, black, white, monkeypatch):
    """The loader's vector layouts 3 / 4 (the streams read directly) with pixel map and stripes in the packed form, every method;
    cs5x5 through k_frame_p and through k_frame (the streaming kernels read 14-bit streams only)"""
    from mlvfs_amd.stream import ClipStream
    for n, (w, h) in enumerate(LC.REDUCED_GEOMETRIES[bpp]):
        frames = LC.footage(LC.KINDS[5], w, h, black, bpp=bpp)
        pixels = oracle.detect_bad_pixels(frames[0], black, (LC.REDUCED.index((bpp, black, white)) + n) % 2)
        s = ClipStream(w, h, bpp, black, white, device=0)
        s.set_pixel_map(pixels)
        s.set_stripes(1, LC.REALISTIC)
        src = s.upload_packed([synth.pack_bits(f, bpp) for f in frames])
        out = s.alloc_out(len(frames))
        for cs in (0, 2, 3, 5):
            want = LC.oracle_pass(oracle, frames, black, white, cs, pixels, LC.REALISTIC)
            for env, first in ((({"MLVFS_AMD_KF_P": "2"}, P_TILES), ({"MLVFS_AMD_KF_P": "0"}, P_NONE)) if cs == 5 else (({}, P_NONE),)):
                switch(monkeypatch, env)
                what = f"{bpp} bits {w}x{h} black {black} white {white} cs {cs} {env}"
                got = launch(s, src, out, cs, True, True)
                S.assert_took(first, what=what)
                check(got, want, what)
        s.close()


# ------------------------------------------------------------------ 16-bit input
@pytest.mark.parametrize("black,name", LC.UNPACKED_STRIPES, ids=[f"black{b}-{n}" for b, n in LC.UNPACKED_STRIPES])
def test_16_bit_stripes_over_the_whole_range(torch_cuda, oracle, black, name):
    """process_unpacked without chroma smoothing: values 0 .. 65535 through the 32-bit epilogue (stripe_px<true>: b, c, e) and the
    64-bit one (d); black 0 with d = 32767 on pixels of 65535 is the largest product __mul24 forms.  stripes_apply gives the same."""
    from mlvfs_amd.stream import ClipStream, to_numpy_u16
    co, white = LC.FAMILIES[name], LC.UNPACKED_WHITE
    for w, h in LC.GEOMETRIES:
        frames = [LC.full_range16(w, h, black, 31 + k) for k in range(LC.NFRAMES)]
        want = LC.oracle_pass(oracle, frames, black, white, 0, None, co)
        s = ClipStream(w, h, 14, black, white, device=0)
        s.set_stripes(1, co)
        src = upload16(torch_cuda, frames)
        what = f"16-bit {w}x{h} black {black} {name}"
        got = launch(s, src, s.alloc_out(len(frames)), 0, False, True, unpacked=True)
        S.assert_took(P_NONE, what=what)
        check(got, want, what)
        check(to_numpy_u16(s.stripes_apply(src.clone())), want, what + ", stripes_apply")
        s.close()


@pytest.mark.parametrize("cs", [2, 3, 5])
def test_16_bit_input_at_dual_iso_levels(torch_cuda, oracle, cs, monkeypatch):
    """What a converted dual-ISO frame looks like: black 8192, white 60000, pixels beyond 14 bits but inside the reference's raw2ev
    table (level_cases.footage16), with pixel map and stripes in the 32-bit and the 64-bit form; cs5x5 through k_frame_p and k_frame.
    The stages one after the other (fix_pixels, chroma_smooth, stripes_apply) give the fused bytes."""
    from mlvfs_amd.stream import ClipStream, to_numpy_u16
    black, white = LC.UNPACKED_BLACK, LC.UNPACKED_WHITE
    for w, h in LC.GEOMETRIES:
        frames = LC.footage16(LC.KINDS[cs], w, h, black)
        pixels = oracle.detect_bad_pixels(frames[0], black, cs % 2)
        for name in LC.UNPACKED_SMOOTH_FAMILIES:
            co = LC.FAMILIES[name]
            want = LC.oracle_pass(oracle, frames, black, white, cs, pixels, co)
            s = ClipStream(w, h, 14, black, white, device=0)
            s.set_pixel_map(pixels)
            s.set_stripes(1, co)
            src = upload16(torch_cuda, frames)
            out = s.alloc_out(len(frames))
            for env, first in ((({"MLVFS_AMD_KF_P": "2"}, P_TILES), ({"MLVFS_AMD_KF_P": "0"}, P_NONE)) if cs == 5 else (({}, P_NONE),)):
                switch(monkeypatch, env)
                what = f"16-bit {w}x{h} cs {cs} {name} {env}"
                got = launch(s, src, out, cs, True, True, unpacked=True)
                S.assert_took(first, what=what)
                check(got, want, what)
            staged = s.stripes_apply(s.chroma_smooth(s.fix_pixels(src.clone()), cs))
            check(to_numpy_u16(staged), want, f"16-bit {w}x{h} cs {cs} {name}, stage API")
            s.close()


# ------------------------------------------------------------------ the per-device cache of output tables
def test_output_table_cache_evicts_and_rebuilds(torch_cuda, oracle, monkeypatch):
    """csrc/k_frame.hip: e2r_table keeps the output tables of 8 black levels per device, evicts the least recently used one and parks
    it until the next eviction.  11 levels in turn, then the first, the second and the last again -- cs2x2, then cs5x5 --, and between
    any two of them a launch of a clip at a twelfth level, whose table therefore stays while its neighbours go.  Every launch equals
    the oracle.  (In a fresh process: six evictions per method round at most, the first two levels rebuilt.)"""
    from mlvfs_amd.stream import ClipStream
    switch(monkeypatch, {})
    w, h = LC.CACHE_GEOMETRY
    order = list(LC.CACHE_LEVELS) + [LC.CACHE_LEVELS[0], LC.CACHE_LEVELS[1], LC.CACHE_LEVELS[-1]]
    clips = {}
    for b in set(order) | {LC.CACHE_NEIGHBOUR}:
        frames = LC.footage(LC.KINDS[2], w, h, b)
        s = ClipStream(w, h, 14, b, 16383, device=0)
        clips[b] = (s, s.upload_packed([synth.pack_bits(f) for f in frames]), s.alloc_out(len(frames)),
                    {cs: LC.oracle_pass(oracle, frames, b, 16383, cs, None, None) for cs in (2, 5)})
    for cs in (2, 5):
        for n, b in enumerate(order):
            for level in (LC.CACHE_NEIGHBOUR, b):
                s, src, out, want = clips[level]
                check(launch(s, src, out, cs, False, False), want[cs], f"cs {cs}, step {n}: black {level}")
    for s, _, _, _ in clips.values():
        s.close()

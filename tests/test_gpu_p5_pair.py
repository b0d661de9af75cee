"""k_frame_p5's pair step against the oracle: tasks of every length parity (tests/p5_pair_cases.py: last segments of 1 .. 4 rows behind
tasks of 30 and of 60 rows, a segment shorter than the warm-up, a frame whose smoothed rows end inside the first rows), and the seams
between the two rows of a pair -- the loader's dark form, a pixel-map cell, an uncertain strip in one row and not in the other.

Every launch is forced through k_frame_p5 and proved from the plan it took (mlvfs_amd_test_last_frame_plan); the output is poisoned
before each launch; everything is bit for bit the oracle's.  The list-mode k_frame does every listed tile again, so the seam cases
also compare what k_frame_p5 listed (mlvfs_amd_test_stream_listed) with what the kernel before the pair step listed for the same input."""
import pytest

import level_cases as LC
import p5_pair_cases as PP
import stream_shapes as S
from mlvfs_amd import synth
from stream_shapes import P_P5
from test_gpu_stream import BLACK, WHITE, make_stream
from test_gpu_stream_shapes import POISON, check_frames, check_on_device, cu_count, repeat

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda(gpu):
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(autouse=True)
def forced(monkeypatch):
    monkeypatch.setenv("MLVFS_AMD_KF_P", "2")
    monkeypatch.setenv("MLVFS_AMD_KF_P5", "2")


@pytest.mark.parametrize("case", PP.CASES, ids=PP.case_id)
def test_task_length_parity(torch_cuda, oracle, case):
    """The benchmark's footage kind, with pixel map and stripes and with neither.  Tasks of 30 rows: a forced short launch of three
    frames; of 60 rows: as many frames as the plan asks for on this device, three distinct ones repeated, every frame compared"""
    torch = torch_cuda
    w, h, seg_rows = case
    frames = S.footage("normal", w, h, 3)
    for pmap, stripes in ((True, True), (False, False)):
        # (the clip's pixel map -- the oracle's detection on the first frame -- and stripe gains are set from outside, as
        # tests/test_gpu_p5_loop_edges.py does: only the steady-state pass runs here)
        pixels = oracle.detect_bad_pixels(frames[0], BLACK, 0) if pmap else None
        coeffs = LC.REALISTIC if stripes else None
        want = LC.oracle_pass(oracle, frames, BLACK, WHITE, 5, pixels, coeffs)
        nf = 3 if seg_rows == 30 else S.frames_for_60_rows(w, h, cu_count(torch), pmap and len(pixels) > 0, int(stripes))
        assert (nf * w * h * 15) // 4 < 6 << 30
        s = make_stream(w, h)
        if pmap:
            s.set_pixel_map(pixels)
        if stripes:
            s.set_stripes(1, coeffs)
        packed = repeat(torch, s.upload_packed([synth.pack_bits(f) for f in frames]), nf)
        out = s.alloc_out(nf)
        out.fill_(POISON)
        s.process(packed, out, cs=5, fix_pixels=pmap, stripes=stripes)
        what = f"map {int(pmap)} stripes {int(stripes)}, {nf} frames"
        S.assert_took(P_P5, w, h, seg_rows, what)
        check_on_device(torch, out, want, w, h, seg_rows, what)
        s.close()
        del packed, out


@pytest.mark.parametrize("kind", PP.SEAM_KINDS)
def test_pair_seams(torch_cuda, oracle, kind):
    """Two frames in one launch: what the case is about happens in the first row of a pair in one and in the second row of a pair in
    the other; the partner row has none of it"""
    from mlvfs_amd.stream import to_numpy_u16
    w, h = PP.SEAM_GEOMETRY
    frames = PP.seam_frames(kind)
    pm = PP.seam_pixel_map(kind)
    want = [oracle.chroma_smooth(f if pm is None else oracle.apply_bad_pixels(f, BLACK, pm), BLACK, 5) for f in frames]
    s = make_stream(w, h)
    if pm is not None:
        s.set_pixel_map(pm)
    packed = s.upload_packed([synth.pack_bits(f) for f in frames])
    out = s.alloc_out(2)
    out.fill_(POISON)
    before = S.listed_tiles()
    s.process(packed, out, cs=5, fix_pixels=pm is not None, stripes=False)
    S.assert_took(P_P5, w, h, 30, kind)
    listed = S.listed_tiles() - before
    print(f"pair seam {kind}: {listed} of {S.launch_tiles(w, h, 2)} tiles listed")
    check_frames(to_numpy_u16(out), want, w, h, 30, kind)
    assert listed == PP.PARENT_LISTED[kind], f"{kind}: k_frame_p5 listed {listed} tiles, the kernel before the pair step {PP.PARENT_LISTED[kind]}"
    s.close()

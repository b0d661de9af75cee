"""The stripe analysis's histograms (csrc/k_stripes.hip; StripesWork and stripes_solve in clip.cpp) against the oracle's, bin by bin.

The coefficients are medians of 10^4 .. 10^6 samples and do not move when a few hundred samples land in the wrong bin, a block reads
its dither from the wrong place or a counter is flushed twice; the (8, 65536) histogram does.  It is taken through the shard entry
points (mlvfs_amd_stripes_count_dev / _hist_dev), with the dither of mlvfs_amd_rand_stream(seed 1), and compared with
oracle.stripes_compute(want_hist=True) on the frames of tests/stripes_hist_cases.py: both ends of the LDS window and the clamped
bins, calls exactly on a bin edge (host re-binning and k_hist_bump), every threshold of accepted() at six level pairs, widths of one
and two groups, frames with no and with one accepted call, and a geometry long enough for the second and third pass of
k_scan_blocks and the round loop of k_stripes_hist.  tests/test_stripes_hist_cases.py shows on the CPU that the frames do what they
are there for."""
import ctypes as C

import numpy as np
import pytest

import stripes_hist_cases as SC
from mlvfs_amd import abi, lib, synth

pytestmark = pytest.mark.gpu

H = SC.SMALL_H


@pytest.fixture(scope="module")
def torch_cuda(gpu):
    import torch
    assert torch.cuda.is_available()
    return torch


def rand_stream(L, n_calls: int) -> np.ndarray:
    rnd = np.zeros(2 * n_calls + 2, np.uint16)
    L.mlvfs_amd_rand_stream(lib.ptr(rnd), 2 * n_calls, 0, 1)
    return rnd


def device_hist(torch, L, f, black, white, edges, repeat: int = 1):
    """The histogram of frame `f` by the shards of rows edges[k] .. edges[k + 1], each added `repeat` times into one device
    histogram -> (hist[8, 65536], num[8], accepted calls per shard)"""
    h, w = f.shape
    geom = lib.Geom(w, h, 14, black, white, 0, 0)
    frame = torch.from_numpy(f.view(np.int16)).cuda()
    dp = lambda t: C.c_void_p(t.data_ptr())
    counts = []
    for r0, r1 in zip(edges[:-1], edges[1:]):
        acc = C.c_int64(-1)
        lib.check(L.mlvfs_amd_stripes_count_dev(C.byref(geom), dp(frame), r0, r1, C.byref(acc), None), "count_dev")
        counts.append(acc.value)
    d_rnd = torch.from_numpy(rand_stream(L, sum(counts)).view(np.int16)).cuda()
    d_hist = torch.zeros(8 * 65536, dtype=torch.int32, device="cuda")
    d_num = torch.zeros(8, dtype=torch.int32, device="cuda")
    off = 0
    for k, (r0, r1) in enumerate(zip(edges[:-1], edges[1:])):
        acc = C.c_int64(-1)
        lib.check(L.mlvfs_amd_stripes_count_dev(C.byref(geom), dp(frame), r0, r1, C.byref(acc), None), "count_dev")
        assert acc.value == counts[k]
        for _ in range(repeat):
            lib.check(L.mlvfs_amd_stripes_hist_dev(C.byref(geom), dp(frame), r0, r1, C.c_void_p(d_rnd.data_ptr() + 4 * off),
                                                   2 * counts[k], dp(d_hist), dp(d_num), None), "hist_dev")
        off += counts[k]
    torch.cuda.synchronize()
    return d_hist.cpu().numpy().reshape(8, 65536), d_num.cpu().numpy(), counts


def differences(got, want) -> str:
    j, k = np.nonzero(got != want)
    inside = (k >= SC.LWIN_LO) & (k < SC.LWIN_LO + SC.LWIN)
    first = [f"(hist {a}, bin {b}, got {got[a, b]}, want {want[a, b]}, {'inside' if i else 'outside'} the LDS window)"
             for a, b, i in zip(j[:8], k[:8], inside[:8])]
    return f"{j.size} bins differ, {int(inside.sum())} of them inside the LDS window: " + ", ".join(first)


def check_against_oracle(L, got, want, frame_size, scale: int = 1):
    hist, num, counts = got
    needed, coeffs, hist_ref, num_ref = want
    assert sum(counts) == int(num_ref.sum())
    assert np.array_equal(hist, scale * hist_ref), differences(hist, scale * hist_ref)
    assert np.array_equal(num, scale * num_ref), (num, num_ref)
    if scale == 1:
        co = np.zeros(8, np.int32)
        hh, nn = np.ascontiguousarray(hist), np.ascontiguousarray(num)
        assert L.mlvfs_amd_stripes_solve(lib.ptr(hh), lib.ptr(nn), frame_size, lib.ptr(co)) == needed
        assert list(co) == list(coeffs)


def shard_edges(h):
    return [[0, h], [0, 1, h - 3, h]]           # whole; three uneven shards, the first a single row


@pytest.mark.parametrize("level", SC.LEVELS, ids=SC.level_id)
@pytest.mark.parametrize("name", SC.SMALL_CASES)
def test_small_case_histogram_equals_oracle(torch_cuda, oracle, name, level):
    black, white = level
    L = lib.load()
    for w in SC.WIDTHS:
        f = SC.small_case(name, w, black, white)
        want = oracle.stripes_compute(f, black, white, want_hist=True)
        if name in SC.NOTHING:
            assert int(want[3].sum()) == SC.expected_calls(name, w)
        if w == 10:
            assert not want[2].any()
        for edges in shard_edges(H):
            got = device_hist(torch_cuda, L, f, black, white, edges)
            try:
                check_against_oracle(L, got, want, w * H * 14 // 8)
            except AssertionError as e:
                raise AssertionError(f"{name} {w}x{H} black {black} white {white} shards {edges}: {e}") from None


@pytest.mark.parametrize("name", ["ratio", "flat", "threshold"])
def test_hist_dev_adds_to_what_is_there(torch_cuda, oracle, name):
    """Two calls into the same histogram and counts give exactly twice the histogram: the contract the shards rely on (LDS window,
    direct bins and the re-binned samples alike)"""
    L = lib.load()
    black, white = SC.LEVELS[0]
    f = SC.small_case(name, 266, black, white)
    want = oracle.stripes_compute(f, black, white, want_hist=True)
    for edges in shard_edges(H):
        check_against_oracle(L, device_hist(torch_cuda, L, f, black, white, edges, repeat=2), want, f.size * 14 // 8, scale=2)


# ------------------------------------------------------------------ the long geometry
@pytest.fixture(scope="module")
def long_case(torch_cuda, oracle):
    cus = torch_cuda.cuda.get_device_properties(0).multi_processor_count
    w, h = SC.long_geometry(cus)
    f = SC.long_frame(w, h)
    want = oracle.stripes_compute(f, synth.BLACK, synth.WHITE, want_hist=True)          # srand(1) + libc rand()
    next_rand = C.CDLL(None).rand()                                                     # where the reference leaves the stream
    return f, want, next_rand


@pytest.mark.parametrize("shards", [1, 2])
def test_long_geometry_histogram_equals_oracle(torch_cuda, long_case, shards):
    """k_scan_blocks beyond 2048 blocks (three passes, the last ragged), k_stripes_hist with a third round that only some workgroups
    run, sub-blocks past the last block, lanes past the last group; as two shards: a boundary inside a block of 256 groups"""
    f, want, _ = long_case
    h, w = f.shape
    cut = 1000
    assert (SC.groups_per_row(w) * cut) % SC.GROUPS_PER_BLOCK != 0
    got = device_hist(torch_cuda, lib.load(), f, synth.BLACK, synth.WHITE, [0, h] if shards == 1 else [0, cut, h])
    check_against_oracle(lib.load(), got, want, w * h * 14 // 8)


def test_long_geometry_through_the_dropin(gpu, long_case):
    f, want, next_rand = long_case
    h, w = f.shape
    libc = C.CDLL(None)
    libc.srand(1)
    corr = gpu.stripes_new_correction(b"long_geometry.MLV")
    fh = abi.make_frame_headers(w, h, black=synth.BLACK, white=synth.WHITE)
    gpu.stripes_compute_correction(C.byref(fh), corr, lib.ptr(f), 0, f.size)
    after = libc.rand()
    assert corr.contents.correction_needed == want[0]
    assert list(corr.contents.coeffficients) == list(want[1])
    assert after == next_rand
    gpu.stripes_free_corrections()


# ------------------------------------------------------------------ nothing accepted / one call accepted
@pytest.mark.parametrize("level", SC.LEVELS, ids=SC.level_id)
@pytest.mark.parametrize("name", SC.NOTHING)
def test_nothing_accepted_through_dropin_and_device_api(torch_cuda, gpu, oracle, name, level):
    """A lens-cap first frame: no histogram is solved, coefficients 2..7 stay what stripes_new_correction made them (0), and libc's
    rand() moves by two values per accepted call -- none, or two"""
    from mlvfs_amd.stream import ClipStream
    black, white = level
    libc = C.CDLL(None)
    libc.srand(1)
    stream = [libc.rand() for _ in range(4)]
    for w in (10, 18, 266):
        f = SC.nothing_frame(name, w, H, black, white)
        calls = SC.expected_calls(name, w)
        needed, coeffs = oracle.stripes_compute(f, black, white)
        assert needed == 1 and list(coeffs) == [65536, 65536, 0, 0, 0, 0, 0, 0]
        libc.srand(1)
        corr = gpu.stripes_new_correction(f"{name}_{w}_{black}_{white}.MLV".encode())
        fh = abi.make_frame_headers(w, H, black=black, white=white)
        gpu.stripes_compute_correction(C.byref(fh), corr, lib.ptr(f), 0, f.size)
        after = libc.rand()
        assert corr.contents.correction_needed == needed and list(corr.contents.coeffficients) == list(coeffs), (w, "drop-in")
        assert after == stream[2 * calls], (w, "rand() after the drop-in")
        # the device API with the private stream (rand_mode 1): the same result, the application's rand() left alone
        libc.srand(1)
        s = ClipStream(w, H, 14, black, white, device=0)
        got_needed, got_co = s.stripes_compute(torch_cuda.from_numpy(f.view(np.int16)).cuda(), rand_mode=1)
        s.close()
        after = libc.rand()
        assert got_needed == needed and list(got_co) == list(coeffs), (w, "stripes_compute_dev")
        assert after == stream[0], (w, "rand() after stripes_compute_dev")
    gpu.stripes_free_corrections()


# ------------------------------------------------------------------ refusals
def test_hist_dev_needs_count_dev_for_the_same_shard(torch_cuda, oracle):
    L = lib.load()
    w, h = 266, H
    black, white = SC.LEVELS[0]
    f = SC.small_case("ratio", w, black, white)
    frame = torch_cuda.from_numpy(f.view(np.int16)).cuda()
    other = torch_cuda.from_numpy(SC.small_case("ratio", 256, black, white).view(np.int16)).cuda()
    geom, geom256 = lib.Geom(w, h, 14, black, white, 0, 0), lib.Geom(256, h, 14, black, white, 0, 0)
    dp = lambda t: C.c_void_p(t.data_ptr())
    acc = C.c_int64(-1)
    lib.check(L.mlvfs_amd_stripes_count_dev(C.byref(geom), dp(frame), 4, 100, C.byref(acc), None))
    d_rnd = torch_cuda.from_numpy(rand_stream(L, 24 * 32 * h).view(np.int16)).cuda()
    d_hist = torch_cuda.full((8 * 65536,), 7, dtype=torch_cuda.int32, device="cuda")
    d_num = torch_cuda.full((8,), 7, dtype=torch_cuda.int32, device="cuda")

    def hist_dev(g, fr, r0, r1):
        return L.mlvfs_amd_stripes_hist_dev(C.byref(g), dp(fr), r0, r1, dp(d_rnd), 2 * acc.value, dp(d_hist), dp(d_num), None)

    def untouched():
        torch_cuda.cuda.synchronize()
        return bool((d_hist == 7).all()) and bool((d_num == 7).all())

    for g, fr, r0, r1 in ((geom, frame, 0, 100), (geom, frame, 4, 101), (geom, frame, 0, h), (geom, frame, 100, 4),
                          (geom256, other, 4, 100)):
        assert hist_dev(g, fr, r0, r1) == lib.ERR_ARG, (g.width, r0, r1)
        assert untouched(), (g.width, r0, r1)
    # count_dev refuses rows outside the frame or in the wrong order, and what it counted before stays in force
    for r0, r1 in ((100, 4), (0, h + 1), (-1, 4), (h, h + 1)):
        bad = C.c_int64(-1)
        assert L.mlvfs_amd_stripes_count_dev(C.byref(geom), dp(frame), r0, r1, C.byref(bad), None) == lib.ERR_ARG, (r0, r1)
        assert hist_dev(geom, frame, r0, r1) == lib.ERR_ARG and untouched(), (r0, r1)
    # the counted shard itself is served, into what is there
    lib.check(hist_dev(geom, frame, 4, 100), "hist_dev")
    torch_cuda.cuda.synchronize()
    n, hist_ref, num_ref = oracle.stripes_hist_rows(f, 4, 100, black, white, rand_stream(L, 24 * 32 * h)[:2 * acc.value + 2])
    assert n == acc.value
    got = d_hist.cpu().numpy().reshape(8, 65536) - 7
    assert np.array_equal(got, hist_ref.reshape(8, 65536)), differences(got, hist_ref.reshape(8, 65536))
    assert np.array_equal(d_num.cpu().numpy() - 7, num_ref)
    # an empty shard is no error
    empty = C.c_int64(-1)
    lib.check(L.mlvfs_amd_stripes_count_dev(C.byref(geom), dp(frame), 50, 50, C.byref(empty), None))
    assert empty.value == 0

"""The two selection networks of k_frame_p5's pair step (csrc/median_nets.h: mlv_sort4, mlv_insert4) through the library's host hook
(mlvfs_amd_test_median_net), without a GPU: every 0/1 input -- which, the networks being min / max only, proves them for all inputs --
and 10 000 random pairs of 16-bit values, each half of a pair a set of its own as in the kernel's packed lanes, against sorted()."""
import itertools

import numpy as np

from mlvfs_amd import lib


def run(amd, net, sets):
    n_in, n_out = (4, 4) if net == 4 else (5, 5)
    a = np.ascontiguousarray(sets, np.int32).reshape(-1, n_in)
    out = np.zeros((len(a), n_out), np.int32)
    assert amd.mlvfs_amd_test_median_net(net, len(a), lib.ptr(a), lib.ptr(out)) == 0
    return out.tolist()


def test_sort4_all_zero_one_inputs(amd):
    sets = list(itertools.product((0, 1), repeat=4))
    assert run(amd, 4, sets) == [sorted(s) for s in sets]


def test_insert4_all_zero_one_inputs(amd):
    """every sorted 0/1 four and either value to insert"""
    sets = [[0] * z + [1] * (4 - z) + [x] for z in range(5) for x in (0, 1)]
    assert run(amd, 5, sets) == [sorted(s) for s in sets]


def test_random_int16_pairs(amd):
    rng = np.random.default_rng(4)
    pairs = rng.integers(-32768, 32768, (10000, 5, 2))               # five values, two 16-bit halves each
    pairs[::7, 1] = pairs[::7, 0]                                     # ties
    pairs[::11, 4] = pairs[::11, 2]
    pairs[0, :, 0], pairs[1, :, 1] = -32768, 32767
    for half in (0, 1):
        v = pairs[:, :, half]
        got4 = run(amd, 4, v[:, :4])
        assert got4 == [sorted(s) for s in v[:, :4].tolist()]
        sets = np.concatenate([np.array(got4), v[:, 4:]], 1)
        assert run(amd, 5, sets) == [sorted(s) for s in v.tolist()]


def test_hook_refuses_what_it_does_not_know(amd):
    a = np.zeros(5, np.int32)
    assert amd.mlvfs_amd_test_median_net(3, 1, lib.ptr(a), lib.ptr(a)) == lib.ERR_ARG
    assert amd.mlvfs_amd_test_median_net(4, 1, None, lib.ptr(a)) == lib.ERR_ARG

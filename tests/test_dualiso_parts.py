"""How an AMaZE dual-ISO batch goes out in parts (csrc/dualiso.cpp: dualiso_parts; host logic, no GPU): from 8 frames on, a second
stream takes everything behind each part's AMaZE; a part holds about four rounds of k_amaze_rows' workgroups (or MLVFS_AMD_DI_PART
frames), and the last part is 3/4 of an even share.  The GPU tests pass whichever way a batch is cut, so the cut is pinned here.
(Not in the sanitizer build's suites: the tile extent it asks for lives in a kernel file, a stub there.)"""
import ctypes as C

import pytest

from mlvfs_amd import lib
from test_amaze_rows_extent import restated


@pytest.fixture
def parts(monkeypatch):
    amd = lib.load()

    def run(w, h, nframes, part=None):
        if part is None:
            monkeypatch.delenv("MLVFS_AMD_DI_PART", raising=False)
        else:
            monkeypatch.setenv("MLVFS_AMD_DI_PART", str(part))
        out, tail = (C.c_int * 128)(), C.c_int(-1)
        n = amd.mlvfs_amd_test_dualiso_parts(w, h, nframes, out, 64, C.byref(tail))
        assert n > 0, (w, h, nframes, part, n)
        return [(out[2 * k], out[2 * k + 1]) for k in range(n)], bool(tail.value)
    return run


def parent_rule(w, h, nframes, part_env=None):
    """The rule as cr2hdr20_batch wrote it inline before it was one function."""
    if nframes < 8:
        return [(0, nframes)], False
    fx, fy = restated(w, h)
    per_frame = fx * fy if fx * fy > 0 else 1
    part = part_env if part_env else max(4, (1024 + per_frame - 1) // per_frame)
    nparts = nframes // part if nframes // part > 1 else 1
    if nparts == 1:
        return [(0, nframes)], True
    last = max(1, (3 * (nframes // nparts) + 2) // 4)
    front = nframes - last
    out = []
    for k in range(nparts - 1):
        f0 = front * k // (nparts - 1)
        out.append((f0, front * (k + 1) // (nparts - 1) - f0))
    return out + [(front, last)], True


def test_pinned_cuts(parts):
    assert parts(3584, 1320, 8) == ([(0, 5), (5, 3)], True)
    assert parts(3584, 1320, 9) == ([(0, 6), (6, 3)], True)
    assert parts(3584, 1320, 16) == ([(0, 4), (4, 4), (8, 5), (13, 3)], True)
    assert parts(1736, 976, 8) == ([(0, 8)], True)                  # one part, yet the tail stream
    for n in range(1, 8):
        assert parts(3584, 1320, n) == ([(0, n)], False)
        assert parts(1736, 976, n) == ([(0, n)], False)
    assert [k for _, k in parts(3584, 1320, 9, part=2)[0]] == [2, 2, 3, 2]


def test_cuts_match_the_parent_rule(parts):
    geoms = [(w, h) for w in (36, 160, 300, 688, 1332, 1736, 1920, 2592, 3584, 4096, 5796) for h in (37, 160, 304, 540, 789, 976, 1080, 1320, 2160)]
    for w, h in geoms:
        for n in range(1, 41):
            for part in (None, 1, 2, 3, 5):
                got = parts(w, h, n, part)
                assert got == parent_rule(w, h, n, part), (w, h, n, part)
                assert sum(k for _, k in got[0]) == n and all(k > 0 for _, k in got[0])
                assert all(a + k == b for (a, k), (b, _) in zip(got[0], got[0][1:])) and got[0][0][0] == 0

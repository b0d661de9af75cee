"""The LJ92 encoder's seam cases (tests/lj92_encode_cases.py) on the CPU: for every case the numpy model of the kernels' block
offsets, the oracle's stream, the reference's own encoder (where its room holds the stream) and the reference's decoder agree; and
every class of cases reaches what tests/test_gpu_lj92_encode_seams.py relies on it to reach.  Every condition is a count against a
fixed threshold -- a phase is met, a chunk of BLOCK 0xFF bytes is there -- computed with the block size the library reports
(mlvfs_amd_test_lj92_encode_plan), not with a literal: whoever retunes LJE_BLOCK sees these fail instead of seams silently unmet.

THE REFERENCE'S DECODER AND SHORT LAST ROWS: lj92.c:442, 456, 480 give up (LJ92_ERROR_CORRUPT) when the read position has reached the
end of the data while pixels are still to come, and the bit reader runs a byte or more ahead of the pixel it hands out.  A stream
whose last rows take less than that -- a constant frame a few pixels wide, a single row -- is refused although every bit is there;
with a byte of slack behind EOI, as a payload in a file has it, the same decoder gives the image back.  decoded() does just that, and
only frames narrower than 32 pixels or of one row may need it."""
import ctypes as C

import numpy as np
import pytest

import lj92_encode_cases as ec
from lossless_cases import max_class
from mlvfs_amd import lib

BLOCK = ec.BLOCK
ALL = ec.CASES + ec.MIXED + ec.ROOM
_facts = {}


def decoded(reference, c, stream):
    st, back = reference.lj92_decode(stream)
    if st != 0:
        assert c.w < 32 or c.h == 1, c.name
        st, back = reference.lj92_decode(stream + bytes(4))
    return st, back


def checked(c, oracle, reference):
    """(model, facts) of a case, after the model, the oracle, the reference's encoder and its decoder were found to agree on it"""
    if c not in _facts:
        img = ec.image(c)
        m = ec.model(img, c.bits, oracle)
        s = ec.want(c, oracle, reference)                  # oracle == the reference's encoder where its room holds the stream
        assert m.refused == c.refused, c.name
        if c.refused:
            assert s is None, c.name                        # the oracle refuses it too
            _facts[c] = (m, None)
        else:
            assert s is not None, c.name
            assert m.head_len == 36 + sum(s[20:36]) + 10 and s[m.head_len - 10:m.head_len - 8] == b"\xff\xda", c.name
            un = ec.unstuff(s, m.head_len)
            assert un.size == m.data.size == (int(m.off[-1]) + 7) // 8, (c.name, un.size, m.data.size)      # unstuffed bytes
            assert len(s) - m.head_len - 2 - un.size == m.stuffed and len(s) == m.length, c.name           # stuffed zeros
            assert np.array_equal(un, m.data), c.name
            assert max_class(s) == max(k for k in range(17) if m.hist[k]), c.name
            st, back = decoded(reference, c, s)
            assert st == 0 and np.array_equal(back, img), c.name
            _facts[c] = (m, ec.facts(m))
    return _facts[c]


def test_encode_plan_hook_is_declared_and_refuses_nonsense(amd):
    assert "mlvfs_amd_test_lj92_encode_plan" in lib.DEVICE_SYMBOLS
    out = (C.c_longlong * 4)(-7, -7, -7, -7)
    for npix in (0, -1, 1 << 27, 1 << 40):
        assert amd.mlvfs_amd_test_lj92_encode_plan(npix, out) == lib.ERR_ARG and list(out) == [-7] * 4
    assert amd.mlvfs_amd_test_lj92_encode_plan(1, None) == lib.ERR_ARG
    assert BLOCK == 256 * ec.PER_THREAD                     # a workgroup of k_lje_hist / k_lje_emit / k_lje_stuff, 16 pixels a thread
    threads = ec.plan(1)["threads"]
    assert threads % 64 == 0
    for npix, nb in ((1, 1), (BLOCK, 1), (BLOCK + 1, 2), (BLOCK * threads, threads), (BLOCK * threads + 1, threads + 1), ((1 << 27) - 1, (1 << 27) // BLOCK)):
        p = ec.plan(npix)
        assert p == dict(block=BLOCK, blocks=nb, threads=threads, per=-(-nb // threads)), npix


@pytest.mark.parametrize("cls", ["phase", "deep", "narrow", "blocks", "mixed", "room"])
def test_model_oracle_and_reference_agree_on_every_case(oracle, reference, cls):
    cases = [c for c in ALL if c.cls == cls]
    assert cases and len({c.name for c in ALL}) == len(ALL)
    for c in cases:
        m, f = checked(c, oracle, reference)
        if f is not None:
            assert f.nb == ec.plan(c.w * c.h)["blocks"] and f.nb >= 3, c.name
            assert f.lds_high <= 2 * BLOCK + 8, (c.name, f.lds_high)          # ldw of k_lje_stuff: 2 * LJE_BLOCK / 4 + 2 dwords
            assert f.double_count == 0, c.name


def test_phase_cases_meet_every_phase_with_a_0xff_byte_across_the_seam(oracle, reference):
    fs = {c: checked(c, oracle, reference)[1] for c in ec.PHASE}
    for c, f in fs.items():
        assert f.nb == 4 and 1 <= c.w * c.h - 3 * BLOCK <= 7 and len(f.seam_phases) == 1, c.name        # three seams, one phase
    assert set().union(*(f.seam_phases for f in fs.values())) == set(range(8))
    assert set().union(*(f.ff_phases for f in fs.values())) == set(range(1, 8))
    assert {c.w * c.h - 3 * BLOCK for c in fs} == {1, 2, 3, 4, 5, 6, 7}
    inside = [c for c, f in fs.items() if f.last_inside]
    assert inside and all(fs[c].last_one_dword for c in inside)
    assert {min(fs[c].seam_phases) for c in inside} >= {1, 2}
    assert sum(f.last_straddles for f in fs.values()) >= 5
    assert {c.bits for c in fs} == {14, 16}
    assert all(checked(c, oracle, reference)[0].len0 == (2 if c.arg else 1) for c in fs)


def test_deep_cases_reach_the_longest_codes_and_the_fullest_lds(oracle, reference):
    got = {c: checked(c, oracle, reference) for c in ec.DEEP}
    assert {m.len0 for c, (m, f) in got.items() if c.bits == 14} >= {8, 11, 15}
    assert {m.len0 for c, (m, f) in got.items() if c.bits == 16} == {16}
    assert any(BLOCK < f.block_bytes <= 2 * BLOCK for m, f in got.values())            # two trips of k_lje_stuff's chunk loop
    assert any(f.block_bytes > 2 * BLOCK for m, f in got.values())                     # three
    assert any((3, BLOCK, BLOCK) in f.chunks for m, f in got.values())                 # BLOCK bytes, all 0xFF, behind three lead bytes
    assert max(f.lds_high for m, f in got.values()) == 3 + 2 * BLOCK
    assert {lead for m, f in got.values() for lead, n, ff in f.chunks if n == ff == BLOCK} >= {0, 2, 3}
    assert any(m.length > c.w * c.h * 3 + 200 for c, (m, f) in got.items())            # past the reference encoder's own room
    assert any(m.length <= c.w * c.h * 3 + 200 for c, (m, f) in got.items())
    for c, (m, f) in got.items():
        assert f.nb >= 3 and f.ff_phases, c.name                                       # and a 0xFF byte across a seam in each


def test_narrow_cases_wrap_rows_at_the_seams(oracle, reference):
    got = {c: checked(c, oracle, reference) for c in ec.NARROW}
    assert {c.w for c in got} == {1, 3, 15, 17, BLOCK - 1, BLOCK + 1}
    for w in ec.NARROW_WIDTHS:
        assert {c.kind for c in got if c.w == w} == {"const", "stairs"}
        assert w % 2 == 1 and (w * 2) % 16                                              # no row but the first on a 16-byte edge
    wraps = {c.w: set().union(*(ec.seam_wraps(d) for d in got if d.w == c.w)) for c in got}
    assert 15 in wraps[1] and max(wraps[3]) >= 5 and {1, 2} & wraps[15] and wraps[17] >= {0, 1} and 0 in wraps[BLOCK - 1] and 1 in wraps[BLOCK + 1]
    every = set().union(*wraps.values())
    assert 0 in every and 1 in every and any(v >= 2 for v in every)
    assert all(m.len0 >= 8 for c, (m, f) in got.items() if c.kind == "stairs")
    assert any((3, BLOCK, BLOCK) in f.chunks for m, f in got.values())
    assert {16} <= {c.bits for c in got}


def test_blocks_cases_reach_every_shape_of_the_scan_kernels_loops(oracle, reference, amd):
    threads = ec.plan(1)["threads"]
    seen = {}
    for c in ec.BLOCKS:
        p = ec.plan(c.w * c.h)
        full = (c.w * c.h) % BLOCK == 0
        busy = -(-p["blocks"] // p["per"])                                              # threads of the scan with a block to sum
        seen.setdefault((p["blocks"], p["per"], busy), set()).add((full, c.kind))
    assert set(seen) == {(threads - 1, 1, threads - 1), (threads, 1, threads), (threads + 1, 2, threads // 2 + 1), (2 * threads + 1, 3, -(-(2 * threads + 1) // 3))}
    for key, kinds in seen.items():
        assert {f for f, _ in kinds} == {True, False} and {k for _, k in kinds} == {"two", "sparse"}, key
    for c in ec.BLOCKS:                                                                 # every phase at some seam, 0xFF bytes across seams
        f = checked(c, oracle, reference)[1]
        assert f.seam_phases == set(range(8)) and f.ff_phases, c.name


def test_mixed_batch_and_room_are_what_they_say(oracle, reference):
    got = [checked(c, oracle, reference) for c in ec.MIXED]
    assert len(ec.MIXED) == 8 and len({(c.w, c.h, c.bits) for c in ec.MIXED}) == 1
    assert [c.refused for c in ec.MIXED] == [None, "diff17", None, None, "table", None, None, None]
    assert got[1][0].hist[17] > 0 and all(got[4][0].hist[:17] > 0)                      # 17-bit differences; all 17 classes
    lengths = [0 if m.refused else m.length for m, f in got]
    room = ec.mixed_room(lengths)
    assert room % 4 == 0 and room >= 128
    assert [k for k, n in enumerate(lengths) if n > room] == [ec.MIXED_NOFIT]
    good = [m for m, f in got if not m.refused]
    assert len({m.len0 for m in good}) >= 4 and len({int(m.off[-1]) for m in good}) == len(good)      # tables and bit counts differ
    # room: L is a multiple of 4, the neighbour fits L - 4 as well
    (m0, f0), (m1, f1) = (checked(c, oracle, reference) for c in ec.ROOM)
    assert m0.length % 4 == 0 and m0.length - 4 >= 128 and m1.length <= m0.length - 4

"""The LJ92 shape cases (tests/lj92_shape_cases.py) on the CPU: the reference's decoder, the oracle and the source image agree on every
stream; the LDS of k_lj_rows, as the library's own rule cuts it (csrc/lj92.h: lj_row_plan through mlvfs_amd_test_lj92_row_plan), holds
every staged row inside the launch's allocation; and the case list reaches what tests/test_gpu_lj92_shapes.py is there to reach."""
import ctypes as C

import numpy as np

import lj92_shape_cases as sc
from mlvfs_amd import lib
from oracle import lj92_testenc as enc

LJ_WAVE_MAX_H = 8192                 # csrc/lj92.h
WIDEST = 65535                       # what a stream's header can say


def test_reference_oracle_and_image_agree_on_every_stream(oracle, reference):
    n = 0
    for case in sc.CASES:
        for f in case.frames:
            img = sc.image(f)
            kinds = [sc.stream(f, reference)]
            if f.pred == 6 and f.bits == 14 and not f.ramp:
                kinds.append(sc.stream(f))                     # the test encoder's stream as well as the reference encoder's
            for s in kinds:
                st_r, dr = reference.lj92_decode(s)
                st_o, do = oracle.lj92_decode(s)
                assert st_r == 0 and st_o == 0, (case.name, f, st_r, st_o)
                assert dr.shape == do.shape == (f.h, f.w), (case.name, f)
                assert np.array_equal(dr, do) and np.array_equal(do, img), (case.name, f)
                assert oracle.lj92_info(s)["predictor"] == f.pred
                n += 1
            if case.video is not None:
                assert case.video[0] % 2 == 0 and case.video[1] % 2 == 0 and case.video[0] * case.video[1] == f.h * f.w, (case.name, f)
    assert n > 150


def test_single_row_predictor_6_the_reference_refuses_and_the_oracle_decodes(oracle, reference):
    """lj92.c:442, 456: the predictor-6 loop reports the stream corrupt when the read position has reached the end of the data behind
    the first row -- where a one-row image ends.  Pinned on both sides: whoever changes either learns that the single-row case of
    lj92_shape_cases.py can take predictor 6 in (or must not)."""
    f = sc.REF_REFUSES
    assert (f.h, f.pred) == (1, 6) and not any(g.pred == 6 for c in sc.CASES for g in c.frames if g.h == 1)
    s = sc.stream(f)
    st_r, _ = reference.lj92_decode(s)
    st_o, do = oracle.lj92_decode(s)
    assert st_r != 0
    assert st_o == 0 and np.array_equal(do, sc.image(f))


def test_refused_predictor_7_height_is_a_valid_stream(oracle, reference, amd):
    """8193 rows with predictor 7: the stream itself is fine (reference and oracle decode it), one row more than the library takes"""
    from mlvfs_amd import lj92
    f = sc.REFUSED_P7
    assert f.pred == 7 and f.h == LJ_WAVE_MAX_H + 1
    s = sc.stream(f)
    st_r, dr = reference.lj92_decode(s)
    st_o, do = oracle.lj92_decode(s)
    assert st_r == st_o == 0 and np.array_equal(dr, do) and np.array_equal(do, sc.image(f))
    assert lj92.info(s) == dict(width=2, height=LJ_WAVE_MAX_H + 1, bits=14, predictor=7)
    assert any(g.pred == 7 and g.h == LJ_WAVE_MAX_H for c in sc.CASES for g in c.frames)


# ------------------------------------------------------------------ the LDS of k_lj_rows
def check_row_in_lds(w, max_w):
    p = sc.row_plan(w, max_w)
    carries = ((max_w + 31) // 32 + 1) * 8                  # carry[0 .. nblk] of the widest row: k_lj_rows writes carry[b + 1], b < nblk
    assert 0 < p["lds_bytes"] <= 64 * 1024, (w, max_w, p)
    assert p["stage_off"] >= carries and p["stage_off"] % 8 == 0 and p["stage_off"] <= p["lds_bytes"], (w, max_w, p)
    if p["staged"]:
        # value i of a staged row lies at word i + (i >> 5): the row's last value must lie inside the launch's bytes
        assert p["stage_end"] - p["stage_off"] >= 4 * ((w - 1) + ((w - 1) >> 5) + 1), (w, max_w, p)
        assert p["stage_off"] < p["stage_end"] <= p["lds_bytes"], (w, max_w, p)
    else:
        assert p["stage_end"] == p["stage_off"], (w, max_w, p)
    return p


def test_row_plan_hook_is_declared_and_refuses_nonsense(amd):
    assert "mlvfs_amd_test_lj92_row_plan" in lib.DEVICE_SYMBOLS
    out = (C.c_longlong * 4)(-7, -7, -7, -7)
    for w, max_w in ((0, 8), (9, 8), (1, 65536), (-1, -1)):
        assert amd.mlvfs_amd_test_lj92_row_plan(w, max_w, out) == lib.ERR_ARG and list(out) == [-7] * 4
    assert amd.mlvfs_amd_test_lj92_row_plan(8, 8, None) == lib.ERR_ARG
    assert amd.mlvfs_amd_test_lj92_row_plan(8, 8, out) == 0 and out[0] == 1


def test_staged_rows_of_the_cases_lie_inside_the_launch_lds(amd):
    pairs = sorted({pair for case in sc.CASES for pair in sc.calls(case)})
    assert (512, 9216) in pairs and (9216, 9216) in pairs
    for w, max_w in [(512, 9216)] + pairs:                  # (first the pair that sizing the LDS by `max_w <= 8192` alone got wrong)
        check_row_in_lds(w, max_w)
    # a narrow frame keeps its fast path beside a wide one
    assert sc.row_plan(512, 9216)["staged"] and not sc.row_plan(9216, 9216)["staged"]


def test_staged_rows_lie_inside_the_launch_lds_for_any_pair(amd):
    rng = np.random.default_rng(92)
    edge = [1, 2, 31, 32, 33, 8191, 8192, 8193, 8194, 9216, 65534, WIDEST]
    pairs = {(w, m) for w in edge for m in edge if w <= m}
    for _ in range(600):
        m = int(rng.integers(1, WIDEST + 1))
        pairs.add((int(rng.integers(1, m + 1)), m))
        m = int(rng.integers(8192, WIDEST + 1))              # a staged row beside a row that is not
        pairs.add((int(rng.integers(1, 8193)), m))
    for w in (8191, 8192, 8193):
        for m in (8191, 8192, 8193):
            assert w > m or (w, m) in pairs
    assert {(1, 1), (1, WIDEST), (WIDEST, WIDEST)} <= pairs
    for w, m in sorted(pairs):
        p = check_row_in_lds(w, m)
        assert p["staged"] == (w <= 8192), (w, m)           # the rule: a frame's own width decides, not its neighbours'
        assert p["lds_bytes"] == sc.row_plan(m, m)["lds_bytes"] and p["stage_off"] == sc.row_plan(m, m)["stage_off"]     # one launch, one layout
    assert sc.row_plan(WIDEST, WIDEST)["lds_bytes"] <= 52 * 1024          # the old static array's size: 2050 carries + 8450 ints


# ------------------------------------------------------------------ the list reaches what it is there for
def test_cases_are_not_vacuous(amd):
    frames = [(c, f) for c in sc.CASES for f in c.frames]
    plan = lambda c, f: sc.row_plan(f.w, max(g.w for g in c.frames))
    for p in range(8):
        assert any(f.pred == p and not plan(c, f)["staged"] for c, f in frames), f"no row worked on in place with predictor {p}"
        assert any(f.pred == p and plan(c, f)["staged"] for c, f in frames), f"no staged row with predictor {p}"
    unstaged = [f for c, f in frames if not plan(c, f)["staged"]]
    assert any(sc.blocks(f.w) == 257 and sc.trips(f.w) == 2 and f.w % 2 == 0 for f in unstaged)       # one block on the second trip
    assert any(sc.blocks(f.w) >= 2048 and sc.trips(f.w) >= 8 for f in unstaged)
    assert all(sc.trips(f.w) == 1 for c, f in frames if plan(c, f)["staged"])
    # the widest staged row: 8192 values staged, 8193 not (asked of the hook, not assumed)
    assert sc.row_plan(8192, 8192)["staged"] and not sc.row_plan(8193, 8193)["staged"]
    assert any(f.w == 8192 and plan(c, f)["staged"] for c, f in frames)
    # mixed batches: the narrowest frame staged, the widest not, in both orders
    orders = set()
    for c in sc.CASES:
        ws = [f.w for f in c.frames]
        lo, hi = min(ws), max(ws)
        if lo != hi and sc.row_plan(lo, hi)["staged"] and not sc.row_plan(hi, hi)["staged"]:
            orders.add(ws.index(lo) < ws.index(hi))
            assert all(f.h * f.w == c.video[0] * c.video[1] for f in c.frames)
    assert orders == {True, False}
    assert any(len(c.frames) > 8 and len({f.w for f in c.frames}) >= 4 and len({f.pred for f in c.frames}) >= 5 for c in sc.CASES)
    # 16-bit samples with predictors 4..7, staged and in place; block edges; one row; one column; the predictor-7 limit
    for p in (4, 5, 6, 7):
        assert {plan(c, f)["staged"] for c, f in frames if f.bits == 16 and f.pred == p} == {True, False}
    edge = {f.w for c, f in frames if c.video is None and f.h == 6 and f.pred == 6}
    assert {1, 2, 3, 31, 32, 33, 34, 63, 64, 65, 66} <= edge
    assert any(f.w == 1 and f.h > 16 for c, f in frames) and any(f.h == 1 for c, f in frames)
    assert any(f.pred == 7 and f.h == LJ_WAVE_MAX_H for c, f in frames)
    assert any(f.ramp and not plan(c, f)["staged"] for c, f in frames)
    assert len({c.name for c in sc.CASES}) == len(sc.CASES)
    for c in sc.CASES:
        assert sc.describe(c).startswith(c.name)

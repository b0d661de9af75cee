"""The C-ABI library loads and exports every symbol include/mlvfs_amd.h declares; the
host-only entry points work without a GPU (no compute calls here)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np

from mlvfs_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_facts():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "reference_facts.json")))


def declared_functions():
    text = open(os.path.join(ROOT, "include", "mlvfs_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b([a-z_][a-z0-9_]*)\s*\(", text))
    return {n for n in names if n not in {"defined", "sizeof"}}


def test_every_declared_symbol_is_exported(amd):
    declared = declared_functions() - {"get_raw2ev", "get_ev2raw"}      # imported (weak) from the caller
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert declared <= exported, sorted(declared - exported)
    assert set(lib.DROPIN_SYMBOLS + lib.DEVICE_SYMBOLS) == declared
    und = subprocess.run(["nm", "-D", "--undefined-only", lib.SO_PATH], capture_output=True, text=True).stdout
    weak = {l.split()[-1] for l in und.splitlines() if " w " in l}
    assert {"get_raw2ev", "get_ev2raw"} <= weak


def test_nothing_else_is_exported(amd):
    """The export table is closed (mlvfs_amd/csrc/exports.map): the symbols of the MLVFS objects the library replaces and its own
    mlvfs_amd_* entry points, no C++ of namespace mlv, no file-scope globals (`t_pipe`, `_ZN3mlv...`)."""
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    declared = declared_functions() - {"get_raw2ev", "get_ev2raw"}
    stray = sorted(s for s in defined if s not in declared)
    assert not stray, stray[:20]
    assert all(s.startswith("mlvfs_amd_") or s in lib.DROPIN_SYMBOLS for s in defined)


def test_no_oracle_or_reference_linkage(amd):
    """The product must not route through the checkers."""
    deps = subprocess.run(["ldd", lib.SO_PATH], capture_output=True, text=True).stdout
    assert "liboracle" not in deps and "libmlvfs_ref" not in deps
    for dirpath, _, files in os.walk(os.path.join(ROOT, "mlvfs_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("oracle-", ""), os.path.join(dirpath, f)


def test_host_selftest(amd):
    assert amd.mlvfs_amd_selftest_host() == 0


def test_size_helpers(amd):
    from mlvfs_amd import abi
    fh = abi.make_frame_headers(3584, 1320)
    assert amd.dng_get_header_size() == 65536                        # dng.c:797-800
    assert amd.dng_get_image_size(C.byref(fh)) == 3584 * 1320 * 2
    assert amd.dng_get_size(C.byref(fh)) == 65536 + 3584 * 1320 * 2


def test_rand_stream_is_glibc(amd):
    libc = C.CDLL(None)
    libc.srand(1)
    want = np.array([libc.rand() % 1024 for _ in range(5000)], np.uint16)
    got = np.zeros(5000, np.uint16)
    amd.mlvfs_amd_rand_stream(lib.ptr(got), 5000, 0, 1)
    assert np.array_equal(got, want)
    part = np.zeros(100, np.uint16)
    amd.mlvfs_amd_rand_stream(lib.ptr(part), 100, 3210, 1)
    assert np.array_equal(part, want[3210:3310])


def test_libc_rand_state_layout_is_recognised_and_the_applications_stream_untouched(amd):
    """stripes_compute_correction takes its dither from the application's rand() stream in bulk (runtime.cpp: take_app_state): that
    rests on glibc's TYPE_3 state layout, which the library checks once on a generator of its own.  Host code: no device needed."""
    import ctypes as C
    libc = C.CDLL(None)
    libc.srand(77)
    want = [libc.rand() for _ in range(50)]
    libc.srand(77)
    head = [libc.rand() for _ in range(7)]
    amd.mlvfs_amd_test_rand_layout.restype = C.c_int
    assert amd.mlvfs_amd_test_rand_layout() == 1          # glibc here; 0 would mean the call-by-call path (still correct, 300 ms)
    assert amd.mlvfs_amd_test_rand_layout() == 1
    assert head + [libc.rand() for _ in range(43)] == want


def test_stripes_solve_matches_oracle(amd, oracle):
    from mlvfs_amd import synth
    f = synth.normal_frame(256, 130)
    needed, co, hist, num = oracle.stripes_compute(f, synth.BLACK, synth.WHITE, want_hist=True)
    got = np.zeros(8, np.int32)
    h = np.ascontiguousarray(hist.reshape(-1))
    assert amd.mlvfs_amd_stripes_solve(lib.ptr(h), lib.ptr(num), 256 * 130 * 14 // 8, lib.ptr(got)) == needed
    assert list(got) == list(co)


def test_histogram_helpers(amd):
    data = np.full(70000, 100, np.uint16)
    data[:3000] = 50
    h = amd.hist_create(1000)
    amd.hist_add(h, lib.ptr(data), data.size, 0)
    # 16-bit counters wrap (histogram.h:30): bin 100 holds 67000 % 65536 = 1464, the running sum
    # never exceeds count/2 and the reference's loop falls through to 0 (histogram.c:74)
    assert amd.hist_median(h) == 0
    small = np.array([5, 7, 7, 9, 1000, 2000], np.uint16)
    h2 = amd.hist_create(1000)
    amd.hist_add(h2, lib.ptr(small), small.size, 0)
    assert amd.hist_median(h2) == 9                                  # first bin whose running sum exceeds count/2
    amd.hist_destroy(h2)
    amd.hist_destroy(h)


def test_stripes_correction_list(amd):
    a = amd.stripes_new_correction(b"/x/a.MLV")
    b = amd.stripes_new_correction(b"/x/b.MLV")
    assert a and b and amd.stripes_get_correction(b"/x/b.MLV").contents.mlv_filename == b"/x/b.MLV"
    assert not amd.stripes_get_correction(b"/x/c.MLV")
    assert a.contents.correction_needed == 0 and list(a.contents.coeffficients) == [0] * 8
    amd.stripes_free_corrections()
    assert not amd.stripes_get_correction(b"/x/a.MLV")


def test_library_covers_what_the_callers_import_from_the_replaced_objects(amd):
    """Link-level drop-in: every global function of the objects the library replaces (mlvfs/Makefile:24,34-38)
    that the rest of MLVFS calls -- main.c, gif.c, webgui.c, resource_manager.c, ... -- must be exported by libmlvfs_amd.so.
    main.c itself cannot be compiled (<fuse.h>), so its calls are found in its text; the set is recorded from the reference tree by
    tests/golden/make_reference_facts.py."""
    needed = set(reference_facts()["called_from_callers"])
    assert {"dng_get_header_data", "dng_get_image_data", "chroma_smooth", "stripes_compute_correction", "cr2hdr20_convert_data",
            "hdr_convert_data", "fix_pattern_noise", "hist_median"} <= needed
    out = subprocess.run(["nm", "-D", "--defined-only", lib.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert needed <= exported, sorted(needed - exported)


def test_wrap_shim_links_and_brackets_process_frame_only(amd, tmp_path):
    """integration/mlvfs_amd_wrap.c: a host that calls mlvfs_load_chunks / mlvfs_close_chunks from one
    object and defines them in another (like main.o / resource_manager.o) links with the two --wrap flags, its calls then go
    through the shim and the shim's through to the host's definitions.  No compute: the bracket calls do not touch a GPU.  And
    in the reference: the pixel stages of process_frame sit between the two wrapped calls (main.c:923-998),
    gif.c's do not (it uses index.c's load_chunks / close_chunks): recorded by tests/golden/make_reference_facts.py."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = tmp_path / "host.c"
    host.write_text('#include <stdint.h>\n#include <stdio.h>\n'
                    'FILE **mlvfs_load_chunks(const char *path, uint32_t *chunk_count);\n'
                    'void mlvfs_close_chunks(FILE **chunk_files, uint32_t chunk_count);\n'
                    'int main(int argc, char **argv) { uint32_t n = 0; FILE **c = mlvfs_load_chunks(argv[0], &n);\n'
                    '  if (!c || n != 1) return 1; mlvfs_close_chunks(c, n); puts("closed"); return 0; }\n')
    exe = tmp_path / "host"
    so_dir = os.path.dirname(lib.SO_PATH)
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(root, "include"), str(host), os.path.join(root, "tests", "c_host_chunks.c"),
                    os.path.join(root, "integration", "mlvfs_amd_wrap.c"), "-Wl,--wrap=mlvfs_load_chunks", "-Wl,--wrap=mlvfs_close_chunks",
                    "-o", str(exe), "-L", so_dir, "-lmlvfs_amd", "-Wl,-rpath," + so_dir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"], check=True)
    syms = subprocess.run(["nm", str(exe)], capture_output=True, text=True, check=True).stdout
    assert " T __wrap_mlvfs_load_chunks" in syms and " T __wrap_mlvfs_close_chunks" in syms and " U mlvfs_amd_frame_begin" in syms
    dis = subprocess.run(["objdump", "-d", "--no-show-raw-insn", str(exe)], capture_output=True, text=True, check=True).stdout
    main_body = dis[dis.index("<main>:"):].split("\n\n")[0]
    assert "<__wrap_mlvfs_load_chunks>" in main_body and "<__wrap_mlvfs_close_chunks>" in main_body
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)          # no GPU here: the bracket must not need one
    assert r.returncode == 0 and "closed" in r.stdout, r.stderr[-1000:]
    assert amd.mlvfs_amd_frame_begin() == 0 and amd.mlvfs_amd_frame_end() == 0 and amd.mlvfs_amd_frame_sync(None) == 0
    facts = reference_facts()
    calls = facts["process_frame_calls"]
    a, b = calls.index("mlvfs_load_chunks"), calls.index("mlvfs_close_chunks")
    for stage in ("get_image_data", "fix_pattern_noise", "cr2hdr20_convert_data", "fix_bad_pixels", "chroma_smooth", "stripes_apply_correction"):
        assert a < calls.index(stage) < b, stage
    gif_c = facts["gif_c_calls"]
    assert not gif_c["mlvfs_load_chunks"] and not gif_c["mlvfs_close_chunks"] and gif_c["load_chunks(path"]


def test_worker_threads_are_bound_round_robin_in_pci_order(amd):
    """SURVEY 8(e), VERDICT r4 next #5: the drop-in symbols' worker threads (libfuse's pool) get the node's cards round-robin in the
    order of their PCI bus ids, whatever order the runtime enumerates them in -- on a faked 8-card node, no GPU needed."""
    bus = ["0000:df:00.0", "0000:0c:00.0", "0000:9f:00.0", "0000:22:00.0", "0000:bf:00.0", "0000:38:00.0", "0000:af:00.0", "0000:5c:00.0"]
    arr = (C.c_char_p * len(bus))(*[b.encode() for b in bus])
    out = np.zeros(20, np.int32)
    assert amd.mlvfs_amd_test_device_order(C.cast(arr, C.c_void_p), len(bus), out.size, lib.ptr(out)) == 0
    by_bus = sorted(range(len(bus)), key=lambda d: bus[d])
    assert list(out[:8]) == by_bus == [1, 3, 5, 7, 2, 6, 4, 0]
    assert list(out[8:16]) == by_bus and list(out[16:20]) == by_bus[:4]          # the ninth worker shares the first card
    one = (C.c_char_p * 1)(b"0000:05:00.0")
    assert amd.mlvfs_amd_test_device_order(C.cast(one, C.c_void_p), 1, 3, lib.ptr(out)) == 0 and list(out[:3]) == [0, 0, 0]
    assert amd.mlvfs_amd_test_device_order(None, 0, 1, lib.ptr(out)) != 0


def test_fix_pattern_noise_refuses_odd_sizes_before_touching_anything(amd):
    """patternnoise.c:284-310 index its half-size planes with x/2 + (y/2)*(w/2): with an odd width the last column of every row lands
    in the next row's first slot, with an odd height the last row lies behind the malloc'ed plane (heap overflow) -- the reference has
    no defined result to match (MLVFS only passes even raw sizes).  The library reports the frame and leaves it alone; the check comes
    before any device call, so it holds without a GPU."""
    for w, h in ((65, 48), (64, 47), (33, 33), (1, 2)):
        f = (np.arange(w * h, dtype=np.int16).reshape(h, w) * 7 + 2048).astype(np.int16)
        g = f.copy()
        amd.fix_pattern_noise(lib.ptr(g), w, h, 15000, 0)
        assert np.array_equal(g, f)
        assert b"not supported" in amd.mlvfs_amd_last_error()


def test_streaming_kernels_plan():
    """Host arithmetic of the streaming kernels' launch plan (no GPU): 3584 px = 7 columns of 62 items and one of 14, which is folded
    four segments to a wave -- 7.25 columns of steps per frame instead of 8; a last column of up to 30 items folds in two."""
    amd = lib.load()
    amd.mlvfs_amd_test_stream_plan.restype = C.c_int
    def plan(w, h, seg=60):
        v = [C.c_int() for _ in range(4)]
        rc = amd.mlvfs_amd_test_stream_plan(w, h, seg, *[C.byref(x) for x in v])
        return rc, tuple(x.value for x in v)
    assert plan(3584, 1320) == (0, (8, 11, 4, 7 * 11 + 3))
    assert plan(1920, 1080) == (0, (4, 9, 1, 36))
    assert plan(512, 124, 30) == (0, (2, 3, 4, 3 + 1))           # 64 items: 62 + 2
    assert plan(656, 190, 30) == (0, (2, 4, 2, 4 + 2))           # 82 items: 62 + 20
    assert plan(3584, 66) == (0, (8, 1, 1, 8))                   # one segment: nothing to fold
    assert plan(3583, 1320)[0] != 0 and plan(3584, 1321)[0] != 0


PLAN_KEYS = ("first", "list_after", "grid", "groups", "run", "singles", "first_grid", "seg_rows", "cols", "segs", "fold", "tasks", "steps",
             "wl_entries", "word")
P_NONE, P_TILES, P_P5, P_S = 0, 1, 2, 3          # first kernel: k_frame alone, k_frame_p, k_frame_p5, k_frame_s


def test_fused_pass_plan(amd, monkeypatch):
    """Which kernels a launch of the fused pass runs and how they are laid out (csrc/frame_plan.cpp, no GPU): every GPU test passes
    whichever kernel runs, so the choice is pinned here.  The numbers are those the launcher computed before the plan was one function;
    only the work list may be larger -- k_frame_p5 can append more entries than a frame has tiles where a frame is one tile row high."""
    for v in ("MLVFS_AMD_KF_P", "MLVFS_AMD_KF_P5", "MLVFS_AMD_KF_S"):
        monkeypatch.delenv(v, raising=False)

    def plan(w=3584, h=1320, bpp=14, black=2048, cs=5, packed=1, vec=1, pmap=1, stripes=1, nframes=400, cus=256, held=0, some_listed=0, **sw):
        for k, v in sw.items():
            monkeypatch.setenv("MLVFS_AMD_KF_" + k.upper(), str(v))
        out = (C.c_longlong * 15)()
        rc = amd.mlvfs_amd_test_frame_plan((C.c_int * 13)(w, h, bpp, black, cs, packed, vec, pmap, stripes, nframes, cus, held, some_listed), out)
        for k in sw:
            monkeypatch.delenv("MLVFS_AMD_KF_" + k.upper())
        return None if rc else dict(zip(PLAN_KEYS, out))

    def pick(p, keys):
        return tuple(p[k] for k in keys.split())

    # 3584x1320 cs5x5 with a pixel map and stripes, 256 CUs: k_frame's grid, groups of eight CUs, runs of 22 tiles
    p = plan()
    assert pick(p, "grid groups run singles word") == (1024, 32, 22, 256, 0)
    # long launches: k_frame_p5 on k_frame's grid in tasks of 60 rows, at 100 frames of 30; at 50 frames k_frame_p -- and the list-mode
    # k_frame behind either.  The work list holds every tile (k_frame_p5 appends fewer: 154 000 entries at most).
    fields = "first list_after first_grid seg_rows cols segs fold tasks wl_entries"
    assert pick(p, fields) == (P_P5, 1, 1024, 60, 8, 11, 4, 400 * (7 * 11 + 3), 28 * 44 * 400)
    assert pick(plan(nframes=100), fields) == (P_P5, 1, 1024, 30, 8, 22, 4, 100 * (7 * 22 + 6), 28 * 44 * 100)
    assert pick(plan(nframes=50), fields) == (P_TILES, 1, 1024, 0, 0, 0, 0, 0, 28 * 44 * 50)
    # what k_frame_p5 does not read goes to k_frame_p: 12-bit streams, 16-bit frames, stripes beyond the packed form
    for kw in (dict(bpp=12, vec=3), dict(bpp=16, packed=0), dict(stripes=2)):
        assert pick(plan(**kw), "first list_after wl_entries") == (P_TILES, 1, 28 * 44 * 400), kw
    # the stream's verdicts: some tiles listed -> k_frame_p (unless KF_P5=2); held back -> k_frame alone (unless KF_P=2)
    assert pick(plan(some_listed=1), "first list_after") == (P_TILES, 1)
    assert pick(plan(some_listed=1, p5=2), "first seg_rows") == (P_P5, 60)
    assert pick(plan(held=1), "first list_after first_grid wl_entries word") == (P_NONE, 0, 0, 0, 0)
    assert pick(plan(held=1, p=2), "first list_after") == (P_P5, 1)
    assert pick(plan(p=0), "first list_after word") == (P_NONE, 0, -1)
    assert pick(plan(p5=0), "first") == (P_TILES,)
    # cs2x2: k_frame_s alone on long launches without a pixel map, k_frame with one; 8 frames are too short unless KF_S=2
    s_fields = "first list_after first_grid seg_rows cols segs fold tasks steps word"
    assert pick(plan(cs=2, pmap=0), s_fields) == (P_S, 0, 1024, 60, 8, 11, 4, 400 * 80, 400 * (7 * 4 + 1) * 660 // 4, 1)
    assert pick(plan(cs=2, pmap=1), s_fields) == (P_NONE, 0, 0, 0, 0, 0, 0, 0, 0, -1)
    assert pick(plan(cs=2, pmap=0, nframes=8), s_fields + " run") == (P_NONE, 0, 0, 0, 0, 0, 0, 0, 0, -1, 19)
    assert pick(plan(cs=2, pmap=0, nframes=8, s=2), s_fields) == (P_S, 0, 160, 60, 8, 11, 4, 8 * 80, 8 * 29 * 660 // 4, 1)
    assert pick(plan(cs=2, pmap=0, held=1), "first word") == (P_NONE, 1)
    assert pick(plan(cs=3, pmap=0, held=1, s=2), "first") == (P_S,)
    assert pick(plan(cs=2, pmap=0, s=0), "first word") == (P_NONE, -1)
    # k_frame_p and k_frame_p5 are cs5x5 kernels: whatever the stream's verdict and the launch, forcing the two-kernel path
    # (KF_P=2, KF_P5=2) never makes one of them the first kernel of a cs2x2 / cs3x3 launch
    for cs in (2, 3):
        for kw in (dict(), dict(pmap=0), dict(held=1), dict(some_listed=1), dict(nframes=8), dict(nframes=50, pmap=0), dict(bpp=12, vec=3),
                   dict(bpp=16, packed=0), dict(stripes=2), dict(s=0), dict(pmap=0, s=0)):
            for force in (dict(p=2), dict(p=2, p5=2)):
                p = plan(cs=cs, **kw, **force)
                assert p["first"] in (P_NONE, P_S) and p["list_after"] == 0, (cs, kw, force)
    # no chroma smoothing: k_frame alone
    assert pick(plan(cs=0), "first list_after word grid") == (P_NONE, 0, -1, 1024)
    # 112x250: one column of 14 items, its segments folded four to a wave
    assert pick(plan(w=112, h=250, cs=2, vec=2, pmap=0, s=2), s_fields) == (P_S, 0, 100, 60, 1, 3, 4, 400, 400 * 125 // 4, 1)
    assert pick(plan(w=112, h=250, vec=2, nframes=3600), fields) == (P_P5, 1, 1024, 30, 1, 5, 4, 3600 * 2, 9 * 3600)
    # 3584x30 (one tile row) forced through k_frame_p5: eight tasks of up to five tile columns each per frame, more than its 28 tiles
    p = plan(h=30, nframes=160, pmap=0, p=2, p5=2)
    assert pick(p, "first seg_rows cols segs fold tasks") == (P_P5, 30, 8, 1, 1, 160 * 8)
    assert p["wl_entries"] >= 160 * 8 * 5 > 28 * 160
    # a launch the fused pass refuses
    assert plan(w=3583) is None and plan(cs=4) is None and plan(nframes=0) is None


def test_last_frame_plan_hook_before_any_launch(amd):
    """mlvfs_amd_test_last_frame_plan hands out the plan the calling thread's last launch of the fused pass took (the GPU tests of the
    streaming kernels ask it which kernel they ran); a thread that has launched nothing gets MLVFS_AMD_ERR_ARG and its buffer back
    untouched.  Host only; exported and declared like every other entry point."""
    import threading
    assert "mlvfs_amd_test_last_frame_plan" in lib.DEVICE_SYMBOLS and "mlvfs_amd_test_last_frame_plan" in declared_functions()
    got = {}

    def fresh_thread():
        out = (C.c_longlong * 15)(*([-7] * 15))
        got["rc"] = amd.mlvfs_amd_test_last_frame_plan(out)
        got["out"] = list(out)
        got["null"] = amd.mlvfs_amd_test_last_frame_plan(None)

    t = threading.Thread(target=fresh_thread)
    t.start()
    t.join()
    assert got == {"rc": lib.ERR_ARG, "out": [-7] * 15, "null": lib.ERR_ARG}

"""The scene check's C ABI and Python binding, and the hand-checked cases of its numpy restatement (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from scene_cases import CUT, FIRST, FORMATS, GRID, HIST, SAME, RefScene, luma_of, moved_views, run_scene, scene, signature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "centerface_hip.h")).read()
SYMBOLS = ("cf_scene_create", "cf_scene_destroy", "cf_scene_forget", "cf_scene_check", "cf_op_scene")
SIZES = ((8, 8), (10, 14), (18, 22), (76, 102), (270, 482))


def test_symbols_exported_declared_and_bound():
    L = cfa._lib.lib()
    for s in SYMBOLS:
        assert s in cfa._lib.EXPORTS
        assert re.search(r"\bint %s\(" % s, HEADER), s
        assert hasattr(L, s) and getattr(L, s).argtypes, s
    assert re.search(r"typedef struct cf_scene cf_scene;", HEADER)
    for name in ("scene_sequence", "scene_signature"):
        assert callable(getattr(cfa.ops, name))
    for name in ("scene_check", "scene_check_device"):
        assert callable(getattr(cfa.Engine, name))
    for name in ("forget", "close", "_handle"):
        assert callable(getattr(cfa.SceneCuts, name))
    assert "SceneCuts" in cfa.__all__


def test_scene_opts_and_codes_agree_with_the_header():
    body = re.search(r"typedef struct cf_scene_opts \{(.*?)\} cf_scene_opts;", HEADER, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t)\s+(\w+);", body, re.M)
    assert [(n, C.c_int32) for _, n in fields] == list(cfa._lib.SceneOpts._fields_)
    assert [n for _, n in fields] == ["hist_thresh", "grid_thresh"]
    assert C.sizeof(cfa._lib.SceneOpts) == 8
    # the others kept their size
    assert C.sizeof(cfa._lib.TrackOpts) == 20 and C.sizeof(cfa._lib.FollowOpts) == 8 and C.sizeof(cfa._lib.RedactOpts) == 20
    assert C.sizeof(cfa._lib.BestShotOpts) == 16
    for name, value in (("FIRST", 0), ("SAME", 1), ("CUT", 2)):
        assert re.search(r"^#define CF_SCENE_%s\s+%d\s*$" % (name, value), HEADER, re.M), name
        assert getattr(cfa._lib, "CF_SCENE_" + name) == value
    assert (FIRST, SAME, CUT) == (0, 1, 2)
    o = cfa._lib.scene_opts()
    assert (o.hist_thresh, o.grid_thresh) == (350, 640) == (HIST, GRID)
    assert cfa._lib.lib().cf_version() == 100


def test_makefile_builds_the_kernel():
    mk = open(os.path.join(ROOT, "lightweight-face-detection-centernet_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "cf_scene.hip" in srcs


def test_the_documents_carry_the_limits_and_make_no_accuracy_claim():
    for name in ("README.md", "DESIGN.md", os.path.join("include", "centerface_hip.h")):
        text = open(os.path.join(ROOT, name)).read()
        at = text.find("cf_scene_check")
        assert at >= 0, name
        for word in ("flash", "dissolve", "no accuracy claim"):
            assert word in text[max(0, at - 6000):at + 8000], (name, word)


# ---------------------------------------------------------------------------------------------- refusals
def _op_scene(opts=(350, 640), S=2, F=2, fmt=0, h=8, w=12, pitch0=12, pitch1=12, null_opts=False, null_table=False, null_plane=None, null_out=False):
    L = cfa._lib.lib()
    o = cfa._lib.scene_opts(*opts)
    planes = [np.full((h * 3 // 2 + 2, max(w, 1) * 3), 7, np.uint8) for _ in range(max(F * S, 1))]      # room for every format's planes
    tab = (cfa._lib.PlanesRW * len(planes))()
    for k, pl in enumerate(planes):
        tab[k].p0, tab[k].p1, tab[k].p2 = pl.ctypes.data, pl.ctypes.data + 8, pl.ctypes.data + 16
    if null_plane is not None:
        setattr(tab[null_plane[0]], "p%d" % null_plane[1], None)
    out, sigs = np.full((max(F, 1), max(S, 1), 4), 9, np.int32), np.full((max(F, 1), max(S, 1), 128), 9, np.int32)
    r = L.cf_op_scene(0, None if null_opts else C.byref(o), S, F, fmt, None if null_table else tab, h, w, pitch0, pitch1,
                      None if null_out else cfa._lib.ptr(out), cfa._lib.ptr(sigs))
    assert (out == 9).all() and (sigs == 9).all()                          # refused: nothing was written
    return r, (L.cf_op_last_error() or b"").decode()


OP_REFUSALS = [(dict(opts=(-1, 640)), "hist_thresh"), (dict(opts=(1001, 640)), "hist_thresh"), (dict(opts=(350, -1)), "grid_thresh"),
               (dict(opts=(350, 16321)), "grid_thresh"), (dict(S=0), "n_streams"), (dict(S=4097), "n_streams"), (dict(F=0), "n_frames"),
               (dict(fmt=-1), "format"), (dict(fmt=5), "format"), (dict(h=6), "[8, 8192]"), (dict(h=7), "even"), (dict(w=8194, pitch0=8194), "[8, 8192]"),
               (dict(pitch0=11), "pitch0"), (dict(fmt=4, pitch0=35), "pitch0"), (dict(pitch1=11), "pitch1"), (dict(fmt=2, pitch1=5), "pitch1"),
               (dict(null_opts=True), "null options"), (dict(null_table=True), "null frame table"), (dict(null_plane=(3, 0)), "null plane"),
               (dict(fmt=1, null_plane=(1, 1)), "null plane"), (dict(fmt=2, null_plane=(2, 2)), "null plane"), (dict(fmt=3, null_plane=(0, 1)), "null plane"),
               (dict(fmt=4, pitch0=36, null_plane=(2, 0)), "null plane"), (dict(null_out=True), "null out")]


@pytest.mark.parametrize("kw, word", OP_REFUSALS, ids=[w + str(i) for i, (_, w) in enumerate(OP_REFUSALS)])
def test_cf_op_scene_refuses_before_any_device(kw, word):
    r, why = _op_scene(**kw)
    assert r == -1 and "cf_op_scene" in why and word in why, (kw, why)


def test_cf_scene_check_and_create_check_their_arguments_before_the_context():
    L = cfa._lib.lib()
    out = np.full((1, 4), 9, np.int32)
    tab = (cfa._lib.PlanesRW * 1)()
    tab[0].p0 = tab[0].p1 = tab[0].p2 = 4096

    def check(B=1, fmt=0, h=8, w=12, pitch0=12, pitch1=12, table=tab, on_device=0):
        assert L.cf_scene_check(None, None, None, 0, B, fmt, table, on_device, h, w, pitch0, pitch1, cfa._lib.ptr(out), 0) == -1
        assert (out == 9).all()
        why = L.cf_op_last_error().decode()
        assert "cf_scene_check" in why
        return why
    for kw, word in ((dict(B=0), "B must be"), (dict(fmt=-1), "format"), (dict(fmt=5), "format"), (dict(h=6), "[8, 8192]"), (dict(h=7), "even"),
                     (dict(w=8194, pitch0=8194), "[8, 8192]"), (dict(pitch0=11), "pitch0"), (dict(fmt=4, pitch0=35), "pitch0"), (dict(pitch1=11), "pitch1"),
                     (dict(table=None), "null frame table"), (dict(on_device=1, pitch0=14), "multiples of 4")):
        why = check(**kw)
        assert word in why and "null context" not in why, (kw, why)
    for fmt, k in ((0, 0), (1, 1), (2, 2), (3, 1), (4, 0)):
        t = (cfa._lib.PlanesRW * 1)()
        t[0].p0 = t[0].p1 = t[0].p2 = 4096
        setattr(t[0], "p%d" % k, None)
        assert "null plane" in check(fmt=fmt, pitch0=36 if fmt == 4 else 12, table=t)
    assert "null context" in check()
    # the options and the count of cf_scene_create
    h = C.c_void_p()
    for opts, S, word in (((-1, 640), 2, "hist_thresh"), ((1001, 640), 2, "hist_thresh"), ((350, -1), 2, "grid_thresh"), ((350, 16321), 2, "grid_thresh"),
                          ((350, 640), 0, "n_streams"), ((350, 640), 4097, "n_streams")):
        o = cfa._lib.scene_opts(*opts)
        assert L.cf_scene_create(None, S, C.byref(o), C.byref(h)) == -1 and h.value is None
        why = L.cf_op_last_error().decode()
        assert "cf_scene_create" in why and word in why and "null context" not in why, why
        with pytest.raises(ValueError):
            cfa.SceneCuts(0, S, *opts)
    assert L.cf_scene_create(None, 2, None, C.byref(h)) == -1 and "null options" in L.cf_op_last_error().decode()
    o = cfa._lib.scene_opts()
    assert L.cf_scene_create(None, 2, C.byref(o), None) == -1 and "null out" in L.cf_op_last_error().decode()
    assert L.cf_scene_create(None, 2, C.byref(o), C.byref(h)) == -1 and "null context" in L.cf_op_last_error().decode()
    assert L.cf_scene_forget(None, 0) == -1 and L.cf_scene_destroy(None) == 0
    s = cfa.SceneCuts(0, 3)                                                # no engine yet: nothing is created, the range is checked
    s.forget(2)
    s.forget()
    with pytest.raises(ValueError):
        s.forget(3)
    with pytest.raises(ValueError):
        cfa.ops.scene_sequence(np.zeros((3, 8, 12, 3), np.uint8), "bgr", 2)      # 3 frames for 2 streams


def test_scenes_needs_a_tracker():
    f = cfa.CenterFace._scene
    assert f(None, None, None, "frames", "bgr") is None and f(None, None, "tracker", "frames", "bgr") is None
    assert f(None, "scenes", "tracker", "frames", "bgr") == ("scenes", "frames", "bgr")
    with pytest.raises(ValueError):
        f(None, "scenes", None, "frames", "bgr")


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_signature_by_hand():
    luma = np.zeros((8, 8), np.int64)
    luma[0, 0], luma[7, 7], luma[3, 4] = 255, 7, 130
    sig = signature(luma)
    assert sig[:64].sum() == 64 and sig[0] == 61 and sig[63] == 1 and sig[1] == 1 and sig[32] == 1
    assert sig[64 + 0] == 255 and sig[64 + 63] == 7 and sig[64 + 8 * 3 + 4] == 130 and sig[64:].sum() == 392
    # 10 x 14: cell columns begin at (i * 14) // 8 = 0 1 3 5 7 8 10 12, cell rows at (j * 10) // 8 = 0 1 2 3 5 6 7 8
    luma = np.arange(140, dtype=np.int64).reshape(10, 14)
    sig = signature(luma)
    assert sig[64 + 0] == 0                                                # one pixel
    assert sig[64 + 1] == (1 + 2 + 1) // 2                                 # pixels 1, 2 of row 0: (3 + 1) // 2
    assert sig[64 + 8 * 3 + 1] == (43 + 44 + 57 + 58 + 2) // 4             # rows 3, 4 x columns 1, 2
    assert sig[:64].sum() == 140 and sig[0] == 4 and sig[34] == 4


def test_first_same_and_cut_by_hand():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (16, 16)).astype(np.int64)
    ref = RefScene(2)
    assert ref.check(0, a) == (FIRST, 0, 0, 0)
    assert ref.check(0, a) == (SAME, 0, 0, 1)                              # the same frame twice
    assert ref.check(0, a) == (SAME, 0, 0, 2)
    assert ref.check(1, a) == (FIRST, 0, 0, 0)                             # the streams share nothing
    assert ref.check(0, a[:8, :12]) == (FIRST, 0, 0, 0)                    # a frame of another size
    assert ref.check(0, a[:8, :12]) == (SAME, 0, 0, 1)
    ref.forget(0)
    assert ref.check(0, a[:8, :12]) == (FIRST, 0, 0, 0) and ref.check(1, a) == (SAME, 0, 0, 1)
    ref = RefScene(1)
    ref.check(0, np.zeros((16, 16), np.int64))
    assert ref.check(0, np.full((16, 16), 255, np.int64)) == (CUT, 1000, 16320, 0)      # black, then white
    assert ref.check(0, np.full((16, 16), 255, np.int64)) == (SAME, 0, 0, 1)
    q = rng.integers(0, 64, (16, 16)).astype(np.int64)
    ref = RefScene(1)
    ref.check(0, 4 * q)
    assert ref.check(0, 4 * q + 3) == (SAME, 0, 192, 1)                    # no pixel leaves its bin, every cell mean rises by 3


def test_thresholds_by_hand():
    rng = np.random.default_rng(6)
    a, b = (rng.integers(0, 256, (16, 16)).astype(np.int64) for _ in range(2))
    ref = RefScene(1, 0, 0)
    assert ref.check(0, a)[0] == FIRST
    for frame in (b, b, a):                                                # thresholds 0, 0: every frame that is not the first is a CUT
        assert ref.check(0, frame)[0] == CUT and ref.run[0] == 0
    _, hist, grid, _ = run_scene([a, b], 1, 0, 0)[0][1, 0]
    assert 0 < hist <= 1000 and 0 < grid <= 16320
    for hi, gr, code in ((hist, grid, CUT), (hist + 1, grid, SAME), (hist, grid + 1, SAME), (hist, 0, CUT), (0, grid, CUT)):
        assert tuple(run_scene([a, b], 1, hi, gr)[0][1, 0]) == (code, hist, grid, 0 if code == CUT else 1)


@pytest.mark.parametrize("fmt", ("nv12", "bgr"))
def test_a_moved_view_is_the_same_scene_and_another_scene_is_a_cut(fmt):
    rng = np.random.default_rng(7)
    for h, w in SIZES[3:]:                                                 # below 76 x 102 random content proves nothing: constructed frames only
        a, b = moved_views(rng, fmt, h, w, ((0, 0), (4, 2)))
        lum = [luma_of((im.reshape(h, -1),), fmt) for im in (a, b)]
        code, hist, grid, run = run_scene(lum, 1)[0][1, 0]
        print("moved view %d x %d %s: hist %d grid %d" % (h, w, fmt, hist, grid))
        assert (code, run) == (SAME, 1) and hist < HIST
    for h, w in SIZES:
        lum = [luma_of((scene(rng, fmt, h, w, lo, hi).reshape(h, -1),), fmt) for lo, hi in ((0, 128), (128, 256))]
        code, hist, grid, run = run_scene(lum, 1)[0][1, 0]
        assert (code, hist, run) == (CUT, 1000, 0) and grid >= GRID, (h, w, grid)


def test_formats_are_the_followers():
    assert FORMATS == ("nv12", "nv21", "i420", "yv12", "bgr")

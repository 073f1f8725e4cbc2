"""Rotated sources through packed views (cf_forward_packed_rot, cf_op_packed_rot, cf_op_merge_packed_rot): what can be checked without a
GPU -- the declarations, the refusals that come before any device work with their named values (with no context at all, and through the
single-op forms), the Python layers' ValueErrors and option handling, the restatement of tests/packrot_cases.py against the one of
tests/rot_cases.py, and the words the documents owe."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import centerface_amd as cfa
from centerface_amd import ops
import csrc_text
from packrot_cases import ROTS, merge_packed_rot_ref, packed_rot_canvases_ref, upright_hw
from rot_cases import rot_geometry_ref, rot_ref, unrot_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "lightweight-face-detection-centernet_amd", "csrc")
L = cfa._lib
SYMBOLS = ("cf_forward_packed_rot", "cf_op_packed_rot", "cf_op_merge_packed_rot")


def _header():
    text = open(os.path.join(REPO, "include", "centerface_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


# ------------------------------------------------------------------------------------------ the declarations
def test_packrot_symbols_match_the_header():
    text, code = _header()
    lib = L.lib()
    for sym in SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % sym, code)
        assert m, sym
        assert sym in L.EXPORTS and hasattr(lib, sym)
        assert len(getattr(lib, sym).argtypes) == len(m.group(1).split(",")), sym      # the binding has the prototype's arity
    proto = lambda sym: re.sub(r"\s+", " ", re.search(r"\bint\s+%s\s*\(([^)]*)\)" % sym, code).group(1))      # noqa: E731
    # the prototypes are those of the unrotated forms with `int rot` behind the context / the device
    assert proto("cf_forward_packed_rot") == proto("cf_forward_packed").replace("cf_ctx* ctx, ", "cf_ctx* ctx, int rot, ")
    assert proto("cf_op_packed_rot") == proto("cf_op_packed").replace("int device, ", "int device, int rot, ")
    assert proto("cf_op_merge_packed_rot") == proto("cf_op_merge_packed").replace("int device, ", "int device, int rot, ")
    assert re.search(r"#define\s+CF_VERSION\s+100\b", text) and lib.cf_version() == 100      # nothing else moved


def test_the_rotated_kernels_have_a_file_of_their_own():
    texts = csrc_text.unit("cf_views_rot.hip")
    src = texts["cf_views_rot.hip"]
    assert "cut_packed_quarter_kernel" in src and "launch_cut_packed_quarter(" in src
    # rot 180 is the packed cutter's own kernel on mirrored taps; the turned rows go through the one collect kernel, the NMS stages unchanged
    views = open(os.path.join(CSRC, "cf_views.hip")).read()
    assert "cut_packed_kernel<SRC, VF, 2>" in views and "launch_cut_packed_quarter(" in views
    merge = csrc_text.unit("cf_tiles.hip")
    for rot in (1, 2, 3):
        assert "collect_rows_kernel<PlacedItems, %d>" % rot in merge["cf_tiles.hip"]
    assert "turn_point<ROT>" in merge["cf_collect.h"] and merge["cf_tiles.hip"].count("launch_nms_stages(") == 1
    assert not re.search(r"atomic", src, flags=re.I)                             # the list and the compaction are prefix sums
    csrc_text.assert_one_statement(texts, ())
    csrc_text.assert_one_statement(merge, ())
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bcf_views_rot\.hip\b", mk, flags=re.M)
    assert re.search(r"^EXTRA_cf_views_rot\s*=.*-ffp-contract=off", mk, flags=re.M)


def test_the_documents_state_what_is_built_and_its_limits():
    header = _header()[0]
    section = header[header.index("rotated sources through views and packed canvases"):header.index("face tracks across video frames")]
    docs = {"header": section}
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        docs[name] = open(os.path.join(REPO, name)).read()
    for name, text in docs.items():
        flat = re.sub(r"[\s*`]+", " ", text.lower())
        assert "cf_forward_packed_rot" in text, name
        at = [m.start() for m in re.finditer("cf_forward_packed_rot", flat)]
        near = " ".join(flat[max(0, p - 3000):p + 3000] for p in at)
        for word in ("mirrored", "one rot per call", "labels", "upright in the stored frame", "per canvas", "no accuracy claim", "stored frame"):
            assert word in near, (name, word)
        assert "no rotated views" not in flat, name                              # the old limit is reworded: it says where they live now
    assert "-0.0" in docs["header"] and "nms that the unfit does not" in re.sub(r"[\s*]+", " ", docs["header"].lower())
    assert "bit for bit" not in docs["header"][docs["header"].index("A single whole-frame placement"):docs["header"].index("Limits, plainly")]
    # the timing file holds the probe's table, or says plainly that there is none -- and then the README repeats that
    prof = open(os.path.join(REPO, "profiles", "pack_rot.md")).read()
    assert "packrot_probe.py" in prof
    measured = re.search(r"^\|.*rot\s*90.*\|\s*\d", prof, flags=re.M)
    assert measured or "not measured on an mi355x yet" in prof.lower()
    if not measured:
        flat = re.sub(r"\s+", " ", docs["README.md"].lower())
        assert any("not measured on an mi355x yet" in flat[max(0, m.start() - 1500):m.start() + 1500] for m in re.finditer("pack_rot.md", flat))
    assert os.path.exists(os.path.join(REPO, "tools", "packrot_probe.py"))


# ------------------------------------------------------------------------------------------ refusals before any device work
def _frames(Bf=1):
    buf = np.zeros(3 * 8192, np.uint8)
    tab = (L.YuvPlanes * max(Bf, 1))()
    for b in range(max(Bf, 1)):
        tab[b].y, tab[b].c0, tab[b].c1 = [buf.ctypes.data + 8192 * k for k in range(3)]
    return tab, buf


def _args(fmt=L.CF_FRAME_BGR, Bf=1, h=8, w=12, places=(), N=1):
    bgr, il = fmt == L.CF_FRAME_BGR, fmt in (L.CF_YUV_NV12, L.CF_YUV_NV21)
    tab, keep = _frames(Bf)
    pt, P = L.place_table(places)
    return (fmt, tab, Bf, h, w, 3 * w if bgr else w, 0 if bgr else w if il else w // 2, pt, P, N, L.fill_bytes((1, 2, 3))), keep


def _forward(rot, **kw):
    """cf_forward_packed_rot without a context: the arguments are checked all the same."""
    (fmt, tab, Bf, h, w, p0, p1, pt, P, N, fill), keep = _args(**kw)
    return L.lib().cf_forward_packed_rot(None, rot, fmt, tab, 0, Bf, h, w, p0, p1, pt, P, N, fill)


def _op(rot, H=8, W=8, **kw):
    (fmt, tab, Bf, h, w, p0, p1, pt, P, N, fill), keep = _args(**kw)
    canv = np.zeros((max(N, 1), H, W, 3), np.uint8)
    return L.lib().cf_op_packed_rot(0, rot, fmt, tab, Bf, h, w, p0, p1, pt, P, N, fill, H, W, L.ptr(canv))


def _merge(rot, places, N=1, Bf=1, h=8, w=12, H=8, W=8, rows=2, max_out=4):
    pt, P = L.place_table(places)
    d, s, l = np.zeros((N, rows, 4), np.float32), np.zeros((N, rows), np.float32), np.zeros((N, rows, 10), np.float32)
    od, ol = np.zeros((Bf, max_out, 5), np.float32), np.zeros((Bf, max_out, 10), np.float32)
    cn, oc, fl = (np.zeros(max(N, Bf), np.int32) for _ in range(3))
    o = L.merge_opts()
    return L.lib().cf_op_merge_packed_rot(0, rot, C.byref(o), pt, P, N, Bf, h, w, H, W, L.ptr(d), L.ptr(s), L.ptr(l), L.ptr(cn), rows, max_out, L.ptr(od),
                                          L.ptr(ol), L.ptr(oc), L.ptr(fl))


WHOLE_U = (0, 0, 0, 0, 8, 12, 0, 0, 4, 6)                # the whole upright view (8 wide, 12 high) of a stored 8 x 12 (h x w) frame at rot 90 / 270
INSIDE_F_ONLY = (0, 0, 0, 0, 12, 8, 0, 0, 4, 4)          # 12 wide, 8 high: inside the stored (h, w) = (8, 12), outside the upright (12, 8)


def test_refusals_name_their_value_with_no_context_and_through_the_ops():
    err = L.lib().cf_op_last_error
    calls = ((lambda rot, **kw: _forward(rot, **kw), b"cf_forward_packed_rot"), (lambda rot, **kw: _op(rot, **kw), b"cf_op_packed_rot"),
             (lambda rot, **kw: _merge(rot, kw["places"], **{k: v for k, v in kw.items() if k in ("N", "Bf", "h", "w")}), b"cf_op_merge_packed_rot"))
    for call, name in calls:
        # a rot outside the four
        for rot in (45, -90, 360, 1):
            assert call(rot, places=[WHOLE_U]) == -1, rot
            assert name in err() and b"rot=%d" % rot in err() and b"null context" not in err(), err()
        # an odd frame side, for BGR too
        for kw in (dict(h=7), dict(w=11)):
            assert call(90, places=[(0, 0, 0, 0, 2, 2, 0, 0, 1, 1)], **kw) == -1
            assert name in err() and b"even" in err(), err()
        # a source inside (h, w) but outside (hu, wu) at a quarter turn: refused, the upright view's size named; at 180 and 0 it is fine
        for rot in (90, 270):
            assert call(rot, places=[INSIDE_F_ONLY]) == -1
            msg = err()
            assert name in msg and b"placement 0" in msg and b"inside the frame" in msg and b"rot=%d" % rot in msg and b"UPRIGHT view, 8 x 12" in msg, msg
        # overlapping contents on one canvas: both indices
        assert call(90, places=[WHOLE_U, (0, 0, 0, 0, 2, 2, 3, 5, 2, 2)]) == -1
        assert name in err() and b"placements 0 and 1 overlap on canvas 0" in err(), err()
    # good arguments: only the context is missing; the upright rectangle is refused where the frame is NOT turned a quarter
    for rot in (90, 270):
        assert _forward(rot, places=[WHOLE_U]) == -1 and b"null context" in err(), err()
    for rot in (0, 180):
        assert _forward(rot, places=[INSIDE_F_ONLY]) == -1 and b"null context" in err(), err()
        assert _forward(rot, places=[WHOLE_U]) == -1 and b"inside the frame" in err(), err()
    for fmt in (L.CF_YUV_NV12, L.CF_YUV_YV12):
        assert _forward(270, fmt=fmt, places=[WHOLE_U]) == -1 and b"null context" in err(), err()
        assert _forward(270, fmt=fmt, h=6, w=10, places=[(0, 0, 2, 4, 4, 6, 1, 1, 3, 3)]) == -1 and b"null context" in err(), err()


def test_python_layers_refuse_and_pass_the_turn_on():
    img = np.zeros((1, 8, 12, 3), np.uint8)
    for call in (lambda: ops.cut_packed(img, [WHOLE_U], 1, (8, 8), rot=45), lambda: ops.cut_packed(img, [INSIDE_F_ONLY], 1, (8, 8), rot=90),
                 lambda: ops.merge_packed([WHOLE_U], 1, (8, 12), (8, 8), np.zeros((1, 2, 4)), np.zeros((1, 2)), np.zeros((1, 2, 10)), np.zeros((1,)), 4, rot=45),
                 lambda: ops.merge_packed([INSIDE_F_ONLY], 1, (8, 12), (8, 8), np.zeros((1, 2, 4)), np.zeros((1, 2)), np.zeros((1, 2, 10)), np.zeros((1,)), 4, rot=270)):
        with pytest.raises(ValueError) as e:
            call()
        assert "rot" in str(e.value)
    face = cfa.CenterFace.__new__(cfa.CenterFace)
    full = face._views_options(True)
    assert full == dict(scales=(1.0, 0.5), tile=None, overlap=None, anchor="center", fill=(0, 0, 0), metric="ios", thresh=0.5, edge=2.0)
    assert "rotate" not in face._views_options(dict(pack=True))                 # the key is in the result only when given
    assert face._views_options(dict(rotate=90)) == dict(full, rotate=90)
    assert face._views_options(dict(rotate=0)) == dict(full, rotate=0)
    assert face._views_options(dict(rotate=270, pack=True, gutter=3)) == dict(full, rotate=270, pack=True, gutter=3)
    for bad in (dict(rotate=45), dict(rotate=-90), dict(rotate="90"), dict(rotated=90)):
        with pytest.raises(ValueError):
            face._views_options(bad)
    frames = np.zeros((1, 8, 12, 3), np.uint8)
    # views= beside the top-level rotate= still raises, and points at the key; rotate= beside tiled= does not speak of views
    for call in (lambda: face.anonymize(frames, views=True, rotate=90), lambda: face.annotate(frames, views=dict(rotate=90), rotate=90),
                 lambda: face.best_shots(frames, tracker=None, shots=None, views=dict(pack=True), rotate=180),
                 lambda: face.detect_aligned_frames(frames, views=True, rotate=270)):
        with pytest.raises(ValueError) as e:
            call()
        assert "views" in str(e.value) and "rotate" in str(e.value) and "key" in str(e.value), e.value
    with pytest.raises(ValueError) as e:
        face.anonymize(frames, tiled=True, rotate=90)
    assert "rotate" in str(e.value) and "tiled" in str(e.value) and "views" not in str(e.value)
    for call in (lambda: face.detect_views(frames, rotate=45), lambda: face.anonymize(frames, views=dict(rotate=45)),
                 lambda: face.anonymize(frames, views=dict(rotate=90), tiled=True), lambda: face.anonymize(frames, views=dict(rotate=90), fit=True)):
        with pytest.raises(ValueError):
            call()
    from centerface_amd import demo
    with pytest.raises(SystemExit):                                              # the demo gets no new flag in this change
        demo.main(["nothing.png", "--scales", "1,0.5", "--rotate", "90"])


# ------------------------------------------------------------------------------------------ the restatements agree with each other
def test_restated_canvas_of_one_whole_frame_placement_is_the_restated_rotated_fit():
    rng = np.random.default_rng(3)
    H, W = 24, 32
    for hw in ((10, 30), (30, 10), (18, 24)):
        bgr = rng.integers(0, 256, (1,) + hw + (3,), dtype=np.uint8)
        for rot in ROTS:
            hu, wu = upright_hw(hw, rot)
            for stretch in (False, True):
                rw, rh, dx, dy = rot_geometry_ref(hw[0], hw[1], H, W, rot, stretch)
                got = packed_rot_canvases_ref(bgr, rot, [(0, 0, 0, 0, wu, hu, dx, dy, rw, rh)], 1, (H, W), (7, 8, 9))[0]
                want = rot_ref(bgr[0], rot, H, W, stretch, fill=(7, 8, 9)) if not stretch else rot_ref(bgr[0], rot, H, W, True)
                assert np.array_equal(got, want), (hw, rot, stretch)


def test_restated_merge_of_one_whole_frame_placement_is_the_restated_unrot_by_value():
    """Non-overlapping boxes, so the NMS keeps all of them: the rows of the placement form equal the unfit's by value (the `+ 0.0` may
    turn a -0.0 into +0.0: np.array_equal, not bytes), sorted by score."""
    frame, net = (40, 120), (64, 96)
    for rot in ROTS:
        geom = rot_geometry_ref(frame[0], frame[1], net[0], net[1], rot, False)
        rw, rh, dx, dy = geom
        hu, wu = upright_hw(frame, rot)
        boxes = [(dx + 1 + 5 * (k % 2), dy + 1 + 4 * (k // 2), dx + 4 + 5 * (k % 2), dy + 3 + 4 * (k // 2)) for k in range(6)]      # a 2 x 3 grid, disjoint
        assert rw >= 10 and rh >= 12
        d = np.zeros((1, 8, 4), np.float32)
        d[0, :len(boxes)] = boxes
        s = np.linspace(0.9, 0.4, 8, dtype=np.float32)[None]
        l = np.arange(80, dtype=np.float32).reshape(1, 8, 10) % 23 + dx
        c = np.array([len(boxes)], np.int32)
        a, af = merge_packed_rot_ref([(0, 0, 0, 0, wu, hu, dx, dy, rw, rh)], 1, frame, rot, d, s, l, c)
        b, bf = unrot_ref(geom, frame, rot, d, s, l, c)
        assert len(a[0][0]) == len(boxes) and af.tolist() == bf.tolist()
        assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1]), rot
